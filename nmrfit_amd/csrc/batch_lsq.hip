// batch_lsq.hip -- least squares over a device batch's resident spectra (include/nmrfit_amd_lsq.h, nmrfit_amd_lsq_im.h):
// the residual rows, Jacobian sums and normal equations of every fit at the caller's points, on one channel or on both.
// A part works through its fits in groups that fit the workspace budget (part_normal_equations, part_normal_group: the
// launches are lsq.hip's); the batch hands every part its share of the caller's arrays (batch_normal_equations), and the
// two nmrfit_batch_normal_equations* entry points differ in the channel count alone.  nmrfit_batch_sandwich
// (include/nmrfit_amd_cov.h) and nmrfit_batch_sandwich_im (include/nmrfit_amd_cov_im.h) are those calls with a Meat
// (batch_sandwich): the same groups, one more pair of launches on the rows and factors the group has just used
// (group_meat: one job per fit, on both channels four).  The swarms are not touched.
#include "batch_part.h"
#include "lsq_internal.h"
#include "nmrfit_amd_cov.h"
#include "nmrfit_amd_cov_im.h"

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <vector>

using namespace nmrfit;

// What nmrfit_batch_sandwich adds to a normal-equations call: the two channels' noise of every fit (K values each, like
// s) and where the meats go (laid out like A; both channels: [3][C x C] per fit, C = D + 1).  A part, then a group, sees
// its own share.
struct Meat {
    const double *sigma_u, *sigma_v;
    double *M_out;
};

// The meat of the fits [k0, k1) of a group (launch_lsq_meat): jobs are the group's LsqJobs, nch per fit (real first), whose
// R and c the meat jobs of the fit read; rows the group's parameter rows (the phase of row 0).  One more block of `mem`:
// [records | segments' sums | M].
static int group_meat(BatchPart *b, int32_t k0, int32_t k1, const LsqJob *jobs, const double *rows, const Meat &meat, int32_t Dmax,
                      int nch, Scratch &mem)
{
    const int32_t Kg = k1 - k0, per = lsq_meat_njobs(nch);
    int64_t n_partial = 0, n_M = 0;
    for (int32_t k = k0; k < k1; ++k) {
        n_partial += lsq_meat_partials(b->Nk[(size_t)k], b->D[(size_t)k], nch);
        n_M += meat_doubles(b->D[(size_t)k], nch);
    }
    const size_t mrec = align256((size_t)Kg * per * sizeof(LsqMeatJob)) / sizeof(double);
    double *d_meat = nullptr;
    NMRFIT_HIP(mem.alloc(&d_meat, mrec + (size_t)(n_partial + n_M)));
    double *d_partial = d_meat + mrec, *d_M = d_partial + n_partial;
    std::vector<LsqMeatJob> mjobs((size_t)Kg * per);
    int64_t at_p = 0, at_M = 0, at_x = 0;
    for (int32_t k = k0; k < k1; ++k) {
        const LsqJob &j = jobs[nch * (k - k0)];   // (the real channel's: its R is the first of the fit's planes)
        const int64_t D = j.D;
        lsq_meat_jobs(&mjobs[(size_t)(k - k0) * per], nch, j.R, j.c, b->h_fits[(size_t)k].wt, j.s, rows[at_x], rows[at_x + 1],
                      meat.sigma_u[k - k0], meat.sigma_v[k - k0], j.N, j.D, d_partial + at_p, d_M + at_M);
        at_p += lsq_meat_partials(j.N, D, nch);
        at_M += meat_doubles(D, nch);
        at_x += (D + 1) * D;
    }
    hipStream_t st = b->stream;
    // (pageable host memory: the copy has left `mjobs` when hipMemcpyAsync returns)
    NMRFIT_HIP(hipMemcpyAsync(d_meat, mjobs.data(), mjobs.size() * sizeof(LsqMeatJob), hipMemcpyHostToDevice, st));
    const int rc = launch_lsq_meat(st, reinterpret_cast<const LsqMeatJob *>(d_meat), per * Kg, Dmax, nch);
    if (rc != NMRFIT_OK) return rc;
    NMRFIT_HIP(hipMemcpyAsync(meat.M_out, d_M, (size_t)n_M * sizeof(double), hipMemcpyDeviceToHost, st));
    return NMRFIT_OK;
}

// include/nmrfit_amd_lsq.h for the fits [k0, k1) of a part: their residual rows in ONE launch over the part's resident
// spectra (lsq.hip, residual_rows_batch_kernel), J tile by tile and the segments' sums in a second, the ordered sums in
// a third.  rows, c, s and the outputs point at fit k0's share.  Everything the call allocates goes with `mem` on every
// path; the caller synchronises the stream before that when the enqueue failed half way.
// fit_im 1 or 2 (include/nmrfit_amd_lsq_im.h): rows of both channels -- nch = 2 planes of residual rows per fit, two jobs
// per fit (real, imaginary) in the same launches, and per fit [2][D x D] of A, [2][D] of g, the pair (rho_re, rho_im) of f.
static int part_normal_group(BatchPart *b, int32_t k0, int32_t k1, size_t lds, unsigned aux_off, const double *rows, const double *c,
                             const double *s, double *A_out, double *g_out, double *f_out, Scratch &mem, int fit_im,
                             const Meat *meat = nullptr)
{
    const int32_t Kg = k1 - k0;
    const bool sums = A_out || g_out;
    const int nch = fit_im ? 2 : 1;
    int64_t n_rows = 0, n_c = 0, n_f = 0, n_R = 0, n_partial = 0, n_A = 0, Smax = 0;
    int32_t Dmax = 0;
    for (int32_t k = k0; k < k1; ++k) {
        const int64_t D = b->D[(size_t)k], N = b->Nk[(size_t)k];
        int32_t nseg, seg_tiles;
        lsq_segments(N, &nseg, &seg_tiles);
        n_rows += (D + 1) * D;
        n_c += D;
        n_f += nch * (D + 1);
        n_R += nch * (D + 1) * N;
        n_partial += sums ? nch * nseg * lsq_sums(D) : 0;
        n_A += sums ? nch * D * D : 0;
        Smax = std::max(Smax, D + 1);
        Dmax = std::max(Dmax, (int32_t)D);
    }
    // one upload: the two record tables, the parameter rows, the factors
    const size_t rec_bytes = align256((size_t)Kg * (sizeof(RowsFit) + nch * sizeof(LsqJob)));
    const int64_t n_up = (int64_t)(rec_bytes / sizeof(double)) + n_rows + n_c;
    double *d_mem = nullptr;
    NMRFIT_HIP(mem.alloc(&d_mem, (size_t)(n_up + n_f + n_R + n_partial + n_A + nch * n_c)));
    RowsFit *d_fits = reinterpret_cast<RowsFit *>(d_mem);
    LsqJob *d_jobs = reinterpret_cast<LsqJob *>(d_fits + Kg);
    double *d_rows = d_mem + rec_bytes / sizeof(double), *d_c = d_rows + n_rows;
    double *d_f = d_mem + n_up, *d_R = d_f + n_f, *d_partial = d_R + n_R, *d_A = d_partial + n_partial, *d_g = d_A + n_A;
    std::vector<double> up((size_t)n_up);
    RowsFit *fits = reinterpret_cast<RowsFit *>(up.data());
    LsqJob *jobs = reinterpret_cast<LsqJob *>(fits + Kg);
    memcpy(up.data() + rec_bytes / sizeof(double), rows, (size_t)n_rows * sizeof(double));
    memcpy(up.data() + rec_bytes / sizeof(double) + n_rows, c, (size_t)n_c * sizeof(double));
    int64_t at_rows = 0, at_c = 0, at_f = 0, at_R = 0, at_partial = 0, at_A = 0;
    int32_t at_job = 0;
    for (int32_t k = k0; k < k1; ++k) {
        const BatchFit &f = b->h_fits[(size_t)k];
        const int64_t D = b->D[(size_t)k], N = f.N;
        RowsFit &q = fits[k - k0];
        q = RowsFit{};
        q.wc = f.wc;
        q.u = f.u;
        q.v = f.v;
        q.wt = f.wt;
        q.chunk = f.chunk;
        q.w0 = f.w0;
        q.wspan = f.wspan;
        q.lane_step = f.lane_step;
        q.rec_devk = f.rec_devk;
        q.X = d_rows + at_rows;
        q.f = d_f + at_f;
        q.R = d_R + at_R;
        q.N = N;
        q.seg_len = f.seg_len;
        q.S = D + 1;
        q.P = f.P;
        q.blk_chunks = f.blk_chunks;
        q.n_blocks = f.n_blocks;
        for (int ch = 0; ch < nch; ++ch) {   // a (fit, channel) pair is one job: the channel's plane of the rows
            LsqJob &j = jobs[at_job++];
            j = LsqJob{};
            j.R = q.R + ch * (D + 1) * N;
            j.c = d_c + at_c;
            j.s = s[k - k0];
            j.N = N;
            j.D = (int32_t)D;
            lsq_segments(N, &j.nseg, &j.seg_tiles);
            j.partial = sums ? d_partial + at_partial : nullptr;
            j.A = sums ? d_A + at_A : nullptr;
            j.g = sums ? d_g + nch * at_c + ch * D : nullptr;
            at_partial += sums ? j.nseg * lsq_sums(D) : 0;
            at_A += sums ? D * D : 0;
        }
        at_rows += (D + 1) * D;
        at_c += D;
        at_f += nch * (D + 1);
        at_R += nch * (D + 1) * N;
    }
    hipStream_t st = b->stream;
    // (pageable host memory: the copy has left `up` when hipMemcpyAsync returns)
    NMRFIT_HIP(hipMemcpyAsync(d_mem, up.data(), up.size() * sizeof(double), hipMemcpyHostToDevice, st));
    int rc = launch_rows_batch(st, d_fits, Kg, Smax, lds, aux_off, fit_im);
    if (rc != NMRFIT_OK) return rc;
    if (sums && (rc = launch_lsq(st, d_jobs, nch * Kg, Dmax, true)) != NMRFIT_OK) return rc;
    if (meat && meat->M_out && (rc = group_meat(b, k0, k1, jobs, rows, *meat, Dmax, nch, mem)) != NMRFIT_OK) return rc;
    if (A_out) NMRFIT_HIP(hipMemcpyAsync(A_out, d_A, (size_t)n_A * sizeof(double), hipMemcpyDeviceToHost, st));
    if (g_out) NMRFIT_HIP(hipMemcpyAsync(g_out, d_g, (size_t)(nch * n_c) * sizeof(double), hipMemcpyDeviceToHost, st));
    std::vector<double> fall(f_out ? (size_t)n_f : 0);
    if (f_out) NMRFIT_HIP(hipMemcpyAsync(fall.data(), d_f, (size_t)n_f * sizeof(double), hipMemcpyDeviceToHost, st));
    NMRFIT_HIP(hipStreamSynchronize(st));
    at_f = 0;
    for (int32_t k = k0; f_out && k < k1; ++k) {   // row 0's value of every fit (both channels: its pair)
        for (int ch = 0; ch < nch; ++ch) f_out[nch * (k - k0) + ch] = fall[(size_t)at_f + ch];
        at_f += nch * (b->D[(size_t)k] + 1);
    }
    return NMRFIT_OK;
}


static int part_normal_equations(BatchPart *b, const double *rows, const double *c, const double *s, double *A_out, double *g_out,
                                 double *f_out, int fit_im, const Meat *meat = nullptr)
{
    const int nch = fit_im ? 2 : 1;
    int rc = bind_batch(b);
    if (rc != NMRFIT_OK) return rc;
    if ((A_out || g_out) && 4 + 3 * (int64_t)b->Pmax > kLsqMaxD) {
        set_error("nmrfit_batch_normal_equations: A and g need D = 4 + 3 P <= " + std::to_string(kLsqMaxD) + " for every fit");
        return NMRFIT_E_UNSUPPORTED;
    }
    size_t lds = 0;
    unsigned aux_off = 0;
    if (!rows_batch_lds(b->Pmax, fit_im, &lds, &aux_off)) {
        set_error("nmrfit_batch_normal_equations: too many peaks for the residual kernel's LDS records in a batched launch");
        return NMRFIT_E_UNSUPPORTED;
    }
    // groups of consecutive fits whose residual rows fit the workspace budget (a fit larger than the budget runs alone)
    int64_t budget = (int64_t)256 << 17;   // doubles: 256 MiB
    if (const char *e = getenv("NMRFIT_LSQ_WORKSPACE_MB")) budget = std::max<int64_t>(1, atoll(e)) << 17;
    int64_t at_rows = 0, at_c = 0, at_A = 0, at_M = 0;
    for (int32_t k0 = 0; k0 < b->K && rc == NMRFIT_OK;) {
        int32_t k1 = k0;
        int64_t n_R = 0, d_rows = 0, d_c = 0, d_A = 0, d_M = 0;
        while (k1 < b->K) {
            const int64_t D = b->D[(size_t)k1], need = nch * (D + 1) * b->Nk[(size_t)k1];   // (both channels: the doubled rows)
            if (k1 > k0 && n_R + need > budget) break;
            n_R += need;
            d_rows += (D + 1) * D;
            d_c += D;
            d_A += nch * D * D;
            d_M += meat_doubles(D, nch);
            ++k1;
        }
        {
            Scratch mem;
            const Meat group{meat ? meat->sigma_u + k0 : nullptr, meat ? meat->sigma_v + k0 : nullptr,
                             meat && meat->M_out ? meat->M_out + at_M : nullptr};
            rc = part_normal_group(b, k0, k1, lds, aux_off, rows + at_rows, c + at_c, s + k0, A_out ? A_out + at_A : nullptr,
                                   g_out ? g_out + nch * at_c : nullptr, f_out ? f_out + nch * k0 : nullptr, mem, fit_im,
                                   meat ? &group : nullptr);
            if (rc != NMRFIT_OK) (void)hipStreamSynchronize(b->stream);   // what was enqueued may still use the buffers `mem` frees
        }
        at_rows += d_rows;
        at_c += d_c;
        at_A += d_A;
        at_M += d_M;
        k0 = k1;
    }
    return rc;
}

// Both entry points: a part's share of every array starts where the fits before it end -- rows [(D + 1) x D], c [D] and
// s [1] per fit, and nch channels of A [D x D], g [D] and f [1] (nch = 2: the batch's own fit_im says which imaginary model)
static int batch_normal_equations(nmrfit_batch *b, const char *who, int nch, const double *rows, const double *c, const double *s,
                                  double *A_out, double *g_out, double *f_out, const Meat *meat = nullptr)
{
    int rc = check_idle(b, who);
    int64_t at_rows = 0, at_A = 0, at_M = 0;
    for (size_t p = 0; p < b->parts.size() && rc == NMRFIT_OK; ++p) {
        const int32_t f0 = b->first[p], f1 = b->first[p + 1];
        const int64_t at_c = b->boff[(size_t)f0];
        const Meat part{meat ? meat->sigma_u + f0 : nullptr, meat ? meat->sigma_v + f0 : nullptr,
                        meat && meat->M_out ? meat->M_out + at_M : nullptr};
        rc = part_normal_equations(b->parts[p], rows + at_rows, c + at_c, s + f0, A_out ? A_out + nch * at_A : nullptr,
                                   g_out ? g_out + nch * at_c : nullptr, f_out ? f_out + nch * f0 : nullptr,
                                   nch == 2 ? b->parts[p]->fit_im : 0, meat ? &part : nullptr);
        for (int32_t k = f0; k < f1; ++k) {
            const int64_t D = b->boff[(size_t)k + 1] - b->boff[(size_t)k];
            at_rows += (D + 1) * D;
            at_A += D * D;
            at_M += meat_doubles(D, nch);
        }
    }
    return rc;
}

#pragma GCC visibility push(default)   // the C-ABI: the only symbols the library exports (build.sh: -fvisibility=hidden)
extern "C" {

int nmrfit_batch_normal_equations(nmrfit_batch *b, const double *rows, const double *c, const double *s, double *A_out,
                                  double *g_out, double *f_out)
{
    const int rc = check_batch_handle(b);
    if (rc != NMRFIT_OK) return rc;
    if (!rows || !c || !s) return refuse(NMRFIT_E_INVALID, "nmrfit_batch_normal_equations: null rows, c or s");
    return batch_normal_equations(b, "nmrfit_batch_normal_equations", 1, rows, c, s, A_out, g_out, f_out);
}

int nmrfit_batch_normal_equations_im(nmrfit_batch *b, const double *rows, const double *c, const double *s, double *A_out,
                                     double *g_out, double *f2_out)
{
    const int rc = check_batch_handle(b);
    if (rc != NMRFIT_OK) return rc;
    if (!rows || !c || !s) return refuse(NMRFIT_E_INVALID, "nmrfit_batch_normal_equations_im: null rows, c or s");
    const int fit_im = b->parts[0]->fit_im;   // (the same in every part)
    if (fit_im != NMRFIT_FIT_IM_REFERENCE && fit_im != NMRFIT_FIT_IM_SUM) {
        set_error("nmrfit_batch_normal_equations_im: the batch was created with fit_im = 0 (real part only): "
                  "nmrfit_batch_normal_equations is the call for it");
        return NMRFIT_E_INVALID;
    }
    return batch_normal_equations(b, "nmrfit_batch_normal_equations_im", 2, rows, c, s, A_out, g_out, f2_out);
}

// include/nmrfit_amd_cov.h and nmrfit_amd_cov_im.h.  Every refusal comes before the first launch: the batch is as it was.
static int batch_sandwich(nmrfit_batch *b, const char *who, int nch, const double *rows, const double *c, const double *s,
                          const double *sigma_u, const double *sigma_v, double *A_out, double *g_out, double *f_out, double *M_out)
{
    int rc = check_batch_handle(b);
    if (rc != NMRFIT_OK) return rc;
    if (!rows || !c || !s || !sigma_u || !sigma_v)
        return refuse(NMRFIT_E_INVALID, std::string(who) + ": null rows, c, s, sigma_u or sigma_v");
    for (int32_t k = 0; k < b->K; ++k)
        if ((rc = check_sigma(who, sigma_u[k], sigma_v[k])) != NMRFIT_OK) return rc;
    for (const BatchPart *p : b->parts) {
        if (nch == 1 && p->fit_im != NMRFIT_FIT_IM_OFF)
            return refuse(NMRFIT_E_UNSUPPORTED, "nmrfit_batch_sandwich: the batch was created with a fit_im mode: its fits minimise "
                                                "a mean of two norms, which this covariance does not describe");
        if (nch == 2 && p->fit_im != NMRFIT_FIT_IM_REFERENCE && p->fit_im != NMRFIT_FIT_IM_SUM)
            return refuse(NMRFIT_E_INVALID, "nmrfit_batch_sandwich_im: the batch was created with fit_im = 0 (real part only): "
                                            "nmrfit_batch_sandwich is the call for it");
        if (4 + 3 * (int64_t)p->Pmax > kLsqMaxD)
            return refuse(NMRFIT_E_UNSUPPORTED, std::string(who) + ": D = 4 + 3 P <= " + std::to_string(kLsqMaxD) + " for every fit");
    }
    const Meat meat{sigma_u, sigma_v, M_out};
    return batch_normal_equations(b, who, nch, rows, c, s, A_out, g_out, f_out, &meat);
}

int nmrfit_batch_sandwich(nmrfit_batch *b, const double *rows, const double *c, const double *s, const double *sigma_u,
                          const double *sigma_v, double *A_out, double *M_out, double *g_out, double *f_out)
{
    return batch_sandwich(b, "nmrfit_batch_sandwich", 1, rows, c, s, sigma_u, sigma_v, A_out, g_out, f_out, M_out);
}

int nmrfit_batch_sandwich_im(nmrfit_batch *b, const double *rows, const double *c, const double *s, const double *sigma_u,
                             const double *sigma_v, double *A_out, double *g_out, double *rho_out, double *M_out)
{
    return batch_sandwich(b, "nmrfit_batch_sandwich_im", 2, rows, c, s, sigma_u, sigma_v, A_out, g_out, rho_out, M_out);
}

}  // extern "C"
#pragma GCC visibility pop

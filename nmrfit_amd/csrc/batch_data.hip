// batch_data.hip -- what a device batch gives back and takes besides its swarms' results, all of it on the parts' resident
// arrays: the post-fit reconstruction of every fit (nmrfit_batch_contributions: enqueued per part, then copied back part
// after part), noise added in place to the resident spectra (nmrfit_batch_add_noise), a fit's spectrum as the kernels
// see it (nmrfit_batch_spectrum) and the residual statistics of every fit (nmrfit_batch_quality_stats).  The kernels are
// result.hip's, noise.hip's and quality.hip's.
#include "batch_part.h"
#include "nmrfit_amd_noise.h"
#include "noise_internal.h"
#include "quality_internal.h"
#include "result_internal.h"

#include <algorithm>
#include <vector>

using namespace nmrfit;

// FitUtility.generate_result (nmrfit/utils.py:226-295) for every fit of the part at its best position: ONE launch of the
// reconstruction kernel (result.hip) over the part's resident grids and best rows, enqueued on the part's stream;
// part_contributions_finish brings the arrays to the host (staged_d2h).  The host pointers are this part's shares.
static int part_contributions_enqueue(BatchPart *b, const int64_t *Nout, const double *w_out, double *real_out, double *imag_out,
                                      double *fit_out, double *data_out)
{
    int rc = bind_started(b, "nmrfit_batch_contributions");
    if (rc != NMRFIT_OK) return rc;
    if ((rc = flush_fold(b)) != NMRFIT_OK) return rc;   // (the tail launch leaves every fit's best row in d_bestx)
    const int32_t K = b->K;
    // per fit: output length n_k (its own grid's, or Nout[k]); rows of contributions P_k x n_k; 4 x n_k; 2 x N_k
    int64_t n_contrib = 0, n_fit = 0, n_w = 0, n_max = 0;
    for (int32_t k = 0; k < K; ++k) {
        const int64_t nk = w_out ? Nout[k] : b->Nk[(size_t)k];
        if (nk < 0) return refuse(NMRFIT_E_INVALID, "nmrfit_batch_contributions: negative output length");
        n_contrib += (int64_t)b->P[(size_t)k] * nk;
        n_fit += 4 * nk;
        n_w += w_out ? nk : 0;
        n_max = std::max(n_max, nk);
    }
    if (!real_out) n_contrib = 0;
    if (!fit_out) n_fit = 0;
    const int64_t n_data = data_out ? 2 * b->noff[(size_t)K] : 0;
    if (2 * n_contrib + n_fit + n_data == 0) return NMRFIT_OK;
    const size_t jobs_bytes = align256((size_t)K * sizeof(ResultJob));
    NMRFIT_HIP(device_alloc(&b->d_result, jobs_bytes + (size_t)(n_w + 2 * n_contrib + n_fit + n_data) * sizeof(double)));
    unsigned char *base = reinterpret_cast<unsigned char *>(b->d_result);
    double *d_w = reinterpret_cast<double *>(base + jobs_bytes);
    double *d_real = d_w + n_w, *d_imag = d_real + n_contrib, *d_fit = d_imag + n_contrib, *d_data = d_fit + n_fit;
    std::vector<ResultJob> jobs((size_t)K);
    int64_t at_contrib = 0, at_fit = 0, at_w = 0;
    for (int32_t k = 0; k < K; ++k) {
        const BatchFit &f = b->h_fits[(size_t)k];
        const int64_t nk = w_out ? Nout[k] : f.N;
        ResultJob &j = jobs[(size_t)k];
        j = ResultJob{};
        j.wc = f.wc;
        j.w_plain = w_out ? d_w + at_w : nullptr;
        j.x = b->d_bestx + b->boff[(size_t)k];
        j.u = f.u;
        j.v = f.v;
        j.w0 = f.w0;
        j.wspan = f.wspan;
        j.Nout = nk;
        j.N = f.N;
        j.P = f.P;
        j.real = real_out ? d_real + at_contrib : nullptr;
        j.imag = real_out ? d_imag + at_contrib : nullptr;
        j.fit = fit_out ? d_fit + at_fit : nullptr;
        j.data = data_out ? d_data + 2 * b->noff[(size_t)k] : nullptr;
        at_contrib += (int64_t)f.P * nk;
        at_fit += 4 * nk;
        at_w += w_out ? nk : 0;
    }
    hipStream_t st = b->stream;
    // (pageable host memory: the copy has left `jobs` when hipMemcpyAsync returns)
    NMRFIT_HIP(hipMemcpyAsync(base, jobs.data(), (size_t)K * sizeof(ResultJob), hipMemcpyHostToDevice, st));
    if (n_w) NMRFIT_HIP(hipMemcpyAsync(d_w, w_out, (size_t)n_w * sizeof(double), hipMemcpyHostToDevice, st));
    if ((rc = launch_result_jobs(st, reinterpret_cast<const ResultJob *>(base), K, std::max(n_max, data_out ? b->Nmax : 0), b->Pmax)) != NMRFIT_OK)
        return rc;
    // what goes where on the host, for part_contributions_finish (the copies are staged and synchronous: they would
    // serialise the parts' launches if they were made here)
    b->result_copies.clear();
    if (n_contrib) {
        b->result_copies.push_back({real_out, d_real, (size_t)n_contrib * sizeof(double)});
        b->result_copies.push_back({imag_out, d_imag, (size_t)n_contrib * sizeof(double)});
    }
    if (n_fit) b->result_copies.push_back({fit_out, d_fit, (size_t)n_fit * sizeof(double)});
    if (n_data) b->result_copies.push_back({data_out, d_data, (size_t)n_data * sizeof(double)});
    return NMRFIT_OK;
}

static int part_contributions_finish(BatchPart *b)
{
    if (!b->d_result) return NMRFIT_OK;
    (void)hipSetDevice(b->device);
    int rc = NMRFIT_OK;
    for (const BatchPart::ResultCopy &c : b->result_copies)
        if (rc == NMRFIT_OK) rc = staged_d2h(b->device, b->stream, c.host, c.dev, c.bytes);
    b->result_copies.clear();
    const hipError_t e = hipStreamSynchronize(b->stream);
    (void)hipFree(b->d_result);
    b->d_result = nullptr;
    if (rc == NMRFIT_OK && e != hipSuccess) rc = hip_fail(e, "hipStreamSynchronize(reconstruction)", __FILE__, __LINE__);
    return rc;
}

// include/nmrfit_amd_noise.h for the fits of a part: one launch of the noise kernel (noise.hip) on the part's stream, in
// place on the resident u and v planes -- point j at grid_slot(j), j < N_k: the padding stays zero.  Nothing else of a
// BatchFit depends on u or v (w0, wspan, lane_step, rec_devk and the chunk table are the grid's).  sigma_u, sigma_v,
// seed: this part's shares, already checked.  The job table goes with `mem`; the caller synchronises.
static int part_add_noise_enqueue(BatchPart *b, const double *sigma_u, const double *sigma_v, const uint64_t *seed, Scratch &mem)
{
    int rc = bind_batch(b);
    if (rc != NMRFIT_OK) return rc;
    std::vector<NoiseJob> jobs((size_t)b->K);
    for (int32_t k = 0; k < b->K; ++k) {
        const BatchFit &f = b->h_fits[(size_t)k];
        double *u = const_cast<double *>(f.u), *v = const_cast<double *>(f.v);
        jobs[(size_t)k] = NoiseJob{u, v, u, v, f.N, sigma_u[k], sigma_v[k], seed[k]};
    }
    NoiseJob *d_jobs = nullptr;
    NMRFIT_HIP(mem.alloc(&d_jobs, jobs.size()));
    // (pageable host memory: the copy has left `jobs` when hipMemcpyAsync returns)
    NMRFIT_HIP(hipMemcpyAsync(d_jobs, jobs.data(), jobs.size() * sizeof(NoiseJob), hipMemcpyHostToDevice, b->stream));
    return launch_noise(b->stream, d_jobs, b->K, b->Nmax, true);
}

// the two planes of fit k as the kernels see them, back in grid order (the inverse of batch_prepare_kernel's scatter)
static int part_spectrum(BatchPart *b, int32_t k, double *u_out, double *v_out)
{
    int rc = bind_batch(b);
    if (rc != NMRFIT_OK) return rc;
    const BatchFit &f = b->h_fits[(size_t)k];
    Scratch mem;
    double *d_out = nullptr;   // [2][N]
    const size_t n = (size_t)f.N;
    NMRFIT_HIP(mem.alloc(&d_out, 2 * n));
    rc = launch_noise_gather(b->stream, f.u, f.v, f.N, d_out, d_out + n);
    if (rc == NMRFIT_OK && u_out) rc = staged_d2h(b->device, b->stream, u_out, d_out, n * sizeof(double));
    if (rc == NMRFIT_OK && v_out) rc = staged_d2h(b->device, b->stream, v_out, d_out + n, n * sizeof(double));
    const hipError_t e = hipStreamSynchronize(b->stream);   // (before `mem` frees what the launch writes)
    if (rc == NMRFIT_OK && e != hipSuccess) rc = hip_fail(e, "hipStreamSynchronize(spectrum)", __FILE__, __LINE__);
    return rc;
}

// include/nmrfit_amd_quality.h for the fits of a part: the three launches of quality.hip on the part's stream, over the
// resident planes (grid_slot order) and, for the regions' nearest points, the grids as they were uploaded.  x: this
// part's parameter vectors (host), or null: the best rows -- the part must have started, and a generation whose fold
// still waits is folded first, as for the reconstruction.  R, edges: this part's shares, already checked.  *d_out: the
// part's rows in device memory (n_rows of them); the caller copies and synchronises.  The launches' buffers are one
// block that stays with the part (d_quality, grown on demand, freed with the part): a hipFree per call would wait for
// whatever the other batches of a fit_many call have queued on the device.
static int part_quality_enqueue(BatchPart *b, const double *x, const int32_t *R, const double *edges, double **d_out,
                                int64_t *n_rows)
{
    int rc = x ? bind_batch(b) : bind_started(b, "nmrfit_batch_quality_stats");
    if (rc != NMRFIT_OK) return rc;
    if (!x && (rc = flush_fold(b)) != NMRFIT_OK) return rc;   // (the tail launch leaves every fit's best row in d_bestx)
    const int32_t K = b->K;
    std::vector<WeightSpec> specs;
    std::vector<int32_t> region_spec;
    weights_layout(K, b->Nk.data(), R, &specs, &region_spec);
    int64_t rows = 0, n_partial = 0;
    int32_t Rmax = 0;
    for (int32_t k = 0; k < K; ++k) {
        rows += R[k] + 2;
        n_partial += (int64_t)(R[k] + 2) * quality_tiles(b->Nk[(size_t)k]);
        Rmax = std::max(Rmax, R[k]);
    }
    const size_t nr = region_spec.size();
    Carver c;
    const size_t o_jobs = c.take((size_t)K * sizeof(QualityJob)), o_specs = c.take(specs.size() * sizeof(WeightSpec));
    const size_t o_rs = c.take(nr * sizeof(int32_t)), o_fl = c.take(2 * nr * sizeof(int64_t)), o_edges = c.take(2 * nr * sizeof(double));
    const size_t o_partial = c.take((size_t)n_partial * kQualityRow * sizeof(double));
    const size_t o_out = c.take((size_t)rows * kQualityRow * sizeof(double)), o_x = c.take(x ? (size_t)b->Dsum * sizeof(double) : 0);
    if (b->cap_quality < c.total) {
        if (b->d_quality) (void)hipFree(b->d_quality);
        b->d_quality = nullptr;
        b->cap_quality = 0;
        NMRFIT_HIP(device_alloc(&b->d_quality, c.total));
        b->cap_quality = c.total;
    }
    unsigned char *base = reinterpret_cast<unsigned char *>(b->d_quality);
    QualityJob *d_jobs = reinterpret_cast<QualityJob *>(base + o_jobs);
    WeightSpec *d_specs = reinterpret_cast<WeightSpec *>(base + o_specs);
    int32_t *d_rs = reinterpret_cast<int32_t *>(base + o_rs);
    int64_t *d_fl = reinterpret_cast<int64_t *>(base + o_fl);
    double *d_edges = reinterpret_cast<double *>(base + o_edges), *d_partial = reinterpret_cast<double *>(base + o_partial);
    double *d_x = reinterpret_cast<double *>(base + o_x);
    *d_out = reinterpret_cast<double *>(base + o_out);
    std::vector<QualityJob> jobs((size_t)K);
    int64_t at_row = 0, at_partial = 0;
    for (int32_t k = 0; k < K; ++k) {
        const BatchFit &f = b->h_fits[(size_t)k];
        QualityJob &j = jobs[(size_t)k];
        j = QualityJob{};
        j.w = f.wc;
        j.u = f.u;
        j.v = f.v;
        j.x = (x ? d_x : b->d_bestx) + b->boff[(size_t)k];
        j.first_last = d_fl + 2 * specs[(size_t)k].r_off;
        j.partial = d_partial + at_partial * kQualityRow;
        j.out = *d_out + at_row * kQualityRow;
        j.w0 = f.w0;
        j.wspan = f.wspan;
        j.N = f.N;
        j.P = f.P;
        j.R = R[k];
        j.tiles = (int32_t)quality_tiles(f.N);
        j.slotted = 1;
        at_row += R[k] + 2;
        at_partial += (int64_t)(R[k] + 2) * j.tiles;
    }
    hipStream_t st = b->stream;
    // (pageable host memory: the copies have left the host arrays when hipMemcpyAsync returns)
    NMRFIT_HIP(hipMemcpyAsync(d_jobs, jobs.data(), jobs.size() * sizeof(QualityJob), hipMemcpyHostToDevice, st));
    NMRFIT_HIP(hipMemcpyAsync(d_specs, specs.data(), specs.size() * sizeof(WeightSpec), hipMemcpyHostToDevice, st));
    if (x) NMRFIT_HIP(hipMemcpyAsync(d_x, x, (size_t)b->Dsum * sizeof(double), hipMemcpyHostToDevice, st));
    if (nr) {
        NMRFIT_HIP(hipMemcpyAsync(d_rs, region_spec.data(), nr * sizeof(int32_t), hipMemcpyHostToDevice, st));
        NMRFIT_HIP(hipMemcpyAsync(d_edges, edges, 2 * nr * sizeof(double), hipMemcpyHostToDevice, st));
    }
    *n_rows = rows;
    return launch_quality(st, d_jobs, K, quality_tiles(b->Nmax), b->Pmax, Rmax, d_specs, d_rs, (int64_t)nr, b->d_w_plain, d_edges, d_fl);
}

#pragma GCC visibility push(default)   // the C-ABI: the only symbols the library exports (build.sh: -fvisibility=hidden)
extern "C" {

int nmrfit_batch_contributions(nmrfit_batch *b, const int64_t *Nout, const double *w_out, double *real_out, double *imag_out,
                               double *fit_out, double *data_out)
{
    int rc = check_batch_handle(b);
    if (rc != NMRFIT_OK) return rc;
    if ((w_out != nullptr) != (Nout != nullptr) || (!real_out != !imag_out)) {
        set_error("nmrfit_batch_contributions: Nout and w_out together or not at all; real_out and imag_out likewise");
        return NMRFIT_E_INVALID;
    }
    if ((rc = check_idle(b, "nmrfit_batch_contributions")) != NMRFIT_OK) return rc;
    // every part enqueues its launch on its own stream, then the copies back are made part after part.  A part's share of
    // each output starts where the fits before it end.
    int64_t at_contrib = 0, at_fit = 0, at_w = 0;
    for (size_t p = 0; p < b->parts.size() && rc == NMRFIT_OK; ++p) {
        BatchPart *q = b->parts[p];
        const int32_t f0 = b->first[p], f1 = b->first[p + 1];
        rc = part_contributions_enqueue(q, Nout ? Nout + f0 : nullptr, w_out ? w_out + at_w : nullptr,
                                        real_out ? real_out + at_contrib : nullptr, imag_out ? imag_out + at_contrib : nullptr,
                                        fit_out ? fit_out + at_fit : nullptr, data_out ? data_out + 2 * b->noff[(size_t)f0] : nullptr);
        for (int32_t k = f0; k < f1; ++k) {
            const int64_t nk = Nout ? std::max<int64_t>(Nout[k], 0) : b->noff[(size_t)k + 1] - b->noff[(size_t)k];
            at_contrib += (b->prow[(size_t)k + 1] - b->prow[(size_t)k]) * nk;
            at_fit += 4 * nk;
            at_w += Nout ? nk : 0;
        }
    }
    for (BatchPart *q : b->parts) {
        const int rc2 = part_contributions_finish(q);
        if (rc == NMRFIT_OK) rc = rc2;
    }
    return rc;
}

int nmrfit_batch_add_noise(nmrfit_batch *b, const double *sigma_u, const double *sigma_v, const uint64_t *seed)
{
    int rc = check_batch_handle(b);
    if (rc != NMRFIT_OK) return rc;
    if ((rc = check_noise_args("nmrfit_batch_add_noise", b->K, sigma_u, sigma_v, seed)) != NMRFIT_OK) return rc;
    for (const BatchPart *q : b->parts)
        if (q->initialized || q->noised) {
            set_error(q->noised ? "nmrfit_batch_add_noise: noise was already added to this batch"
                                : "nmrfit_batch_add_noise after the first generation");
            return NMRFIT_E_STATE;
        }
    if ((rc = check_idle(b, "nmrfit_batch_add_noise")) != NMRFIT_OK) return rc;
    // From here on the batch counts as perturbed, every part of it: should a part's launch fail, the others may have run, the
    // spectra are then neither the upload nor the replica, and a second call must not add noise to the parts that did.
    for (BatchPart *q : b->parts) q->noised = true;
    // every part enqueues its launch on its own stream; then all are waited for (the job tables go with `mem` after that)
    Scratch mem;
    for (size_t p = 0; p < b->parts.size() && rc == NMRFIT_OK; ++p) {
        const int32_t f0 = b->first[p];
        rc = part_add_noise_enqueue(b->parts[p], sigma_u + f0, sigma_v + f0, seed + f0, mem);
    }
    for (BatchPart *q : b->parts) {
        const hipError_t e = hipStreamSynchronize(q->stream);
        if (rc == NMRFIT_OK && e != hipSuccess) rc = hip_fail(e, "hipStreamSynchronize(noise)", __FILE__, __LINE__);
    }
    return rc;
}

int nmrfit_batch_spectrum(nmrfit_batch *b, int32_t k, double *u_out, double *v_out)
{
    int rc = check_batch_handle(b);
    if (rc != NMRFIT_OK) return rc;
    if (k < 0 || k >= b->K) return refuse(NMRFIT_E_INVALID, "nmrfit_batch_spectrum: fit index out of range");
    const int q = part_of(b, k);
    return part_spectrum(b->parts[(size_t)q], k - b->first[(size_t)q], u_out, v_out);
}

int nmrfit_batch_quality_stats(nmrfit_batch *b, const double *x, const int32_t *R, const double *edges, double *out)
{
    const char *who = "nmrfit_batch_quality_stats";
    int rc = check_batch_handle(b);
    if (rc != NMRFIT_OK) return rc;
    if (!out) return refuse(NMRFIT_E_INVALID, std::string(who) + ": null pointer");
    std::vector<int64_t> N((size_t)b->K);
    for (int32_t k = 0; k < b->K; ++k) N[(size_t)k] = b->noff[(size_t)k + 1] - b->noff[(size_t)k];
    int64_t n_points = 0, n_regions = 0;
    if ((rc = check_quality_args(who, b->K, N.data(), R, edges, &n_points, &n_regions)) != NMRFIT_OK) return rc;
    if (!x && (rc = check_idle(b, who)) != NMRFIT_OK) return rc;
    // every part enqueues its launches on its own stream; then the rows come back part after part and all streams are
    // waited for.  A part's share of x, R, edges and out starts where the fits before it end.
    std::vector<double *> d_rows(b->parts.size(), nullptr);
    std::vector<int64_t> n_rows(b->parts.size(), 0);
    int64_t r0 = 0;
    for (size_t p = 0; p < b->parts.size() && rc == NMRFIT_OK; ++p) {
        const int32_t f0 = b->first[p], f1 = b->first[p + 1];
        rc = part_quality_enqueue(b->parts[p], x ? x + b->boff[(size_t)f0] : nullptr, R + f0, edges ? edges + 2 * r0 : nullptr, &d_rows[p],
                                  &n_rows[p]);
        for (int32_t k = f0; k < f1; ++k) r0 += R[k];
    }
    int64_t at = 0;
    for (size_t p = 0; p < b->parts.size(); ++p) {
        BatchPart *q = b->parts[p];
        if (rc == NMRFIT_OK)
            rc = staged_d2h(q->device, q->stream, out + at * kQualityRow, d_rows[p], (size_t)n_rows[p] * kQualityRow * sizeof(double));
        at += n_rows[p];
        const hipError_t e = hipStreamSynchronize(q->stream);
        if (rc == NMRFIT_OK && e != hipSuccess) rc = hip_fail(e, "hipStreamSynchronize(quality)", __FILE__, __LINE__);
    }
    return rc;
}

}  // extern "C"
#pragma GCC visibility pop

// lsq_analytic.hip -- the analytic Jacobian of the real-channel residual on the device
// (include/nmrfit_amd_lsq_analytic.h): J, r and the normal equations A = J^T J, g = J^T r, f = ||r|| of a
// fit in ONE pass over its resident spectrum, without residual rows.  lsq_analytic_kernel is lsq_normal_kernel (lsq.hip)
// with another form stage: the tile of [J | r] comes from closed forms of the pseudo-Voigt residual's derivatives
// (lsq_tile.h, lsq_form_analytic) instead of from differences of D + 1 rows; the write-out, the accumulation and the
// segments' sums are the same stages, called.  The sums carry one more entry, the pair (D, D) = sum_j r_j^2, whose root
// is f.  No atomics: every order is fixed by N and P alone.  No objective kernel is launched here: the kernel variant a
// context is set to does not matter.
//
// The host side of the two entry points is here too: the refusal of points at which the model is not differentiable in
// the library's own sense (a width of zero or below the kernels' floor, a non-finite parameter) before any launch, one
// upload and two launches per context call or per group of a batch part.
#include "batch_part.h"
#include "lsq_tile.h"
#include "nmrfit_amd_lsq_analytic.h"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <vector>

namespace nmrfit {
namespace {

__global__ __launch_bounds__(kLsqThreads) void lsq_analytic_kernel(const LsqAnalyticJob *__restrict__ jobs)
{
    extern __shared__ double T[];   // [kLsqTile][pitch] | head [kLsqHead] | the peaks' constants [P] | the strips [2][kLsqWaves][kLsqTile]
    const LsqAnalyticJob &q = jobs[blockIdx.y];
    if ((int)blockIdx.x >= q.nseg) return;   // (a batch's launch is as wide as its longest grid needs)
    const int D = q.D, pitch = (D + 1) | 1;
    const int64_t N = q.N;
    const int tid = threadIdx.x, jl = tid & (kLsqTile - 1);
    const int i0 = __builtin_amdgcn_readfirstlane(tid >> 6);   // (one value per wave: see lsq_normal_kernel)
    double *head = T + kLsqTile * pitch;
    LsqPeakConst *pk = reinterpret_cast<LsqPeakConst *>(head + kLsqHead);
    double *strip = reinterpret_cast<double *>(pk + q.P);
    lsq_peak_consts(head, pk, q.x, q.P, q.w0, q.s, N);
    const LsqResident g = lsq_resident(q);
    const bool sums = q.partial != nullptr;
    const int nout = sums ? D * (D + 1) / 2 + D + 1 : 0;   // (the last entry: lsq_pair gives it the pair (D, D))
    int pa[kLsqAcc], pb[kLsqAcc];
    double acc[kLsqAcc];
    lsq_own_pairs(nout, [D](int o, int *a, int *b) { lsq_pair(o, D, a, b); }, pa, pb, acc);
    int64_t t0, t1;
    lsq_tile_range(N, q.seg_tiles, &t0, &t1);
    __syncthreads();
    for (int t = (int)t0; t < (int)t1; ++t) {   // (tiles count in 32 bits: N < 2^37)
        const int64_t j0 = (int64_t)t * kLsqTile;
        const int nj = (int)((N - j0 < kLsqTile) ? N - j0 : kLsqTile);
        const bool have = jl < nj;
        lsq_form_analytic(T, pitch, strip, head, pk, q, g, j0, have, i0);
        __syncthreads();
        lsq_write_tile(T, pitch, g, D, j0, nj, have, i0, jl);
        if (sums) lsq_accumulate<false>(T, pitch, T, pitch, nullptr, nj, pa, pb, acc);
        __syncthreads();
    }
    // (nout again as a value the compiler has not seen: otherwise it keeps the twelve `o < nout` masks of lsq_own_pairs in
    // scalar registers across the tile loop for this store, and parks other scalars in vector lanes to make room)
    int nout_store = nout;
    asm volatile("" : "+s"(nout_store));
    if (sums) lsq_store_partial(g.partial, nout_store, acc);
}

// the segments' sums one after the other, segment 0 first; A comes back whole (both triangles from the same sum)
__global__ __launch_bounds__(kLsqThreads) void lsq_analytic_reduce_kernel(const LsqAnalyticJob *__restrict__ jobs)
{
    const LsqAnalyticJob &q = jobs[blockIdx.x];
    if (!q.partial) return;
    const int D = q.D, nout = D * (D + 1) / 2 + D + 1;
    for (int o = threadIdx.x; o < nout; o += kLsqThreads) {
        const double sum = lsq_segment_sum(q.partial, q.nseg, nout, o);
        int a, b;
        lsq_pair(o, D, &a, &b);
        if (a == D) {
            if (q.f) q.f[0] = sqrt(sum);
        } else if (b == D) {
            if (q.g) q.g[a] = sum;
        } else if (q.A) {
            q.A[a * D + b] = sum;
            q.A[b * D + a] = sum;
        }
    }
}

}  // namespace

int launch_lsq_analytic(hipStream_t st, const LsqAnalyticJob *d_jobs, int32_t K, int32_t Dmax, bool sums)
{
    if (K <= 0) return NMRFIT_OK;
    if (Dmax > kLsqMaxD) {
        set_error("analytic Jacobian: D = 4 + 3 P above " + std::to_string(kLsqMaxD));
        return NMRFIT_E_UNSUPPORTED;
    }
    const size_t lds = ((size_t)kLsqTile * (size_t)((Dmax + 1) | 1) + (size_t)lsq_analytic_extra((Dmax - 4) / 3)) * sizeof(double);
    hipLaunchKernelGGL(lsq_analytic_kernel, dim3((unsigned)kLsqMaxSegments, (unsigned)K), dim3(kLsqThreads), lds, st, d_jobs);
    NMRFIT_HIP(hipGetLastError());
    if (sums) {
        hipLaunchKernelGGL(lsq_analytic_reduce_kernel, dim3((unsigned)K), dim3(kLsqThreads), 0, st, d_jobs);
        NMRFIT_HIP(hipGetLastError());
    }
    return NMRFIT_OK;
}

}  // namespace nmrfit

using namespace nmrfit;

static_assert(sizeof(LsqAnalyticJob) % sizeof(double) == 0, "a job follows the parameters in a buffer of doubles");
constexpr int64_t kJobDoubles = sizeof(LsqAnalyticJob) / sizeof(double);

// Where the model is not differentiable in the library's own sense, the call is refused: a parameter that is not finite,
// a width of zero or below the kernels' floor (|2 / width| > 1e18 / (wspan + |loc - w0|): the objective kernels evaluate
// the line of the floor width there, which does not move with the width).  `fit` < 0: a lone context.
static int check_point(const char *who, int64_t fit, int32_t P, const double *x, double w0, double wspan)
{
    const std::string where = std::string(who) + (fit >= 0 ? ": fit " + std::to_string(fit) : std::string()) + ": ";
    for (int64_t i = 0; i < 4 + 3 * (int64_t)P; ++i)
        if (!std::isfinite(x[i])) return refuse(NMRFIT_E_INVALID, where + "parameter " + std::to_string(i) + " is not finite");
    for (int32_t k = 0; k < P; ++k) {
        const double width = x[4 + 3 * k], loc = x[5 + 3 * k];
        const double lim = 1.0e18 / (wspan + std::fabs(loc - w0));
        if (width == 0.0 || std::fabs(2.0 / width) > lim)
            return refuse(NMRFIT_E_INVALID, where + "peak " + std::to_string(k) + ": its width is zero or below the kernels' floor, "
                                                                                 "where the model does not move with the width");
    }
    return NMRFIT_OK;
}

// The fits [k0, k1) of a part: one upload (the records and the points), the two launches, the copies back.  x and the
// outputs point at fit k0's share.  Everything the call allocates goes with `mem` on every path; the caller synchronises
// the stream before that when the enqueue failed half way.
static int part_analytic_group(BatchPart *b, int32_t k0, int32_t k1, const double *x, double *A_out, double *g_out, double *f_out,
                               Scratch &mem)
{
    const int32_t Kg = k1 - k0;
    int64_t n_x = 0, n_partial = 0, n_A = 0;
    int32_t Dmax = 0;
    for (int32_t k = k0; k < k1; ++k) {
        const int64_t D = b->D[(size_t)k];
        int32_t nseg, seg_tiles;
        lsq_segments(b->Nk[(size_t)k], &nseg, &seg_tiles);
        n_x += D;
        n_partial += nseg * lsq_sums_analytic(D);
        n_A += D * D;
        Dmax = std::max(Dmax, (int32_t)D);
    }
    const size_t rec = align256((size_t)Kg * sizeof(LsqAnalyticJob)) / sizeof(double);
    const int64_t n_up = (int64_t)rec + n_x;
    double *d_mem = nullptr;
    NMRFIT_HIP(mem.alloc(&d_mem, (size_t)(n_up + n_partial + n_A + n_x + Kg)));
    double *d_x = d_mem + rec, *d_partial = d_mem + n_up, *d_A = d_partial + n_partial, *d_g = d_A + n_A, *d_f = d_g + n_x;
    std::vector<double> up((size_t)n_up);
    LsqAnalyticJob *jobs = reinterpret_cast<LsqAnalyticJob *>(up.data());
    memcpy(up.data() + rec, x, (size_t)n_x * sizeof(double));
    int64_t at_x = 0, at_partial = 0, at_A = 0;
    for (int32_t k = k0; k < k1; ++k) {
        const BatchFit &f = b->h_fits[(size_t)k];
        const int64_t D = b->D[(size_t)k];
        LsqAnalyticJob &j = jobs[k - k0];
        j = LsqAnalyticJob{};
        j.wc = f.wc;
        j.u = f.u;
        j.v = f.v;
        j.wt = f.wt;
        j.x = d_x + at_x;
        j.w0 = f.w0;
        j.s = 1.0 / std::sqrt((double)f.N);
        j.N = f.N;
        j.P = f.P;
        j.D = (int32_t)D;
        lsq_segments(f.N, &j.nseg, &j.seg_tiles);
        j.partial = d_partial + at_partial;
        j.A = d_A + at_A;
        j.g = d_g + at_x;
        j.f = d_f + (k - k0);
        at_x += D;
        at_partial += j.nseg * lsq_sums_analytic(D);
        at_A += D * D;
    }
    hipStream_t st = b->stream;
    // (pageable host memory: the copy has left `up` when hipMemcpyAsync returns)
    NMRFIT_HIP(hipMemcpyAsync(d_mem, up.data(), up.size() * sizeof(double), hipMemcpyHostToDevice, st));
    const int rc = launch_lsq_analytic(st, reinterpret_cast<const LsqAnalyticJob *>(d_mem), Kg, Dmax, true);
    if (rc != NMRFIT_OK) return rc;
    if (A_out) NMRFIT_HIP(hipMemcpyAsync(A_out, d_A, (size_t)n_A * sizeof(double), hipMemcpyDeviceToHost, st));
    if (g_out) NMRFIT_HIP(hipMemcpyAsync(g_out, d_g, (size_t)n_x * sizeof(double), hipMemcpyDeviceToHost, st));
    if (f_out) NMRFIT_HIP(hipMemcpyAsync(f_out, d_f, (size_t)Kg * sizeof(double), hipMemcpyDeviceToHost, st));
    NMRFIT_HIP(hipStreamSynchronize(st));
    return NMRFIT_OK;
}

// groups of consecutive fits whose segment sums fit the workspace budget (a fit larger than the budget runs alone)
static int part_analytic(BatchPart *b, const double *x, double *A_out, double *g_out, double *f_out)
{
    int rc = bind_batch(b);
    if (rc != NMRFIT_OK) return rc;
    int64_t budget = (int64_t)256 << 17;   // doubles: 256 MiB
    if (const char *e = getenv("NMRFIT_LSQ_WORKSPACE_MB")) budget = std::max<int64_t>(1, atoll(e)) << 17;
    int64_t at_x = 0, at_A = 0;
    for (int32_t k0 = 0; k0 < b->K && rc == NMRFIT_OK;) {
        int32_t k1 = k0;
        int64_t n_partial = 0, d_x = 0, d_A = 0;
        while (k1 < b->K) {
            const int64_t D = b->D[(size_t)k1];
            int32_t nseg, seg_tiles;
            lsq_segments(b->Nk[(size_t)k1], &nseg, &seg_tiles);
            const int64_t need = nseg * lsq_sums_analytic(D);
            if (k1 > k0 && n_partial + need > budget) break;
            n_partial += need;
            d_x += D;
            d_A += D * D;
            ++k1;
        }
        {
            Scratch mem;
            rc = part_analytic_group(b, k0, k1, x + at_x, A_out ? A_out + at_A : nullptr, g_out ? g_out + at_x : nullptr,
                                     f_out ? f_out + k0 : nullptr, mem);
            if (rc != NMRFIT_OK) (void)hipStreamSynchronize(b->stream);   // what was enqueued may still use the buffers `mem` frees
        }
        at_x += d_x;
        at_A += d_A;
        k0 = k1;
    }
    return rc;
}

#pragma GCC visibility push(default)   // the C-ABI: the only symbols the library exports (build.sh: -fvisibility=hidden)
extern "C" {

int nmrfit_jacobian_analytic(nmrfit_ctx *ctx, int32_t P, const double *x, double *J_out, double *r_out, double *A_out,
                             double *g_out, double *f_out)
{
    const char *who = "nmrfit_jacobian_analytic";
    int rc = bind(ctx);
    if (rc != NMRFIT_OK) return rc;
    if (!x || P < 0) return refuse(NMRFIT_E_INVALID, std::string(who) + ": null x or a negative peak count");
    const int64_t D = 4 + 3 * (int64_t)P, N = ctx->N;
    if (D > kLsqMaxD)
        return refuse(NMRFIT_E_UNSUPPORTED, std::string(who) + ": every output of this path needs D = 4 + 3 P <= " + std::to_string(kLsqMaxD));
    if ((rc = check_point(who, -1, P, x, ctx->w0, ctx->wspan)) != NMRFIT_OK) return rc;
    const bool sums = A_out || g_out || f_out;
    if (!J_out && !r_out && !sums) return NMRFIT_OK;
    LsqAnalyticJob job{};
    lsq_segments(N, &job.nseg, &job.seg_tiles);
    const int64_t n_J = J_out ? N * D : 0, n_r = r_out ? N : 0, n_partial = sums ? job.nseg * lsq_sums_analytic(D) : 0;
    const int64_t n_up = D + kJobDoubles;
    if ((rc = ensure(ctx, &ctx->d_X, &ctx->cap_X, n_up)) != NMRFIT_OK) return rc;
    if ((rc = ensure(ctx, &ctx->d_lsq, &ctx->cap_lsq, n_J + n_r + n_partial + D * D + D + 1)) != NMRFIT_OK) return rc;
    double *d_J = ctx->d_lsq, *d_r = d_J + n_J, *d_partial = d_r + n_r, *d_A = d_partial + n_partial, *d_g = d_A + D * D, *d_f = d_g + D;
    job.wc = ctx->d_wc;
    job.u = ctx->d_u;
    job.v = ctx->d_v;
    job.wt = ctx->d_wt;
    job.x = ctx->d_X;
    job.w0 = ctx->w0;
    job.s = 1.0 / std::sqrt((double)N);
    job.N = N;
    job.P = P;
    job.D = (int32_t)D;
    job.J = J_out ? d_J : nullptr;
    job.r = r_out ? d_r : nullptr;
    job.partial = sums ? d_partial : nullptr;
    job.A = sums ? d_A : nullptr;
    job.g = sums ? d_g : nullptr;
    job.f = sums ? d_f : nullptr;
    hipStream_t st = ctx->stream;
    std::vector<double> up((size_t)n_up);
    memcpy(up.data(), x, (size_t)D * sizeof(double));
    memcpy(up.data() + D, &job, sizeof(LsqAnalyticJob));
    // (pageable host memory: the copy has left `up` when hipMemcpyAsync returns)
    NMRFIT_HIP(hipMemcpyAsync(ctx->d_X, up.data(), up.size() * sizeof(double), hipMemcpyHostToDevice, st));
    if ((rc = launch_lsq_analytic(st, reinterpret_cast<const LsqAnalyticJob *>(ctx->d_X + D), 1, (int32_t)D, sums)) != NMRFIT_OK) return rc;
    if (A_out) NMRFIT_HIP(hipMemcpyAsync(A_out, d_A, (size_t)(D * D) * sizeof(double), hipMemcpyDeviceToHost, st));
    if (g_out) NMRFIT_HIP(hipMemcpyAsync(g_out, d_g, (size_t)D * sizeof(double), hipMemcpyDeviceToHost, st));
    if (f_out) NMRFIT_HIP(hipMemcpyAsync(f_out, d_f, sizeof(double), hipMemcpyDeviceToHost, st));
    if (r_out && (rc = staged_d2h(ctx->device, st, r_out, d_r, (size_t)N * sizeof(double))) != NMRFIT_OK) return rc;
    if (J_out && (rc = staged_d2h(ctx->device, st, J_out, d_J, (size_t)(N * D) * sizeof(double))) != NMRFIT_OK) return rc;
    NMRFIT_HIP(hipStreamSynchronize(st));
    return NMRFIT_OK;
}

// Every refusal comes before the first launch: the batch is as it was.  A batch created with a fit_im mode is served its
// real channel, as nmrfit_batch_normal_equations serves it.
int nmrfit_batch_normal_equations_analytic(nmrfit_batch *b, const double *x, double *A_out, double *g_out, double *f_out)
{
    const char *who = "nmrfit_batch_normal_equations_analytic";
    int rc = check_batch_handle(b);
    if (rc != NMRFIT_OK) return rc;
    if (!x) return refuse(NMRFIT_E_INVALID, std::string(who) + ": null x");
    for (size_t p = 0; p < b->parts.size(); ++p) {
        const BatchPart *q = b->parts[p];
        if (4 + 3 * (int64_t)q->Pmax > kLsqMaxD)
            return refuse(NMRFIT_E_UNSUPPORTED, std::string(who) + ": D = 4 + 3 P <= " + std::to_string(kLsqMaxD) + " for every fit");
        const int32_t f0 = b->first[p];
        for (int32_t k = 0; k < q->K; ++k) {
            const BatchFit &f = q->h_fits[(size_t)k];
            if ((rc = check_point(who, f0 + k, f.P, x + b->boff[(size_t)(f0 + k)], f.w0, f.wspan)) != NMRFIT_OK) return rc;
        }
    }
    if ((rc = check_idle(b, who)) != NMRFIT_OK) return rc;
    int64_t at_A = 0;
    for (size_t p = 0; p < b->parts.size() && rc == NMRFIT_OK; ++p) {
        const int32_t f0 = b->first[p], f1 = b->first[p + 1];
        const int64_t at_x = b->boff[(size_t)f0];
        rc = part_analytic(b->parts[p], x + at_x, A_out ? A_out + at_A : nullptr, g_out ? g_out + at_x : nullptr,
                           f_out ? f_out + f0 : nullptr);
        for (int32_t k = f0; k < f1; ++k) {
            const int64_t D = b->boff[(size_t)k + 1] - b->boff[(size_t)k];
            at_A += D * D;
        }
    }
    return rc;
}

}  // extern "C"
#pragma GCC visibility pop

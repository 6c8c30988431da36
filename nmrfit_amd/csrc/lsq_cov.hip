// lsq_cov.hip -- the "meat" of the sandwich covariance of a fit's parameters (include/nmrfit_amd_cov.h): from the D + 1
// residual rows that the normal-equations launch of the same call has just used, M = J^T diag(q) J with
// q_j = (weights_j s)^2 (cos^2 phi_j sigma_u^2 + sin^2 phi_j sigma_v^2) the variance of the weighted residual at grid
// point j under independent noise on u and v.  lsq_meat_kernel is the stages of lsq_tile.h, which states the plan, on
// the D columns of J with the q of kind rr.  
//
// And the host side of BOTH meats, this one and the two-channel one of lsq_cov_im.hip: the jobs of a fit
// (lsq_meat_jobs), the launch (launch_lsq_meat) and the calls on a context, nmrfit_sandwich and nmrfit_sandwich_im.
#include "host_call.h"
#include "lsq_tile.h"
#include "nmrfit_amd_cov.h"
#include "nmrfit_amd_cov_im.h"

#include <cmath>

namespace nmrfit {
namespace {

__global__ __launch_bounds__(kLsqThreads) void lsq_meat_kernel(const LsqMeatJob *__restrict__ jobs)
{
    extern __shared__ double T[];   // [kLsqTile][pitch], then Q [kLsqTile]
    const LsqMeatJob &q = jobs[blockIdx.y];
    if ((int)blockIdx.x >= q.nseg) return;   // (a batch's launch is as wide as its longest grid needs)
    const int D = q.D, pitch = D | 1;
    double *Q = T + kLsqTile * pitch;
    const int64_t N = q.N;
    const int tid = threadIdx.x, jl = tid & (kLsqTile - 1), i0 = tid >> 6;
    const int nout = D * (D + 1) / 2;
    int pa[kLsqAcc], pb[kLsqAcc];
    double acc[kLsqAcc];
    lsq_own_pairs(nout, [D](int o, int *a, int *b) { lsq_pair(o, D, a, b); }, pa, pb, acc);
    int64_t t0, t1;
    lsq_tile_range(N, q.seg_tiles, &t0, &t1);
    for (int64_t t = t0; t < t1; ++t) {
        const int64_t j0 = t * kLsqTile;
        const int nj = (int)((N - j0 < kLsqTile) ? N - j0 : kLsqTile);
        const bool have = jl < nj;
        lsq_form(T, pitch, q.Rb, q.c, 0.0, N, D, j0, have, i0, 0, D);
        if (i0 == kLsqWaves - 1) Q[jl] = have ? lsq_q(q, kMeatRR, j0 + jl) : 0.0;   // (the wave with the fewest columns of T)
        __syncthreads();
        lsq_accumulate<true>(T, pitch, T, pitch, Q, nj, pa, pb, acc);
        __syncthreads();
    }
    lsq_store_partial(q.partial, nout, acc);
}

// the segments' sums one after the other, segment 0 first; M comes back whole (both triangles from the same sum)
__global__ __launch_bounds__(kLsqThreads) void lsq_meat_reduce_kernel(const LsqMeatJob *__restrict__ jobs)
{
    const LsqMeatJob &q = jobs[blockIdx.x];
    const int D = q.D, nout = D * (D + 1) / 2;
    for (int o = threadIdx.x; o < nout; o += kLsqThreads) {
        const double sum = lsq_segment_sum(q.partial, q.nseg, nout, o);
        int a, b;
        lsq_pair(o, D, &a, &b);
        q.M[a * D + b] = sum;
        q.M[b * D + a] = sum;
    }
}

}  // namespace

int64_t lsq_meat_partials(int64_t N, int64_t D, int nch)
{
    int32_t nseg, seg_tiles;
    lsq_segments(N, &nseg, &seg_tiles);
    const int64_t C = D + 1;
    // one upper triangle of D columns; both channels: two of C columns and the whole cross block
    return nseg * (nch == 2 ? C * (C + 1) + C * C : D * (D + 1) / 2);
}

void lsq_meat_jobs(LsqMeatJob *job, int nch, const double *R, const double *c, const double *wt, double s, double p0, double p1,
                   double sigma_u, double sigma_v, int64_t N, int32_t D, double *partial, double *M)
{
    const int32_t C = nch == 2 ? D + 1 : D;   // the columns of a block: on both channels Jt carries r
    const double *im = R + (int64_t)(D + 1) * N;   // (the imaginary plane: read by the jobs of nch = 2 alone)
    const double var_u = sigma_u * sigma_u, var_v = sigma_v * sigma_v;
    for (int n = 0; n < lsq_meat_njobs(nch); ++n) {
        LsqMeatJob &j = job[n];
        j = LsqMeatJob{};
        j.kind = n < 2 ? n : kMeatRI;
        j.Ra = n == 1 ? im : R;
        j.Rb = n == 0 ? R : im;
        j.c = c;
        j.wt = wt;
        j.s = s;
        j.p0 = p0;
        j.p1 = p1;
        j.var_u = j.kind == kMeatRI ? var_u - var_v : var_u;
        j.var_v = j.kind == kMeatRI ? 0.0 : var_v;
        j.N = N;
        j.D = D;
        lsq_segments(N, &j.nseg, &j.seg_tiles);
        j.row0 = n == 3 ? cross_split(C) : 0;
        j.row1 = n == 2 ? cross_split(C) : C;
        j.partial = partial;
        j.M = M + (int64_t)j.kind * C * C;
        partial += j.nseg * (j.kind == kMeatRI ? (int64_t)(j.row1 - j.row0) * C : (int64_t)C * (C + 1) / 2);
    }
}

int launch_lsq_meat(hipStream_t st, const LsqMeatJob *d_jobs, int32_t njobs, int32_t Dmax, int nch)
{
    if (njobs <= 0) return NMRFIT_OK;
    if (Dmax > kLsqMaxD) {
        set_error(std::string(nch == 2 ? "sandwich_im" : "sandwich") + ": D = 4 + 3 P above " + std::to_string(kLsqMaxD));
        return NMRFIT_E_UNSUPPORTED;
    }
    if (nch == 2) return launch_lsq_meat_im_kernels(st, d_jobs, njobs, Dmax);
    const size_t lds = (size_t)kLsqTile * (size_t)((Dmax | 1) + 1) * sizeof(double);
    hipLaunchKernelGGL(lsq_meat_kernel, dim3((unsigned)kLsqMaxSegments, (unsigned)njobs), dim3(kLsqThreads), lds, st, d_jobs);
    NMRFIT_HIP(hipGetLastError());
    hipLaunchKernelGGL(lsq_meat_reduce_kernel, dim3((unsigned)njobs), dim3(kLsqThreads), 0, st, d_jobs);
    NMRFIT_HIP(hipGetLastError());
    return NMRFIT_OK;
}

int check_sigma(const char *who, double sigma_u, double sigma_v)
{
    if (!(std::isfinite(sigma_u) && std::isfinite(sigma_v) && sigma_u >= 0.0 && sigma_v >= 0.0))
        return refuse(NMRFIT_E_INVALID, std::string(who) + ": sigma_u and sigma_v must be finite and >= 0");
    return NMRFIT_OK;
}

}  // namespace nmrfit

using namespace nmrfit;

#pragma GCC visibility push(default)   // the C-ABI: the only symbols the library exports (build.sh: -fvisibility=hidden)
extern "C" {

// Both entry points.  A, g and f are nmrfit_jacobian*'s own (ctx_eval.hip; nch = 2: f is the pair rho): that call leaves
// the nch planes of D + 1 residual rows in the context's d_R and the factors behind the parameter rows in d_X, and the
// meat launch reads them there, on the same stream.  The records and sums of the meat are one Scratch block of this
// call: [records | segments' sums | M].
static int ctx_sandwich(nmrfit_ctx *ctx, const char *who, int nch, int fit_im, int32_t P, const double *rows, const double *c, double s,
                        double sigma_u, double sigma_v, double *A_out, double *g_out, double *f_out, double *M_out)
{
    int rc = bind(ctx);
    if (rc != NMRFIT_OK) return rc;
    if (!rows || !c) return refuse(NMRFIT_E_INVALID, std::string(who) + ": null rows or c");
    if (nch == 2 && fit_im != NMRFIT_FIT_IM_REFERENCE && fit_im != NMRFIT_FIT_IM_SUM)
        return refuse(NMRFIT_E_INVALID, std::string(who) + ": fit_im must be 1 (reference fit_im=True) or 2 (all-peak imaginary model)");
    if ((rc = check_batch(1, P, rows, c)) != NMRFIT_OK) return rc;
    if ((rc = check_sigma(who, sigma_u, sigma_v)) != NMRFIT_OK) return rc;
    const int64_t D = 4 + 3 * (int64_t)P, B = D + 1, N = ctx->N;
    if (D > kLsqMaxD) return refuse(NMRFIT_E_UNSUPPORTED, std::string(who) + ": D = 4 + 3 P <= " + std::to_string(kLsqMaxD));
    if (ctx->variant != NMRFIT_VARIANT_DEFAULT)
        return refuse(NMRFIT_E_UNSUPPORTED, std::string(who) + ": the context's kernel variant must be DEFAULT");
    if (!A_out && !g_out && !f_out && !M_out) return NMRFIT_OK;
    // (with M alone the call still runs the rows launch: f is the cheapest thing to ask of it)
    double f_own[2] = {0.0, 0.0};
    double *f = f_out ? f_out : (A_out || g_out ? nullptr : f_own);
    rc = nch == 2 ? nmrfit_jacobian_im(ctx, P, rows, c, s, fit_im, nullptr, nullptr, A_out, g_out, f)
                  : nmrfit_jacobian(ctx, P, rows, c, s, nullptr, nullptr, A_out, g_out, f);
    if (rc != NMRFIT_OK || !M_out) return rc;
    const int njobs = lsq_meat_njobs(nch);
    const int64_t kJobDoubles = (int64_t)(align256((size_t)njobs * sizeof(LsqMeatJob)) / sizeof(double));
    const int64_t n_partial = lsq_meat_partials(N, D, nch), n_M = meat_doubles(D, nch);
    hipStream_t st = ctx->stream;
    Scratch mem;
    const auto enqueue_and_wait = [&]() -> int {
        double *d_mem = nullptr;
        NMRFIT_HIP(mem.alloc(&d_mem, (size_t)(kJobDoubles + n_partial + n_M)));
        double *d_M = d_mem + kJobDoubles + n_partial;
        LsqMeatJob job[4];
        lsq_meat_jobs(job, nch, ctx->d_R, ctx->d_X + B * D, ctx->d_wt, s, rows[0], rows[1], sigma_u, sigma_v, N, (int32_t)D,
                      d_mem + kJobDoubles, d_M);
        // (pageable host memory: the copy has left `job` when hipMemcpyAsync returns)
        NMRFIT_HIP(hipMemcpyAsync(d_mem, job, (size_t)njobs * sizeof(LsqMeatJob), hipMemcpyHostToDevice, st));
        const int launched = launch_lsq_meat(st, reinterpret_cast<const LsqMeatJob *>(d_mem), njobs, (int32_t)D, nch);
        if (launched != NMRFIT_OK) return launched;
        NMRFIT_HIP(hipMemcpyAsync(M_out, d_M, (size_t)n_M * sizeof(double), hipMemcpyDeviceToHost, st));
        NMRFIT_HIP(hipStreamSynchronize(st));
        return NMRFIT_OK;
    };
    rc = enqueue_and_wait();
    if (rc != NMRFIT_OK) (void)hipStreamSynchronize(st);   // what was enqueued may still use the buffers `mem` frees
    return rc;
}

int nmrfit_sandwich(nmrfit_ctx *ctx, int32_t P, const double *rows, const double *c, double s, double sigma_u, double sigma_v,
                    double *A_out, double *M_out, double *g_out, double *f_out)
{
    return ctx_sandwich(ctx, "nmrfit_sandwich", 1, 0, P, rows, c, s, sigma_u, sigma_v, A_out, g_out, f_out, M_out);
}

int nmrfit_sandwich_im(nmrfit_ctx *ctx, int32_t P, int fit_im, const double *rows, const double *c, double s, double sigma_u,
                       double sigma_v, double *A_out, double *g_out, double *rho_out, double *M_out)
{
    return ctx_sandwich(ctx, "nmrfit_sandwich_im", 2, fit_im, P, rows, c, s, sigma_u, sigma_v, A_out, g_out, rho_out, M_out);
}

}  // extern "C"
#pragma GCC visibility pop

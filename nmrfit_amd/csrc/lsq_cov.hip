// lsq_cov.hip -- the "meat" of the sandwich covariance of a fit's parameters (include/nmrfit_amd_cov.h): from the D + 1
// residual rows that the normal-equations launch of the same call has just used, M = J^T diag(q) J with
// q_j = (weights_j s)^2 (cos^2 phi_j sigma_u^2 + sin^2 phi_j sigma_v^2) the variance of the weighted residual at grid
// point j under independent noise on u and v; and nmrfit_sandwich, the call on a context.
//
// lsq_meat_kernel is built on the plan of lsq_normal_kernel (lsq.hip): a workgroup owns a segment of the grid
// (lsq_segments: whole tiles of 64 points, a function of N alone), forms T[j][0..D) = (R[i + 1][j] - R[0][j]) * c_i per
// tile in LDS -- the row loads coalesced along the grid, the LDS rows at an ODD pitch -- and every thread adds the tile's
// 64 products to the (up to) twelve entries of the upper triangle it owns (lsq_pair), in registers, point after point:
//     acc = fma(q_j * T[j][a], T[j][b], acc)
// What is new is q_j: one wave forms it per tile from the RESIDENT weights (grid_slot order, as the objective kernels
// read them), s and sincos(p0 + p1 * (j / N)) in fp64 -- neither J nor the weights move.  The per-segment sums go to
// memory; lsq_meat_reduce_kernel adds them segment 0 first and writes both triangles from the one sum.  Every sum has
// ONE order, fixed by N: no atomics, nothing depends on scheduling, on the batch or on the position in it.  Plain fp64
// FMAs for the reasons lsq.hip gives.  
#include "host_call.h"
#include "lsq_internal.h"
#include "nmrfit_amd_cov.h"

#include <cmath>

namespace nmrfit {
namespace {

constexpr int kMeatWaves = kLsqThreads / kLsqTile;

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
#pragma unroll
    for (int m = 0; m < kLsqAcc; ++m) {
        const int o = tid + m * kLsqThreads;
        pa[m] = pb[m] = 0;
        if (o < nout) lsq_pair(o, D, &pa[m], &pb[m]);
        acc[m] = 0.0;
    }
    const int64_t tiles = (N + kLsqTile - 1) / kLsqTile;
    const int64_t t0 = (int64_t)blockIdx.x * q.seg_tiles;
    const int64_t t1 = (t0 + q.seg_tiles < tiles) ? t0 + q.seg_tiles : tiles;
    const double *__restrict__ R = q.R;
    const double *__restrict__ c = q.c;
    for (int64_t t = t0; t < t1; ++t) {
        const int64_t j0 = t * kLsqTile;
        const int nj = (int)((N - j0 < kLsqTile) ? N - j0 : kLsqTile);
        const bool have = jl < nj;
        const double r0 = have ? R[j0 + jl] : 0.0;
        for (int i = i0; i < D; i += kMeatWaves) {
            const double ri = have ? R[(int64_t)(i + 1) * N + j0 + jl] : 0.0;
            T[jl * pitch + i] = (ri - r0) * c[i];
        }
        if (i0 == kMeatWaves - 1) {   // (the wave with the fewest columns of T)
            double qj = 0.0;
            if (have) {
                const int64_t j = j0 + jl;
                double sn, cs;
                sincos(q.p0 + q.p1 * ((double)j / (double)N), &sn, &cs);
                const double ws = q.wt[grid_slot(j)] * q.s;
                qj = (ws * ws) * (cs * cs * q.var_u + sn * sn * q.var_v);
            }
            Q[jl] = qj;
        }
        __syncthreads();
        for (int jj = 0; jj < nj; ++jj) {
            const double *row = T + jj * pitch;
            const double qq = Q[jj];
#pragma unroll
            for (int m = 0; m < kLsqAcc; ++m) acc[m] = __builtin_fma(qq * row[pa[m]], row[pb[m]], acc[m]);
        }
        __syncthreads();
    }
    double *__restrict__ out = q.partial + (int64_t)blockIdx.x * nout;
#pragma unroll
    for (int m = 0; m < kLsqAcc; ++m) {
        const int o = tid + m * kLsqThreads;
        if (o < nout) out[o] = acc[m];
    }
}

// the segments' sums one after the other, segment 0 first; M comes back whole (both triangles from the same sum)
__global__ __launch_bounds__(kLsqThreads) void lsq_meat_reduce_kernel(const LsqMeatJob *__restrict__ jobs)
{
    const LsqMeatJob &q = jobs[blockIdx.x];
    const int D = q.D, nout = D * (D + 1) / 2;
    for (int o = threadIdx.x; o < nout; o += kLsqThreads) {
        double sum = 0.0;
        for (int sgm = 0; sgm < q.nseg; ++sgm) sum += q.partial[(int64_t)sgm * nout + o];
        int a, b;
        lsq_pair(o, D, &a, &b);
        q.M[a * D + b] = sum;
        q.M[b * D + a] = sum;
    }
}

}  // namespace

int launch_lsq_meat(hipStream_t st, const LsqMeatJob *d_jobs, int32_t K, int32_t Dmax)
{
    if (K <= 0) return NMRFIT_OK;
    if (Dmax > kLsqMaxD) {
        set_error("sandwich: D = 4 + 3 P above " + std::to_string(kLsqMaxD));
        return NMRFIT_E_UNSUPPORTED;
    }
    const size_t lds = (size_t)kLsqTile * (size_t)((Dmax | 1) + 1) * sizeof(double);
    hipLaunchKernelGGL(lsq_meat_kernel, dim3((unsigned)kLsqMaxSegments, (unsigned)K), dim3(kLsqThreads), lds, st, d_jobs);
    NMRFIT_HIP(hipGetLastError());
    hipLaunchKernelGGL(lsq_meat_reduce_kernel, dim3((unsigned)K), dim3(kLsqThreads), 0, st, d_jobs);
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

// A, g and f are nmrfit_jacobian's own (ctx_eval.hip): that call leaves the D + 1 residual rows in the context's d_R and
// the factors behind the parameter rows in d_X, and the meat launch reads them there, on the same stream.  The records
// and sums of the meat are one Scratch block of this call.
int nmrfit_sandwich(nmrfit_ctx *ctx, int32_t P, const double *rows, const double *c, double s, double sigma_u, double sigma_v,
                    double *A_out, double *M_out, double *g_out, double *f_out)
{
    int rc = bind(ctx);
    if (rc != NMRFIT_OK) return rc;
    if (!rows || !c) return refuse(NMRFIT_E_INVALID, "nmrfit_sandwich: null rows or c");
    if ((rc = check_batch(1, P, rows, c)) != NMRFIT_OK) return rc;
    if ((rc = check_sigma("nmrfit_sandwich", sigma_u, sigma_v)) != NMRFIT_OK) return rc;
    const int64_t D = 4 + 3 * (int64_t)P, B = D + 1, N = ctx->N;
    if (D > kLsqMaxD) return refuse(NMRFIT_E_UNSUPPORTED, "nmrfit_sandwich: D = 4 + 3 P <= " + std::to_string(kLsqMaxD));
    if (ctx->variant != NMRFIT_VARIANT_DEFAULT)
        return refuse(NMRFIT_E_UNSUPPORTED, "nmrfit_sandwich: the context's kernel variant must be DEFAULT");
    if (!A_out && !M_out && !g_out && !f_out) return NMRFIT_OK;
    // (with M alone the call still runs the rows launch: f is the cheapest thing to ask of it)
    double f_own = 0.0;
    rc = nmrfit_jacobian(ctx, P, rows, c, s, nullptr, nullptr, A_out, g_out, f_out ? f_out : (A_out || g_out ? nullptr : &f_own));
    if (rc != NMRFIT_OK || !M_out) return rc;
    LsqMeatJob job{};
    job.R = ctx->d_R;
    job.c = ctx->d_X + B * D;
    job.wt = ctx->d_wt;
    job.s = s;
    job.p0 = rows[0];
    job.p1 = rows[1];
    job.var_u = sigma_u * sigma_u;
    job.var_v = sigma_v * sigma_v;
    job.N = N;
    job.D = (int32_t)D;
    lsq_segments(N, &job.nseg, &job.seg_tiles);
    const int64_t kJobDoubles = (int64_t)(align256(sizeof(LsqMeatJob)) / sizeof(double));
    hipStream_t st = ctx->stream;
    Scratch mem;
    const auto enqueue_and_wait = [&]() -> int {
        double *d_mem = nullptr;
        NMRFIT_HIP(mem.alloc(&d_mem, (size_t)(kJobDoubles + job.nseg * (D * (D + 1) / 2) + D * D)));
        job.partial = d_mem + kJobDoubles;
        job.M = job.partial + job.nseg * (D * (D + 1) / 2);
        // (pageable host memory: the copy has left `job` when hipMemcpyAsync returns)
        NMRFIT_HIP(hipMemcpyAsync(d_mem, &job, sizeof(job), hipMemcpyHostToDevice, st));
        const int launched = launch_lsq_meat(st, reinterpret_cast<const LsqMeatJob *>(d_mem), 1, (int32_t)D);
        if (launched != NMRFIT_OK) return launched;
        NMRFIT_HIP(hipMemcpyAsync(M_out, job.M, (size_t)(D * D) * sizeof(double), hipMemcpyDeviceToHost, st));
        NMRFIT_HIP(hipStreamSynchronize(st));
        return NMRFIT_OK;
    };
    rc = enqueue_and_wait();
    if (rc != NMRFIT_OK) (void)hipStreamSynchronize(st);   // what was enqueued may still use the buffers `mem` frees
    return rc;
}

}  // extern "C"
#pragma GCC visibility pop

// lsq_cov_im.hip -- the "meat" of the sandwich covariance of a fit made on BOTH channels (include/nmrfit_amd_cov_im.h):
// from the two planes of D + 1 residual rows that the both-channel rows launch of the same call has just written, the
// three blocks Mt_rr, Mt_ii, Mt_ri of Mt_ab = Jt_a^T diag(q_ab) Jt_b, Jt_ch = [J_ch | r_ch] (C = D + 1 columns: the last
// one carries the derivative of 1 / rho_ch).
//
// lsq_meat_im_kernel is the stages of lsq_tile.h, which states the plan, on C columns with the q of the job's kind.  A
// workgroup owns a segment of the grid and one JOB of a fit (LsqMeatJob): a symmetric block's upper triangle,
// C (C + 1) / 2 <= 3003 entries, or a band of rows of the cross block, at most 39 x 77 = 3003 -- twelve sums per thread
// either way.  A cross job also forms the band's own columns of channel a (Ta: the whole launch stays below 64 KiB of LDS
// at D = 76), and its reduce writes every entry once.  The kernel does not know the imaginary model's mode: it differs in
// the rows alone.  The host side is lsq_cov.hip's.  
#include "lsq_tile.h"

namespace nmrfit {
namespace {

__global__ __launch_bounds__(kLsqThreads) void lsq_meat_im_kernel(const LsqMeatJob *__restrict__ jobs)
{
    extern __shared__ double T[];   // [kLsqTile][pitch]; a cross job: then Ta [kLsqTile][pitch_a]; then Q [kLsqTile]
    const LsqMeatJob &q = jobs[blockIdx.y];
    if ((int)blockIdx.x >= q.nseg) return;   // (a launch is as wide as its longest grid needs)
    const int D = q.D, C = D + 1, pitch = C | 1;
    const bool cross = q.kind == kMeatRI;
    const int row0 = q.row0, na = q.row1 - q.row0, pitch_a = cross ? (na | 1) : pitch;
    double *Ta = cross ? T + kLsqTile * pitch : T;
    double *Q = Ta + (cross ? kLsqTile * pitch_a : kLsqTile * pitch);
    const int64_t N = q.N;
    const int tid = threadIdx.x, jl = tid & (kLsqTile - 1), i0 = tid >> 6;
    const int nout = cross ? na * C : C * (C + 1) / 2;
    int pa[kLsqAcc], pb[kLsqAcc];
    double acc[kLsqAcc];
    lsq_own_pairs(nout, [C, cross](int o, int *a, int *b) {
        if (cross) {
            *a = o / C;   // (the band's own column of Ta)
            *b = o - *a * C;
        } else {
            lsq_pair(o, C, a, b);
        }
    }, pa, pb, acc);
    int64_t t0, t1;
    lsq_tile_range(N, q.seg_tiles, &t0, &t1);
    for (int64_t t = t0; t < t1; ++t) {
        const int64_t j0 = t * kLsqTile;
        const int nj = (int)((N - j0 < kLsqTile) ? N - j0 : kLsqTile);
        const bool have = jl < nj;
        lsq_form(T, pitch, q.Rb, q.c, q.s, N, D, j0, have, i0, 0, C);
        if (cross) lsq_form(Ta, pitch_a, q.Ra, q.c, q.s, N, D, j0, have, i0, row0, row0 + na);
        if (i0 == kLsqWaves - 1) Q[jl] = have ? lsq_q(q, q.kind, j0 + jl) : 0.0;
        __syncthreads();
        lsq_accumulate<true>(Ta, pitch_a, T, pitch, Q, nj, pa, pb, acc);
        __syncthreads();
    }
    lsq_store_partial(q.partial, nout, acc);
}

// the segments' sums one after the other, segment 0 first; a symmetric block comes back whole (both triangles from the
// same sum), a band of the cross block entry by entry
__global__ __launch_bounds__(kLsqThreads) void lsq_meat_im_reduce_kernel(const LsqMeatJob *__restrict__ jobs)
{
    const LsqMeatJob &q = jobs[blockIdx.x];
    const int C = q.D + 1;
    const bool cross = q.kind == kMeatRI;
    const int nout = cross ? (q.row1 - q.row0) * C : C * (C + 1) / 2;
    for (int o = threadIdx.x; o < nout; o += kLsqThreads) {
        const double sum = lsq_segment_sum(q.partial, q.nseg, nout, o);
        if (cross) {
            q.M[q.row0 * C + o] = sum;
        } else {
            int a, b;
            lsq_pair(o, C, &a, &b);
            q.M[a * C + b] = sum;
            q.M[b * C + a] = sum;
        }
    }
}

}  // namespace

int launch_lsq_meat_im_kernels(hipStream_t st, const LsqMeatJob *d_jobs, int32_t njobs, int32_t Dmax)
{
    // the largest job of the launch: a band of the cross block, T and Ta, and the q row
    const int C = Dmax + 1;
    const size_t lds = (size_t)kLsqTile * (size_t)((C | 1) + (cross_split(C) | 1) + 1) * sizeof(double);
    hipLaunchKernelGGL(lsq_meat_im_kernel, dim3((unsigned)kLsqMaxSegments, (unsigned)njobs), dim3(kLsqThreads), lds, st, d_jobs);
    NMRFIT_HIP(hipGetLastError());
    hipLaunchKernelGGL(lsq_meat_im_reduce_kernel, dim3((unsigned)njobs), dim3(kLsqThreads), 0, st, d_jobs);
    NMRFIT_HIP(hipGetLastError());
    return NMRFIT_OK;
}

}  // namespace nmrfit

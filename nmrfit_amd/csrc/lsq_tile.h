// lsq_tile.h -- the stages the three least-squares sums of the device are composed from: lsq_normal_kernel (lsq.hip:
// A = J^T J, g = J^T r, and J and r themselves), lsq_meat_kernel (lsq_cov.hip: M = J^T diag(q) J) and lsq_meat_im_kernel
// (lsq_cov_im.hip: the blocks Mt_ab = Jt_a^T diag(q_ab) Jt_b, Jt_ch = [J_ch | r_ch]), and their three reduce kernels.
//
// The plan.  A workgroup owns a SEGMENT of the grid (lsq_segments: whole tiles of 64 points,
// at most 64 segments per fit, a function of N alone) and up to 256 x 12 entries of one matrix.  Per tile it forms columns
// of [J | r] in LDS -- T[j][i < D] = (R[i + 1][j] - R[0][j]) * c_i, T[j][D] = R[0][j] * s; the row loads coalesced along the
// grid, the LDS rows at an ODD pitch so that the 64 lanes of a load (64 different j) hit 64 different bank pairs -- and, for
// a meat, one wave forms q_j from the RESIDENT weights (grid_slot order, as the objective kernels read them), s and
// sincos(p0 + p1 * (j / N)) in fp64: neither J nor the weights move.  Then every thread adds the tile's 64 products to the
// (up to) twelve entries it owns, in registers, point after point:
//     acc = fma([q_j *] Ta[j][a], T[j][b], acc)
// (Ta is T unless the job is a band of the cross block, whose rows are columns of the other channel).  The per-segment sums
// go to memory; a reduce kernel adds them segment after segment, segment 0 first.  Every sum has ONE order, fixed by N: no
// atomics, nothing depends on scheduling, on the batch or on the position in it.  That the kernels are made of the SAME
// stages is what their bit-for-bit promises rest on: the D x D corner of Mt_rr is M, and both are numpy's sums of the
// products J and r give.
//
// The products are plain fp64 FMAs, not v_mfma_f64_16x16x4_f64: D = 4 + 3 P is never a multiple of 16 (76 = 4.75 blocks: a
// quarter of the last block row and column would multiply padding), the contraction is N D^2 / 2 = 47 MFLOP at the C5
// shape -- microseconds next to the rows launch before it, which evaluates (D + 1) N P Voigt profiles -- and with scalar
// FMAs the order of every sum is written down in lsq_accumulate below.
//
// J and r equal the host's expressions bit for bit: `(a - b) * c` has nothing added to the product, so -ffp-contract=on
// finds nothing to fuse.
//
// pa, pb and acc are plain arrays passed by reference: wrapped in a struct they cost lsq_normal_kernel ten VGPRs.
#pragma once
#include "lsq_internal.h"

namespace nmrfit {

constexpr int kLsqWaves = kLsqThreads / kLsqTile;   // a wave is one column of a tile at a time

// the tiles [t0, t1) of the workgroup's segment
__device__ __forceinline__ void lsq_tile_range(int64_t N, int seg_tiles, int64_t *t0, int64_t *t1)
{
    const int64_t tiles = (N + kLsqTile - 1) / kLsqTile;
    *t0 = (int64_t)blockIdx.x * seg_tiles;
    *t1 = (*t0 + seg_tiles < tiles) ? *t0 + seg_tiles : tiles;
}

// the entries o = tid + m * 256 < nout a thread owns: pair(o, &a, &b) says which columns entry o multiplies; sums at zero
template <class Pair>
__device__ __forceinline__ void lsq_own_pairs(int nout, Pair pair, int (&pa)[kLsqAcc], int (&pb)[kLsqAcc], double (&acc)[kLsqAcc])
{
#pragma unroll
    for (int m = 0; m < kLsqAcc; ++m) {
        const int o = (int)threadIdx.x + m * kLsqThreads;
        pa[m] = pb[m] = 0;
        if (o < nout) pair(o, &pa[m], &pb[m]);
        acc[m] = 0.0;
    }
}

// columns [c0, c1) of [J | r] (c1 <= D + 1) for the thread's point j0 + jl of the tile into T[jl][0 .. c1 - c0): wave i0
// takes every kLsqWaves-th column.  have: the point lies on the grid (else zeros, which add nothing to any sum).
__device__ __forceinline__ void lsq_form(double *T, int pitch, const double *__restrict__ R, const double *__restrict__ c, double s,
                                         int64_t N, int D, int64_t j0, bool have, int i0, int c0, int c1)
{
    const int jl = threadIdx.x & (kLsqTile - 1);
    const double r0 = have ? R[j0 + jl] : 0.0;
    for (int i = c0 + i0; i < c1; i += kLsqWaves) {
        if (i < D) {
            const double ri = have ? R[(int64_t)(i + 1) * N + j0 + jl] : 0.0;
            T[jl * pitch + (i - c0)] = (ri - r0) * c[i];
        } else {
            T[jl * pitch + (i - c0)] = r0 * s;
        }
    }
}

// q_j of a kind: the (co)variance of the weighted residuals of the kind's two channels at grid point j under independent
// noise on u and v.  kMeatRI: var_u holds sigma_u^2 - sigma_v^2, formed once on the host -- the cross block is exactly 0
// when the two are equal.
__device__ __forceinline__ double lsq_q(const LsqMeatJob &q, int kind, int64_t j)
{
    double sn, cs;
    sincos(q.p0 + q.p1 * ((double)j / (double)q.N), &sn, &cs);
    const double ws = q.wt[grid_slot(j)] * q.s;
    if (kind == kMeatRR) return (ws * ws) * (cs * cs * q.var_u + sn * sn * q.var_v);
    if (kind == kMeatII) return (ws * ws) * (sn * sn * q.var_u + cs * cs * q.var_v);
    return (ws * ws) * (cs * sn * q.var_u);
}

// the tile's nj points, one after the other, onto the thread's sums.  WEIGHTED: by Q[j]
template <bool WEIGHTED>
__device__ __forceinline__ void lsq_accumulate(const double *Ta, int pitch_a, const double *T, int pitch, const double *Q, int nj,
                                               const int (&pa)[kLsqAcc], const int (&pb)[kLsqAcc], double (&acc)[kLsqAcc])
{
    for (int jj = 0; jj < nj; ++jj) {
        const double *rowa = Ta + jj * pitch_a;
        const double *rowb = T + jj * pitch;
        if (WEIGHTED) {
            const double qq = Q[jj];
#pragma unroll
            for (int m = 0; m < kLsqAcc; ++m) acc[m] = __builtin_fma(qq * rowa[pa[m]], rowb[pb[m]], acc[m]);
        } else {
#pragma unroll
            for (int m = 0; m < kLsqAcc; ++m) acc[m] = __builtin_fma(rowa[pa[m]], rowb[pb[m]], acc[m]);
        }
    }
}

// the segment's sums: row blockIdx.x of partial [nseg][nout]
__device__ __forceinline__ void lsq_store_partial(double *partial, int nout, const double (&acc)[kLsqAcc])
{
    double *__restrict__ out = partial + (int64_t)blockIdx.x * nout;
#pragma unroll
    for (int m = 0; m < kLsqAcc; ++m) {
        const int o = (int)threadIdx.x + m * kLsqThreads;
        if (o < nout) out[o] = acc[m];
    }
}

// entry o of every segment, one after the other, segment 0 first
__device__ __forceinline__ double lsq_segment_sum(const double *partial, int nseg, int nout, int o)
{
    double sum = 0.0;
    for (int sgm = 0; sgm < nseg; ++sgm) sum += partial[(int64_t)sgm * nout + o];
    return sum;
}

}  // namespace nmrfit

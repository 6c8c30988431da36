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

// ---- the analytic form stage (lsq_analytic.hip) ------------------------------------------------------
// What one peak contributes at a point, with t = (wc_j - locc) ihw, S = 1 + t^2, e = 2^-t^2 and q = s wt_j:
//     L = al / S            G = ag e                           the peak's two lines (their sum: the model)
//     d/dr     -q (dl / S - dg e)                              summed over the peaks
//     d/dwidth +q (ihw / 2) (L (1 - t^2) / S + G (1 - 2 ln2 t^2))
//     d/dloc   -q 2 ihw t (L / S + ln2 G)
//     d/da     -q (rl / S + rg e)
// The constants are formed once per workgroup (lsq_peak_consts): on the per-point path 1 / S is the only division.
struct LsqPeakConst {
    double ihw;    // 2 / width
    double locc;   // loc - w0
    double al;     // a r ihw / pi
    double ag;     // a (1 - r) ihw sqrt(ln2 / pi)
    double dl;     // a ihw / pi
    double dg;     // a ihw sqrt(ln2 / pi)
    double rl;     // r ihw / pi
    double rg;     // (1 - r) ihw sqrt(ln2 / pi)
};
constexpr double kLsqInvPi = 0.31830988618379067154;
constexpr double kLsqSqrtLn2OverPi = 0.46971863934982566689;   // sqrt(ln2 / pi)
constexpr double kLsqLn2 = 0.69314718055994530942;
constexpr int kLsqStrip = kLsqWaves * kLsqTile;                 // one [wave][point] strip of partial sums

// the fit's four resident arrays as the kernel holds them: in VECTOR registers (lsq_resident) -- as scalars they, with the
// twelve `o < nout` masks that lsq_own_pairs and lsq_store_partial share, leave the kernel parking scalars in vector lanes
struct LsqResident {
    const double *wc, *u, *v, *wt;
    double *J, *r;   // (and where the tile and the segment's sums go: lsq_write_tile takes the record as its job)
    double *partial;
};
__device__ __forceinline__ LsqResident lsq_resident(const LsqAnalyticJob &q)
{
    LsqResident g{q.wc, q.u, q.v, q.wt, q.J, q.r, q.partial};
    // (no instruction: the values are vector ones from here on)
    asm volatile("" : "+v"(g.wc), "+v"(g.u), "+v"(g.v), "+v"(g.wt), "+v"(g.J), "+v"(g.r), "+v"(g.partial));
    return g;
}
constexpr int kLsqHead = 6;   // what the columns 0 - 3 and D need of x and the job: p0, p1, P yoff, P, s, N (read from LDS: the
                              // kernel has no scalar registers to spare for them across its tile loop)

// doubles of LDS behind the tile: the head, the peaks' constants, the two strips (model, d/dr)
__host__ __device__ inline int lsq_analytic_extra(int P)
{
    return kLsqHead + P * (int)(sizeof(LsqPeakConst) / sizeof(double)) + 2 * kLsqStrip;
}

// head [kLsqHead] and pk [P]: formed once per workgroup
__device__ __forceinline__ void lsq_peak_consts(double *head, LsqPeakConst *pk, const double *__restrict__ x, int P, double w0, double s,
                                                int64_t N)
{
    const double r = x[2];
    if (threadIdx.x == kLsqThreads - 1) {
        head[0] = x[0];
        head[1] = x[1];
        head[2] = (double)P * x[3];   // (the reference adds yoff once per peak)
        head[3] = (double)P;
        head[4] = s;
        head[5] = (double)N;
    }
    for (int k = threadIdx.x; k < P; k += kLsqThreads) {
        const double width = x[4 + 3 * k], loc = x[5 + 3 * k], a = x[6 + 3 * k];
        const double ihw = 2.0 / width;   // (the host has refused a width at or below the floor: finite, |t| <= 1e18)
        const double cl = ihw * kLsqInvPi, cg = ihw * kLsqSqrtLn2OverPi;
        LsqPeakConst c;
        c.ihw = ihw;
        c.locc = loc - w0;
        c.al = a * r * cl;
        c.ag = a * (1.0 - r) * cg;
        c.dl = a * cl;
        c.dg = a * cg;
        c.rl = r * cl;
        c.rg = (1.0 - r) * cg;
        pk[k] = c;
    }
}

// [J | r] of the thread's point j0 + jl of the tile into T[jl][0 .. D]: lane = grid point, the four resident values read at
// grid_slot(j); wave i0 takes the peaks k = i0 (mod 4) and writes their three columns; the waves' sums over their peaks of
// the model and of d/dr meet in `strip` [2][4][64] and are added in wave order 0, 1, 2, 3; after the barrier wave 0 writes
// the phase columns, wave 1 those of r and yoff, wave 2 the residual.  have: the point lies on the grid (else zeros).
// Contains a barrier: every thread of the workgroup calls it.
__device__ __forceinline__ void lsq_form_analytic(double *T, int pitch, double *strip, const double *head, const LsqPeakConst *pk,
                                                  const LsqAnalyticJob &q, const LsqResident &g, int64_t j0, bool have, int i0)
{
    const int jl = threadIdx.x & (kLsqTile - 1);
    const int P = q.P, D = q.D;
    const int64_t j = j0 + jl;
    double wc = 0.0, u = 0.0, v = 0.0, qs = 0.0;
    if (have) {
        const int64_t slot = grid_slot(j);
        wc = g.wc[slot];
        u = g.u[slot];
        v = g.v[slot];
        qs = head[4] * g.wt[slot];
    }
    double *row = T + jl * pitch;
    double msum = 0.0, rsum = 0.0;
#pragma unroll 1
    for (int k = i0; k < P; k += kLsqWaves) {
        const LsqPeakConst c = pk[k];
        const double t = (wc - c.locc) * c.ihw;
        const double t2 = t * t;
        const double iS = 1.0 / (1.0 + t2);
        const double e = exp2(-t2);
        const double L = c.al * iS, G = c.ag * e;
        msum += L + G;
        rsum += c.dl * iS - c.dg * e;
        // |t| <= 1e18 (no width at or below the floor gets here), so t^2 <= 1e36 is finite: where the Gaussian has
        // underflowed, G (1 - 2 ln2 t^2) and t G are 0 times a finite number -- 0, never 0 times infinity
        row[4 + 3 * k] = (qs * (0.5 * c.ihw)) * (L * ((1.0 - t2) * iS) + G * (1.0 - (2.0 * kLsqLn2) * t2));
        row[5 + 3 * k] = -(qs * (2.0 * c.ihw * t)) * (L * iS + kLsqLn2 * G);
        row[6 + 3 * k] = -qs * (c.rl * iS + c.rg * e);
    }
    strip[i0 * kLsqTile + jl] = msum;
    strip[kLsqStrip + i0 * kLsqTile + jl] = rsum;
    __syncthreads();
    if (i0 == 0 || i0 == 2) {
        const double frac = (double)j / head[5];
        double sn, cs;
        sincos(head[0] + head[1] * frac, &sn, &cs);
        if (i0 == 0) {
            const double I = sn * u + cs * v;
            row[0] = -qs * I;
            row[1] = -qs * I * frac;
        } else {
            const double *m = strip + jl;
            const double model = ((m[0] + m[kLsqTile]) + m[2 * kLsqTile]) + m[3 * kLsqTile];
            row[D] = qs * ((cs * u - sn * v) - (model + head[2]));
        }
    } else if (i0 == 1) {
        const double *m = strip + kLsqStrip + jl;
        row[2] = -qs * (((m[0] + m[kLsqTile]) + m[2 * kLsqTile]) + m[3 * kLsqTile]);
        row[3] = -qs * head[3];
    }
}

// the tile out of LDS for a record with J and r: rows j0 .. j0 + nj of the row-major N x D matrix J are nj D consecutive
// doubles -- wave i0 takes every kLsqWaves-th row, its lanes the row's columns (consecutive addresses; no division, whose
// constants lsq_analytic_kernel has no scalar registers for); r is column D.  (lsq_normal_kernel keeps its own write-out in
// its body: its instruction stream is pinned by tools/isa_hash.py.)
template <class Job>
__device__ __forceinline__ void lsq_write_tile(const double *T, int pitch, const Job &q, int D, int64_t j0, int nj, bool have, int i0,
                                               int jl)
{
    if (q.J) {
        double *__restrict__ Jt = q.J + j0 * D;
        for (int jj = i0; jj < nj; jj += kLsqWaves)
            for (int i = jl; i < D; i += kLsqTile) Jt[jj * D + i] = T[jj * pitch + i];
    }
    if (q.r && i0 == 0 && have) q.r[j0 + jl] = T[jl * pitch + D];
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

// lsq_internal.h -- shared by lsq.hip (the kernels of include/nmrfit_amd_lsq.h), lsq_cov.hip (those of
// include/nmrfit_amd_cov.h, nmrfit_sandwich*), lsq_cov_im.hip (those of include/nmrfit_amd_cov_im.h), ctx_eval.hip
// (nmrfit_jacobian*) and batch_lsq.hip (nmrfit_batch_normal_equations*, nmrfit_batch_sandwich*): the per-fit records the
// kernels read and the launches.
#pragma once
#include "nmrfit_amd_lsq.h"
#include "nmrfit_amd_lsq_im.h"
#include "nmrfit_internal.h"

namespace nmrfit {

constexpr int kLsqTile = NMRFIT_LSQ_TILE;            // grid points per tile
constexpr int kLsqMaxSegments = NMRFIT_LSQ_MAX_SEGMENTS;
constexpr int kLsqMaxD = NMRFIT_LSQ_MAX_D;
constexpr int kLsqThreads = 256;
constexpr int kLsqAcc = 12;                          // sums per thread: 256 x 12 >= 76 x 77 / 2 + 76
static_assert(kLsqThreads * kLsqAcc >= kLsqMaxD * (kLsqMaxD + 1) / 2 + kLsqMaxD, "accumulators for the largest D");

// One fit of a normal-equations launch.  R: its D + 1 residual rows, N doubles each, in plain grid order.
struct LsqJob {
    const double *R;
    const double *c;       // D factors s / h_i
    double s;
    int64_t N;
    int32_t D;
    int32_t nseg;          // workgroups (segments of the grid) of this fit: a function of N alone
    int32_t seg_tiles;     // tiles per segment
    int32_t pad;
    double *J;             // N x D row-major, or null
    double *r;             // N, or null
    double *partial;       // nseg x (D (D + 1) / 2 + D), or null: no sums
    double *A;             // D x D
    double *g;             // D
};

// the segments of a grid of N points: at most kLsqMaxSegments, whole tiles each
inline void lsq_segments(int64_t N, int32_t *nseg, int32_t *seg_tiles)
{
    const int64_t tiles = (N + kLsqTile - 1) / kLsqTile;
    const int64_t per = (tiles + kLsqMaxSegments - 1) / kLsqMaxSegments;
    *seg_tiles = (int32_t)per;
    *nseg = (int32_t)((tiles + per - 1) / per);
}
inline int64_t lsq_sums(int64_t D) { return D * (D + 1) / 2 + D; }

// entry o of a fit's sums -> the pair (a, b): the upper triangle row after row, then the D entries of g as (i, D)
__device__ __forceinline__ void lsq_pair(int o, int D, int *a, int *b)
{
    const int ntri = D * (D + 1) / 2;
    if (o >= ntri) {
        *a = o - ntri;
        *b = D;
        return;
    }
    int row = 0, rem = o;
    while (rem >= D - row) {
        rem -= D - row;
        ++row;
    }
    *a = row;
    *b = row + rem;
}

// J, r and -- where a job has `partial` -- A and g of K fits (jobs: device memory), on `st`.  Dmax <= kLsqMaxD.
int launch_lsq(hipStream_t st, const LsqJob *d_jobs, int32_t K, int32_t Dmax, bool sums);

// One job of a meat launch (lsq_cov.hip, lsq_cov_im.hip; the stages: lsq_tile.h): one block of
// Mt_ab = Jt_a^T diag(q_ab) Jt_b.  A fit on the real channel (include/nmrfit_amd_cov.h) is ONE job, kind rr, of D columns:
// Jt = J, Ra = Rb = its residual rows, M = J^T diag(q) J.  A fit on both channels (include/nmrfit_amd_cov_im.h) is FOUR,
// of C = D + 1 columns, Jt_ch = [J_ch | r_ch]: (re, re) and (im, im), the upper triangle of a symmetric block each, and
// (re, im) in two bands of rows.  lsq_meat_kernel reads neither kind, rows nor Ra.
enum { kMeatRR = 0, kMeatII = 1, kMeatRI = 2 };
struct LsqMeatJob {
    const double *Ra;      // the D + 1 residual rows of channel a (the rows of the block), N doubles each
    const double *Rb;      // those of channel b (its columns); Ra for a symmetric kind
    const double *c;       // as the fit's LsqJob has it
    const double *wt;      // the fit's resident weights (grid_slot order, padded to whole chunks)
    double s, p0, p1;      // p0, p1: the phase of row 0
    double var_u, var_v;   // sigma_u^2, sigma_v^2 (kMeatRI: sigma_u^2 - sigma_v^2 in var_u, var_v unused)
    int64_t N;
    int32_t D;
    int32_t nseg, seg_tiles;   // lsq_segments(N)
    int32_t kind;          // kMeat*
    int32_t row0, row1;    // kMeatRI: the job's rows [row0, row1) of the block; else 0, the columns
    double *partial;       // nseg x the sums one segment leaves: a triangle of the columns, or every entry of the band
    double *M;             // the block, row-major
};
inline int lsq_meat_njobs(int nch) { return nch == 2 ? 4 : 1; }
// the rows of the cross block's first band: the second takes the rest
inline int32_t cross_split(int32_t C) { return (C + 1) / 2; }
static_assert(kLsqThreads * kLsqAcc >= (kLsqMaxD + 1) * (kLsqMaxD + 2) / 2, "accumulators for a symmetric block of the largest D");
static_assert(kLsqThreads * kLsqAcc >= ((kLsqMaxD + 2) / 2) * (kLsqMaxD + 1), "accumulators for a band of the cross block");
// doubles of M one fit of D parameters takes: D x D, or on both channels [3][C x C], the blocks rr, ii, ri
inline int64_t meat_doubles(int64_t D, int nch) { return nch == 2 ? 3 * (D + 1) * (D + 1) : D * D; }
// doubles of segment sums the jobs of one fit need
int64_t lsq_meat_partials(int64_t N, int64_t D, int nch);
// the lsq_meat_njobs(nch) jobs of one fit: R its [nch][D + 1][N] residual rows (real plane first), partial
// lsq_meat_partials(N, D, nch) doubles -- the jobs' sums in job order -- and M meat_doubles(D, nch)
void lsq_meat_jobs(LsqMeatJob *job, int nch, const double *R, const double *c, const double *wt, double s, double p0, double p1,
                   double sigma_u, double sigma_v, int64_t N, int32_t D, double *partial, double *M);
// the blocks of njobs jobs of nch channels (device memory), on `st`, after the rows launch that made every R: the kernel
// pair and the LDS of the channel count.  Dmax <= kLsqMaxD.
int launch_lsq_meat(hipStream_t st, const LsqMeatJob *d_jobs, int32_t njobs, int32_t Dmax, int nch);
int launch_lsq_meat_im_kernels(hipStream_t st, const LsqMeatJob *d_jobs, int32_t njobs, int32_t Dmax);   // (lsq_cov_im.hip's half of it)
// NMRFIT_E_INVALID unless both are finite and >= 0
int check_sigma(const char *who, double sigma_u, double sigma_v);
// J and r alone for one fit of any D (no LDS tile): what nmrfit_jacobian runs beyond kLsqMaxD
int launch_lsq_plain(hipStream_t st, const LsqJob &job);

// One fit of an analytic launch (lsq_analytic.hip; include/nmrfit_amd_lsq_analytic.h): no residual rows -- the kernel forms
// [J | r] from the fit's resident arrays (grid_slot order, as the objective kernels read them) and x.
struct LsqAnalyticJob {
    const double *wc, *u, *v, *wt;
    const double *x;       // D = 4 + 3 P parameters, device memory
    double w0, s;
    int64_t N;
    int32_t P, D;
    int32_t nseg, seg_tiles;   // lsq_segments(N)
    double *J;             // N x D row-major, or null
    double *r;             // N, or null
    double *partial;       // nseg x lsq_sums_analytic(D), or null: no sums
    double *A;             // D x D, or null
    double *g;             // D, or null
    double *f;             // 1, or null
};
// the sums of an analytic job: lsq_sums(D) and one more entry, the pair (D, D) = sum_j r_j^2
inline int64_t lsq_sums_analytic(int64_t D) { return lsq_sums(D) + 1; }
static_assert(kLsqThreads * kLsqAcc >= kLsqMaxD * (kLsqMaxD + 1) / 2 + kLsqMaxD + 1, "accumulators for the largest D and f");
// J, r and -- where a job has `partial` -- A, g and f of K fits (jobs: device memory), on `st`.  Dmax <= kLsqMaxD.
int launch_lsq_analytic(hipStream_t st, const LsqAnalyticJob *d_jobs, int32_t K, int32_t Dmax, bool sums);

// One fit of a residual-rows launch over a batch's resident spectra: the grid as BatchFit holds it, S parameter rows
// X [S x D], their objective values f [S] and residual rows R [S x N].  A batch with an imaginary-channel mode may ask for
// the rows of both channels instead (launch_rows_batch, fit_im 1 or 2): R is then [2][S][N], the imaginary rows second,
// and f [S][2] the two RMSEs of every row.
struct RowsFit {
    const double *wc, *u, *v, *wt;
    const double2 *chunk;
    double w0, wspan, lane_step, rec_devk;
    const double *X;
    double *f;
    double *R;
    int64_t N, seg_len, S;
    int32_t P, blk_chunks, n_blocks, pad;
};
// false: these peak counts leave the kernel's LDS records no room
bool rows_batch_lds(int32_t Pmax, int fit_im, size_t *lds, unsigned *aux_off);
int launch_rows_batch(hipStream_t st, const RowsFit *d_fits, int32_t K, int64_t Smax, size_t lds, unsigned aux_off, int fit_im);

}  // namespace nmrfit

/*
 * nmrfit_amd_baseline.h -- least-squares polynomial baselines and noise levels of many spectra on the device (opt-in;
 * found by symbol lookup like the other entry points added within ABI 6: the version number does not change).  The
 * product interface is nmrfit_amd.h.  Same conventions as nmrfit_amd.h.
 *
 * The reference estimates a noise level by a quadratic fit over a signal-free stretch (utils.sample_noise: np.polyfit
 * on raw ppm values, then np.std of what is left) and has one constant, yoff, for the baseline of a fit.  Here one
 * device primitive fits, over a masked part of a grid, a least-squares polynomial in a Chebyshev basis on the masked
 * points' own domain, in a fixed summation order, and returns the coefficients, the baseline at every grid point and
 * the spread of the residual over the mask -- from host arrays, or on the residual data_V - V of the fits of a batch.
 *
 * JOB.  A job is (spectrum k, channel c): N points w_j, values y_j, j = 0 .. N-1, a degree d, 0 <= d <=
 * NMRFIT_BASELINE_MAX_DEG, R >= 0 intervals (lo_r, hi_r) in units of w, swapped if reversed, and a flag `complement`.
 * The channels of a spectrum share w, d, the intervals and the flag.
 *
 * MASK.  in_j is true when lo_r <= w_j <= hi_r for some r (the rule of utils.sample_noise: by value, w in any order).
 * m_j = in_j when complement = 0, m_j = !in_j when complement != 0 (R = 0 with complement: the whole grid).  A NaN w_j
 * is never in the mask, whatever the flag.  An infinite edge is valid.
 *
 * DOMAIN.  n = sum m_j; a and b are the smallest and the largest masked w_j.  n = 0: status 1 (empty; a and b are
 * NaN).  n < d + 1: status 2 (rank), nothing is solved.  Else
 *   t_j = ((w_j - a) - (b - w_j)) / (b - a)        every operation rounded once;  t_j = 0 for every j if b == a
 * for EVERY j of the grid, masked or not (|t_j| > 1 outside [a, b]).
 *
 * BASIS.  T_0 = 1, T_1 = t, T_k = (2 t) T_{k-1} - T_{k-2}: the product rounded, then the difference (no fused
 * multiply-add anywhere in this header).
 *
 * SUMS, over the masked points:
 *   mu_k = sum T_k(t_j)            k = 0 .. 2 d
 *   g_i  = sum T_i(t_j) * y_j      i = 0 .. d          (each product rounded, then summed)
 *   G_ik = 0.5 * (mu_{i+k} + mu_{|i-k|})                (T_i T_k = (T_{i+k} + T_{|i-k|}) / 2: 3 d + 2 sums in all)
 *
 * SUMMATION ORDER.  Point j is lane j % 64 of wave (j % 256) / 64.  A lane starts from +0.0 and adds its terms (+0.0
 * for a point outside the mask) over the tiles j / 256 in ascending order into ONE running sum.  Then
 *   1. within a wave: x[l] += x[l + 32] for l < 32, then x[l] += x[l ^ 16], l ^ 8, l ^ 4, l ^ 2, l ^ 1; lane 0 holds the sum
 *   2. ((wave 0 + wave 1) + wave 2) + wave 3
 * (step 1 is step 1 of nmrfit_amd_quality.h; the order across tiles is NOT quality's: a wave tree per tile for up to
 * 26 sums would cost more than the arithmetic.)  There are no floating-point atomics: a row is a pure function of
 * (w, y, mask, d) -- the same alone, in any batch, as either channel, through either entry point, from call to call.
 *
 * SOLVE.  G c = g by L D L^T without pivoting and without square roots; every multiply, subtract and divide rounded:
 *   for j = 0 .. d:
 *       v_k = L_jk * D_k                                      k = 0 .. j-1
 *       s = G_jj;  s = s - L_jk * v_k                         k = 0 .. j-1 ascending;   D_j = s
 *       status 2 (rank) unless D_j > 0 (a NaN included); nothing further is computed
 *       for i = j+1 .. d:  s = G_ij;  s = s - L_ik * v_k      k = 0 .. j-1 ascending;   L_ij = s / D_j
 *   for i = 0 .. d:     z_i = g_i;  z_i = z_i - L_ik * z_k    k = 0 .. i-1 ascending
 *   for i = 0 .. d:     z_i = z_i / D_i
 *   for i = d .. 0:     c_i = z_i;  c_i = c_i - L_ki * c_k    k = i+1 .. d ascending
 * The row carries (min_j D_j) / (max_j D_j), so that a caller can judge a thin mask.
 *
 * BASELINE.  b_j = c_0, then b_j = b_j + c_i * T_i(t_j) for i = 1 .. d (the product rounded, then added), for every j
 * of the grid.
 *
 * SPREAD.  r_j = y_j - b_j.  S1 = sum_mask r_j;  rbar = S1 / n;  S2 = sum_mask (r_j - rbar)^2 (the difference
 * rounded, its square rounded), both in the order above.  The caller forms sigma = sqrt(S2 / n): np.std with ddof 0,
 * as utils.sample_noise does.
 *
 * ROW.  NMRFIT_BASELINE_ROW doubles per job:
 *   0 status (0 fitted, 1 empty mask, 2 rank)   1 n   2 a   3 b   4 S1   5 S2   6 min D / max D   7 d
 *   8 .. 16   c_0 .. c_8 (zero above d)
 * With status != 0 entries 4, 5, 6, c_0 .. c_d and the job's baseline values are NaN.  A NaN y_j inside the mask leaves
 * status 0 and makes the coefficients, the baseline and the sums NaN; outside the mask it touches nothing that is
 * returned.
 */
#ifndef NMRFIT_AMD_BASELINE_H
#define NMRFIT_AMD_BASELINE_H

#include "nmrfit_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* the largest degree */
#define NMRFIT_BASELINE_MAX_DEG 8
/* doubles per row */
#define NMRFIT_BASELINE_ROW 17
/* intervals per spectrum: a job's workgroup stages them in LDS, 16 bytes each.  1024 of them are 16 KiB, with the
 * waves' partial sums and the solve 18 KiB per workgroup: eight such workgroups fit a CU's 160 KiB, and eight
 * workgroups of 256 threads are all the wave slots of a CU hold -- the largest power of two that costs no residency. */
#define NMRFIT_BASELINE_MAX_INTERVALS 1024

/* The rows of K spectra x C channels from host arrays.  The K spectra are laid out one after the other as in
 * nmrfit_batch_create_ragged: spectrum k has N[k] > 0 points of w; y: C planes of N[0] + ... + N[K-1] doubles, channel
 * after channel; deg[k], R[k], complement[k] per spectrum; edges: 2 doubles per interval, spectrum after spectrum.
 * rows_out: C planes of K rows; baseline_out: C planes like y, or NULL.  Host pointers both ways.  Synchronous.
 * NMRFIT_E_INVALID, reported before any device work: a null pointer (edges may be null when no spectrum has an
 * interval, baseline_out may be null), K <= 0, N[k] <= 0, R[k] < 0, deg[k] outside 0 .. NMRFIT_BASELINE_MAX_DEG, C
 * outside {1, 2}, a NaN edge.  NMRFIT_E_UNSUPPORTED: K > 65535, N[0] + ... + N[K-1] > 2^26 (the limits of
 * nmrfit_weights_build), or an R[k] > NMRFIT_BASELINE_MAX_INTERVALS. */
int nmrfit_baseline_fit(int device, int32_t K, const int64_t *N, const double *w, int32_t C, const double *y,
                        const int32_t *deg, const int32_t *R, const double *edges, const int32_t *complement,
                        double *rows_out, double *baseline_out);

/* The same for the residual of the fits of a created batch, on its resident spectra: one channel, y_j = d_j - V_j with
 * V_j and d_j as in nmrfit_amd_quality.h (the reconstruction's own bits), w the grids as they were uploaded.  x: the K
 * parameter vectors one after the other (4 + 3 P_k doubles), allowed in any state of the batch; or NULL: every fit's
 * best position -- NMRFIT_E_STATE before the first generation, or while a reconstruction of the batch is in flight.
 * deg, R, edges, complement as above; rows_out: K rows; baseline_out: the batch's points, fit after fit, or NULL.  The
 * swarms are not touched.  A null handle, deg, R, complement or rows_out, R[k] < 0, a deg[k] out of range, edges null
 * where there is an interval, or a NaN edge is NMRFIT_E_INVALID; an R[k] > NMRFIT_BASELINE_MAX_INTERVALS is
 * NMRFIT_E_UNSUPPORTED.  Synchronous. */
int nmrfit_batch_residual_baseline(nmrfit_batch *batch, const double *x, const int32_t *deg, const int32_t *R,
                                   const double *edges, const int32_t *complement, double *rows_out, double *baseline_out);

#ifdef __cplusplus
}
#endif
#endif /* NMRFIT_AMD_BASELINE_H */

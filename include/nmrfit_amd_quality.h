/*
 * nmrfit_amd_quality.h -- residual statistics of finished fits on the device (opt-in; found by symbol lookup like the
 * other entry points added within ABI 6: the version number does not change).  The product interface is nmrfit_amd.h.
 * Same conventions as nmrfit_amd.h.
 *
 * The reference judges a fit by a plot of fit.V - data.V (plot.residual; panel E of plot.isotope_ratio).  At the batched
 * fit rates nobody reads plots: here the residual is reduced on the device, per region of the grid and in a fixed order,
 * and (R + 2) rows of 64 bytes per fit come back instead of the (2 P + 6) N doubles of the reconstruction.
 *
 * THE RESIDUAL.  For one fit with parameters x (4 + 3 P doubles) on its own grid of N points, j = 0 .. N-1:
 *   V_j   the summed real lines at w_j: what nmrfit_generate_result / nmrfit_batch_contributions return as fit_out[0][j]
 *   d_j   cos(phi_j) u_j - sin(phi_j) v_j, phi_j = x[0] + (x[1] j) / N: what they return as data_out[0][j]
 *   e_j = V_j - d_j      (plot.residual's ys - y_data on the real channel; unweighted: the weights are the optimiser's)
 * V_j and d_j are the reconstruction's own bits (one device function evaluates them in both kernels).
 *
 * REGIONS AND ROWS.  A region is a pair of edges in units of w.  It covers the indices first .. last inclusive: first
 * and last are the nearest grid points to the two edges as np.argmin(|w - edge|) finds them (the lowest index on ties;
 * an infinite edge: every distance is infinite, index 0), swapped if reversed -- the rule of utils.compute_weights /
 * nmrfit_weights_build, evaluated by the same launch; w in any order.  Regions may overlap; a point counts in every
 * region that holds it.  A fit with R regions gives R + 2 rows:
 *   rows 0 .. R-1   the regions, in the caller's order
 *   row  R          the whole grid
 *   row  R+1        the complement of the union of the regions (the whole grid when R = 0)
 * Each row is 8 doubles:
 *   0   n, the number of points in the row
 *   1   sum e_j
 *   2   sum e_j * e_j                  (each product rounded once, then summed: no fused multiply-add)
 *   3   sum (e_j - e_{j-1})^2          over the j for which both j and j-1 are in the row (the difference rounded, its
 *                                      square rounded, then summed; in the complement row: index-adjacent pairs only)
 *   4   sum d_j
 *   5   sum d_j * d_j
 *   6   max |e_j| over the row's points whose e_j is not NaN; 0 when there is none
 *   7   the lowest index j that attains that maximum, as a double; -1 when there is none (an empty row)
 *
 * SUMMATION ORDER.  Point j belongs to tile j / 256, wave (j % 256) / 64 and lane j % 64.  To each sum a lane contributes
 * its term, or +0.0 if its point is outside the row or past N.
 *   1. within a wave: x[l] += x[l + 32] for l < 32, then x[l] += x[l ^ 16], l ^ 8, l ^ 4, l ^ 2, l ^ 1; lane 0 holds the sum
 *   2. within a tile: ((wave 0 + wave 1) + wave 2) + wave 3
 *   3. across tiles:  ((tile 0 + tile 1) + tile 2) + ...  over ALL tiles of the grid, ascending
 * There are no floating-point atomics: the rows are a pure function of (spectrum, x, regions) -- the same for a lone fit,
 * in any batch, through either entry point, at any launch geometry and from call to call.  A NaN in u or v makes the sums
 * of the rows that hold its point NaN (two pair terms of sum 3); quantities 0, 6 and 7 are those of the other points.
 */
#ifndef NMRFIT_AMD_QUALITY_H
#define NMRFIT_AMD_QUALITY_H

#include "nmrfit_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* doubles per row */
#define NMRFIT_QUALITY_ROW 8
/* regions per fit: a workgroup stages its fit's (first, last) pairs in LDS next to the per-peak records */
#define NMRFIT_QUALITY_MAX_REGIONS 2048

/* The rows of K fits from host arrays.  The K spectra are laid out one after the other as in nmrfit_batch_create_ragged:
 * spectrum k has N[k] > 0 points of w, u and v; x: the K parameter vectors one after the other, 4 + 3 P[k] doubles each;
 * R[k] >= 0 regions per fit, edges: 2 doubles per region, fit after fit; out: (R[0] + 2 + ... + R[K-1] + 2) * 8 doubles,
 * fit after fit.  Host pointers in both directions.  Synchronous.
 * NMRFIT_E_INVALID, reported before any device work: a null pointer (edges may be null when no fit has a region),
 * K <= 0, N[k] <= 0, R[k] < 0, P[k] < 0 or above the library's peak limit, a NaN edge.  An infinite edge is valid.
 * NMRFIT_E_UNSUPPORTED: K > 65535, N[0] + ... + N[K-1] > 2^26 (the limits of nmrfit_weights_build), or an
 * R[k] > NMRFIT_QUALITY_MAX_REGIONS. */
int nmrfit_quality_stats(int device, int32_t K, const int64_t *N, const double *w, const double *u, const double *v,
                         const int32_t *P, const double *x, const int32_t *R, const double *edges, double *out);

/* The same on the resident spectra of a created batch (after nmrfit_batch_add_noise: the replicas), one launch per part
 * of the batch on the part's stream.  x: the K parameter vectors one after the other (4 + 3 P_k doubles, the batch's
 * peak counts), allowed in any state of the batch; or NULL: every fit's best position -- NMRFIT_E_STATE before the first
 * generation, or while a reconstruction of the batch is in flight.  R, edges, out as above.  The swarms are not touched.
 * A null handle, R or out, R[k] < 0, edges null where there is a region, or a NaN edge is NMRFIT_E_INVALID; an
 * R[k] > NMRFIT_QUALITY_MAX_REGIONS is NMRFIT_E_UNSUPPORTED.  Synchronous. */
int nmrfit_batch_quality_stats(nmrfit_batch *batch, const double *x, const int32_t *R, const double *edges, double *out);

#ifdef __cplusplus
}
#endif
#endif /* NMRFIT_AMD_QUALITY_H */

/*
 * nmrfit_amd_lsq_analytic.h -- the analytic Jacobian of a fit's real-channel residual on the device (opt-in; found by
 * symbol lookup like the other entry points added within ABI 6: the version number does not change).  The product
 * interface is nmrfit_amd.h; nmrfit_amd_lsq.h is the forward-difference form of the same quantities.  Same conventions.
 *
 * For a fit with grid w_j (j < N), data (u_j, v_j), weights wt_j, s = 1 / sqrt(N) and
 * x = (p0, p1, r, yoff, width_k, loc_k, a_k, ...), D = 4 + 3 P:
 *   phi_j = p0 + p1 j / N     V_j = cos(phi_j) u_j - sin(phi_j) v_j     I_j = sin(phi_j) u_j + cos(phi_j) v_j
 *   ihw = 2 / width   t = (w_j - loc) ihw   S = 1 + t^2
 *   Lh = ihw / (pi S)         Gh = ihw sqrt(ln2 / pi) 2^(-t^2)          L = a r Lh     G = a (1 - r) Gh
 *   r[j]    = s wt_j (V_j - sum_k (yoff + L_k + G_k))                   ||r|| is the objective
 *   J[j][i] = d r[j] / d x_i, in closed form, with q = s wt_j:          N x D, row-major
 *     p0: -q I_j     p1: -q I_j (j / N)     r: -q sum_k a_k (Lh_k - Gh_k)     yoff: -q P
 *     width_k: +q (ihw / 2) (L (1 - t^2) / S + G (1 - 2 ln2 t^2))
 *     loc_k:   -q 2 ihw t (L / S + ln2 G)           a_k: -q (r Lh + (1 - r) Gh)
 *   A = J^T J    D x D, row-major, symmetric as returned        g = J^T r    D        f = sqrt(sum_j r[j]^2)
 * No residual rows are launched and no steps are taken: one kernel forms [J | r] tile by tile from the resident
 * spectrum and sums its products, a second adds the per-segment sums.  A, g and f are summed in a fixed order that depends
 * on N and P alone: the same inputs give the same bits on every run, alone or in any batch.  No floating-point atomics.
 * The formulas hold for negative widths, r outside [0, 1], a <= 0 and P = 0.  f is this call's own sum: it agrees with
 * the objective kernels' value to rounding, not bit for bit.
 *
 * Refused with NMRFIT_E_INVALID before any launch: a parameter that is not finite; a width of zero or below the kernels'
 * floor, |2 / width| > 1e18 / (wspan + |loc - w0|) (w0 the grid's middle value, wspan = max_j |w_j - w0|), where the
 * library evaluates the line of the floor width and the model does not move with the width.
 * D <= NMRFIT_LSQ_MAX_D for every output, J included (else NMRFIT_E_UNSUPPORTED).
 */
#ifndef NMRFIT_AMD_LSQ_ANALYTIC_H
#define NMRFIT_AMD_LSQ_ANALYTIC_H

#include "nmrfit_amd_lsq.h"

#ifdef __cplusplus
extern "C" {
#endif

/* One fit on a context, whatever kernel variant it is set to.  x: D values on the host, required.  Any output pointer may
 * be NULL: J_out N x D, r_out N, A_out D x D, g_out D, f_out 1 (all on the host; the data is there on return). */
int nmrfit_jacobian_analytic(nmrfit_ctx *ctx, int32_t P, const double *x,
                             double *J_out, double *r_out, double *A_out, double *g_out, double *f_out);

/* Every fit of a device batch, from the batch's resident spectra: two launches per part.  Ragged in D, laid out as
 * nmrfit_batch_normal_equations lays it out: x fit k's D_k values at o1_k, A_out fit k's D_k x D_k block at o2_k, g_out
 * fit k's D_k values at o1_k, f_out K values.  x is required; any output pointer may be NULL.  Fits are processed in
 * groups when their per-segment sums exceed the workspace budget (256 MiB; NMRFIT_LSQ_WORKSPACE_MB overrides): the grouping
 * changes no bit of any result.  Every fit's A, g and f are bit-identical to nmrfit_jacobian_analytic's on a context of the
 * same spectrum.  A batch created with a fit_im mode is served its real channel.  NMRFIT_E_STATE while a reconstruction of
 * the batch is in flight.  A refused call leaves the batch as it was. */
int nmrfit_batch_normal_equations_analytic(nmrfit_batch *batch, const double *x,
                                           double *A_out, double *g_out, double *f_out);

#ifdef __cplusplus
}
#endif
#endif /* NMRFIT_AMD_LSQ_ANALYTIC_H */

/*
 * nmrfit_amd_cov_im.h -- the first-order covariance of a fit made on BOTH channels (fit_im = 1 or 2) from one Jacobian
 * (opt-in; found by symbol lookup like the other entry points added within ABI 6: the version number does not change).
 * nmrfit_amd_cov.h covers the real channel and refuses such fits; this is their entrance.  Same conventions.
 *
 * The fit minimises f = (rho_re + rho_im) / 2, a mean of two norms (nmrfit_amd_lsq_im.h).  Its estimator solves
 * grad f = sum_ch J_ch^T r_ch / (2 rho_ch) = 0; linearised in the data with J held fixed, the score moves by
 *   d(grad f) = 1/2 sum_ch (1 / rho_ch) B_ch Jt_ch^T dr_ch,    Jt_ch = [ J_ch | r_ch ]   N x C, C = D + 1
 *                                                              B_ch  = [ I_D | -g_ch / rho_ch^2 ]   D x C
 * (the last column of Jt carries the derivative of 1 / rho_ch).  With independent noise of standard deviation sigma_u on u
 * and sigma_v on v, V_j = u_j cos phi_j - v_j sin phi_j, I_j = u_j sin phi_j + v_j cos phi_j, phi_j = p0 + p1 * (j / N),
 * ws_j = weights_j * s, the weighted residuals of a grid point have the covariances
 *   q_rr,j = ws_j^2 (cos^2 phi_j sigma_u^2 + sin^2 phi_j sigma_v^2)
 *   q_ii,j = ws_j^2 (sin^2 phi_j sigma_u^2 + cos^2 phi_j sigma_v^2)
 *   q_ri,j = ws_j^2 cos phi_j sin phi_j (sigma_u^2 - sigma_v^2)
 * and the device returns the three C x C blocks
 *   Mt_ab[x][y] = sum_j (q_ab,j * Jt_a[j][x]) * Jt_b[j][y],    ab in (rr, ii, ri);   Mt_ir = Mt_ri^T is not returned
 * next to A_ch, g_ch and rho_ch, which are nmrfit_jacobian_im / nmrfit_batch_normal_equations_im's own bits (the same
 * launches).  The D x D algebra -- H = 1/2 sum_ch (A_ch / rho_ch - g_ch g_ch^T / rho_ch^3), the meat
 * M = 1/4 sum_ab B_a Mt_ab B_b^T / (rho_a rho_b), cov = H^-1 M H^-1 over the free parameters -- is the caller's
 * (nmrfit_amd/uncertainty.py, covariance_im).
 *
 * Every sum runs over the grid in an order that N alone fixes -- per-segment sums over whole tiles of NMRFIT_LSQ_TILE
 * points, then the segments one after the other -- with the expressions of nmrfit_amd_cov.h: the D x D corner of Mt_rr is
 * bit for bit nmrfit_sandwich's M for the same spectrum, weights, rows and sigmas; Mt_ri is exactly 0 for
 * sigma_u == sigma_v.  The symmetric blocks come back with both triangles written from one sum.  No atomics: the same
 * inputs give the same bits on every run, on a context or anywhere in any batch.  The kernel does not know the mode: 1
 * (the reference's fit_im=True) and 2 (the sum over all peaks) differ in the rows it reads.
 * D = 4 + 3 P <= NMRFIT_LSQ_MAX_D, else NMRFIT_E_UNSUPPORTED.  sigma_u, sigma_v: finite and >= 0, else NMRFIT_E_INVALID.
 */
#ifndef NMRFIT_AMD_COV_IM_H
#define NMRFIT_AMD_COV_IM_H

#include "nmrfit_amd_lsq_im.h"

#ifdef __cplusplus
extern "C" {
#endif

/* One fit on a context.  rows: (D + 1) x D, c: D, both on the host and required; fit_im 1 or 2 (else NMRFIT_E_INVALID).
 * Any output pointer may be NULL: A_out [2][D x D], g_out [2][D], rho_out [2], M_out [3][C x C] (rr, ii, ri; all on the
 * host, the data is there on return).  NMRFIT_E_UNSUPPORTED on a context whose kernel variant is not DEFAULT (as for
 * nmrfit_jacobian_im).  A refused call leaves the context as it was. */
int nmrfit_sandwich_im(nmrfit_ctx *ctx, int32_t P, int fit_im, const double *rows, const double *c, double s,
                       double sigma_u, double sigma_v,
                       double *A_out, double *g_out, double *rho_out, double *M_out);

/* Every fit of a device batch, in the batch's own imaginary-channel mode, from its resident spectra and weights.  rows, c,
 * s, the layouts of A_out, g_out and rho_out (f2_out there), the ragged offsets and the grouping under the workspace
 * budget (NMRFIT_LSQ_WORKSPACE_MB: no bit depends on it) are nmrfit_batch_normal_equations_im's; sigma_u, sigma_v: K values
 * each, required; M_out: fit k's [3][C_k x C_k] behind those of the fits before it.  Any output pointer may be NULL.
 * NMRFIT_E_INVALID for a batch created with fit_im = 0; NMRFIT_E_STATE while a reconstruction of the batch is in
 * flight.  A refused or failed call leaves the batch usable and its swarms untouched. */
int nmrfit_batch_sandwich_im(nmrfit_batch *batch, const double *rows, const double *c, const double *s,
                             const double *sigma_u, const double *sigma_v,   /* K values each */
                             double *A_out, double *g_out, double *rho_out, double *M_out);

#ifdef __cplusplus
}
#endif
#endif /* NMRFIT_AMD_COV_IM_H */

/*
 * nmrfit_amd_lsq_im.h -- least squares on BOTH channels: the imaginary residual rows of a fit, their Jacobian and normal
 * equations per channel (opt-in; found by symbol lookup like the other entry points added within ABI 6: the version number
 * does not change).  nmrfit_amd_lsq.h sees the real channel only; a fit made with fit_im = 1 (the reference's fit_im=True:
 * the imaginary model is the LAST peak's dispersion line) or 2 (the sum over all peaks) minimises
 *   f = (rho_re + rho_im) / 2,     rho_ch = RMSE of channel ch
 * and the entry points here give what a refinement of THAT function needs.  Same conventions as nmrfit_amd_lsq.h: D + 1
 * forward-difference parameter rows, c_i = s / h_i, s = 1 / sqrt(N).  With ch in {0: re, 1: im} and R_ch the D + 1
 * residual rows of channel ch,
 *   R_re[b][j] = weights_j (Vd_bj - Vf_bj)            what nmrfit_residual_batch returns, bit for bit
 *   R_im[b][j] = weights_j (Id_bj - If_bj)            If of the mode: the residual the objective kernel squares and sums
 *   r_ch[j]    = R_ch[0][j] * s
 *   J_ch[j][i] = (R_ch[i + 1][j] - R_ch[0][j]) * c_i  N x D, row-major
 *   A_ch       = J_ch^T J_ch,   g_ch = J_ch^T r_ch
 *   f2         = (rho_re, rho_im) of row 0: the rows launch's own values; (f2[0] + f2[1]) / 2 is the objective
 * J and r are bit-identical to the same expressions on the host.  A (fit, channel) pair is one job of the reduction
 * kernel of nmrfit_amd_lsq.h: the same summation orders, fixed by N; no floating-point atomics anywhere.
 * The combination a damped Gauss-Newton step uses -- H = (A_re / rho_re + A_im / rho_im) / 2, the gradient
 * (g_re / rho_re + g_im / rho_im) / 2 -- is D x D host arithmetic and is left to the caller (nmrfit_amd.lsq.combine_channels).
 *
 * The rows of both channels come from the DEFAULT kernel only: a context set to another variant, or with so many peaks
 * that DEFAULT's LDS records do not fit, is NMRFIT_E_UNSUPPORTED.  fit_im must be 1 or 2 (else NMRFIT_E_INVALID).
 */
#ifndef NMRFIT_AMD_LSQ_IM_H
#define NMRFIT_AMD_LSQ_IM_H

#include "nmrfit_amd_lsq.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Residual rows of both channels of B parameter rows X [B x D] (host).  R_out [2][B][N]: the real rows, then the imaginary
 * rows (required); f2_out [B][2]: (rho_re, rho_im) of every row (may be NULL). */
int nmrfit_residual_batch_im(nmrfit_ctx *ctx, int64_t B, int32_t P, const double *X, int fit_im, double *R_out, double *f2_out);

/* One fit on a context, per channel.  rows: (D + 1) x D, c: D, both on the host and required.  Any output pointer may be
 * NULL: J_out [2][N x D], r_out [2][N], A_out [2][D x D], g_out [2][D], f2_out [2].  A and g need D <= NMRFIT_LSQ_MAX_D
 * (else NMRFIT_E_UNSUPPORTED); J, r and f2 have no such limit. */
int nmrfit_jacobian_im(nmrfit_ctx *ctx, int32_t P, const double *rows, const double *c, double s, int fit_im,
                       double *J_out, double *r_out, double *A_out, double *g_out, double *f2_out);

/* Every fit of a device batch, in the batch's own imaginary-channel mode.  rows, c and s as
 * nmrfit_batch_normal_equations takes them (all required); the outputs carry a leading channel index per fit:
 *   A_out  fit k's [2][D_k x D_k] at 2 o2_k        g_out  fit k's [2][D_k] at 2 o1_k        f2_out  fit k's (rho_re, rho_im) at 2 k
 * Any output pointer may be NULL.  The workspace grouping (NMRFIT_LSQ_WORKSPACE_MB) counts the rows of both channels and
 * changes no bit of any result.  Every fit's A, g and f2 are bit-identical to nmrfit_jacobian_im's on a context of the
 * same spectrum.  A batch created with fit_im = 0 is NMRFIT_E_INVALID; NMRFIT_E_STATE while a reconstruction of the batch
 * is in flight.  A failed call leaves the batch usable. */
int nmrfit_batch_normal_equations_im(nmrfit_batch *batch, const double *rows, const double *c, const double *s,
                                     double *A_out, double *g_out, double *f2_out);

#ifdef __cplusplus
}
#endif
#endif /* NMRFIT_AMD_LSQ_IM_H */

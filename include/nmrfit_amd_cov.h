/*
 * nmrfit_amd_cov.h -- the first-order covariance of a fit's parameters from one Jacobian (opt-in; found by symbol
 * lookup like the other entry points added within ABI 6: the version number does not change).  The product interface is
 * nmrfit_amd.h; a binding that reports no uncertainties needs nothing here.  Same conventions as nmrfit_amd.h.
 *
 * The fit minimises a WEIGHTED residual whose weights are not 1 / sigma, so sigma^2 (J^T J)^-1 / N is not the
 * covariance of its parameters; the sandwich A^-1 M A^-1 is.  With the quantities of nmrfit_amd_lsq.h -- the D + 1
 * parameter rows of a forward-difference Jacobian, c_i = s / h_i, s = 1 / sqrt(N), R their residual rows,
 * J[j][i] = (R[i + 1][j] - R[0][j]) * c_i, A = J^T J, g = J^T r -- and independent noise of standard deviation sigma_u on
 * u and sigma_v on v, V_data,j = u_j cos phi_j - v_j sin phi_j with phi_j = p0 + p1 * (j / N), p0 and p1 the first two
 * parameters of row 0:
 *   omega_j  = cos^2 phi_j * sigma_u^2 + sin^2 phi_j * sigma_v^2       variance of V_data,j
 *   q_j      = (weights_j * s)^2 * omega_j                             variance of r_j
 *   M[a][b]  = sum_j (q_j * J[j][a]) * J[j][b]                         D x D, row-major, symmetric as returned
 * The calls return A, M, g and f; the D x D algebra (bounds, scaling, Cholesky, the area fraction) is the caller's
 * (nmrfit_amd/uncertainty.py).  A, g and f are bit for bit what nmrfit_jacobian / nmrfit_batch_normal_equations return
 * for the same rows: they come from the same launches.  M is summed like A, in an order that N alone fixes (per-segment
 * sums over whole tiles of NMRFIT_LSQ_TILE points, then the segments one after the other, both triangles written from
 * one sum): the same inputs give the same bits on every run, on a context or anywhere in any batch.  No atomics.
 * The weights are the resident ones (the context's, the batch's); q_j is formed in fp64 on the device.
 * Real channel only: a fit made with fit_im minimises a mean of two norms, and is refused here (its entrance is
 * nmrfit_amd_cov_im.h: nmrfit_sandwich_im, nmrfit_batch_sandwich_im).
 * D = 4 + 3 P <= NMRFIT_LSQ_MAX_D, else NMRFIT_E_UNSUPPORTED.  sigma_u, sigma_v: finite and >= 0, else NMRFIT_E_INVALID.
 */
#ifndef NMRFIT_AMD_COV_H
#define NMRFIT_AMD_COV_H

#include "nmrfit_amd_lsq.h"

#ifdef __cplusplus
extern "C" {
#endif

/* One fit on a context.  rows: (D + 1) x D, c: D, both on the host and required.  Any output pointer may be NULL:
 * A_out D x D, M_out D x D, g_out D, f_out 1 (all on the host; the data is there on return).  NMRFIT_E_UNSUPPORTED on a
 * context whose kernel variant is not DEFAULT (as for nmrfit_jacobian_im).  A refused call leaves the context as it was. */
int nmrfit_sandwich(nmrfit_ctx *ctx, int32_t P, const double *rows, const double *c, double s,
                    double sigma_u, double sigma_v,
                    double *A_out, double *M_out, double *g_out, double *f_out);

/* Every fit of a device batch, from the batch's resident spectra and weights.  rows, c, s, the ragged offsets and the
 * grouping under the workspace budget (NMRFIT_LSQ_WORKSPACE_MB: no bit depends on it) are
 * nmrfit_batch_normal_equations's; sigma_u, sigma_v: K values each, required; M_out is laid out like A_out.  Any output
 * pointer may be NULL.  NMRFIT_E_UNSUPPORTED for a batch created with a fit_im mode; NMRFIT_E_STATE while a
 * reconstruction of the batch is in flight.  A refused or failed call leaves the batch usable and its swarms untouched. */
int nmrfit_batch_sandwich(nmrfit_batch *batch, const double *rows, const double *c, const double *s,
                          const double *sigma_u, const double *sigma_v,   /* K values each */
                          double *A_out, double *M_out, double *g_out, double *f_out);

#ifdef __cplusplus
}
#endif
#endif /* NMRFIT_AMD_COV_H */

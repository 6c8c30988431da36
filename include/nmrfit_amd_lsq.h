/*
 * nmrfit_amd_lsq.h -- the least-squares pieces of a fit on the device (opt-in; found by symbol lookup like the other
 * entry points added within ABI 6: the version number does not change).  The product interface is nmrfit_amd.h; a
 * binding that does not polish needs nothing here.  Same conventions as nmrfit_amd.h.
 *
 * For a fit with N grid points and D = 4 + 3 P parameters the caller hands over the D + 1 parameter rows of a
 * forward-difference Jacobian (row 0: x; row i + 1: x with component i moved by the realised step h_i), the D factors
 * c_i = s / h_i (negative where the step was flipped at the upper bound) and s = 1 / sqrt(N): the device never divides.
 * With R the D + 1 residual rows of those parameter rows (what nmrfit_residual_batch returns for them, bit for bit):
 *   r[j]        = R[0][j] * s
 *   J[j][i]     = (R[i + 1][j] - R[0][j]) * c_i          N x D, row-major
 *   A           = J^T J                                  D x D, row-major, symmetric as returned
 *   g           = J^T r                                  D
 *   f           = the objective value the rows launch itself returns for row 0
 * J and r are bit-identical to the same expressions evaluated on the host.  A and g are summed in a fixed order that
 * depends on N alone (per-workgroup partial sums over a segment of the grid, then the partials one after the other): the
 * same inputs give the same bits on every run, alone or in any batch.  No floating-point atomics anywhere.
 * A and g need D <= NMRFIT_LSQ_MAX_D (else NMRFIT_E_UNSUPPORTED); J, r and f have no such limit.
 */
#ifndef NMRFIT_AMD_LSQ_H
#define NMRFIT_AMD_LSQ_H

#include "nmrfit_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* largest D = 4 + 3 P (P = 24) whose normal equations the reduction kernel holds in its accumulators */
#define NMRFIT_LSQ_MAX_D 76
/* grid points per tile of the reduction kernel, and the most workgroups (segments of the grid) per fit */
#define NMRFIT_LSQ_TILE 64
#define NMRFIT_LSQ_MAX_SEGMENTS 64

/* One fit on a context.  rows: (D + 1) x D, c: D, both on the host and required.  Any output pointer may be NULL:
 * J_out N x D, r_out N, A_out D x D, g_out D, f_out 1 (all on the host; the data is there on return). */
int nmrfit_jacobian(nmrfit_ctx *ctx, int32_t P, const double *rows, const double *c, double s,
                    double *J_out, double *r_out, double *A_out, double *g_out, double *f_out);

/* Every fit of a device batch, from the batch's resident spectra: residual rows of all K fits in one launch, the normal
 * equations in two more.  Ragged in D: with D_k = 4 + 3 P_k of fit k (the P given at creation) and
 * o1_k = sum_{i<k} D_i, o2_k = sum_{i<k} D_i^2, oR_k = sum_{i<k} (D_i + 1) D_i,
 *   rows   fit k's (D_k + 1) x D_k block at oR_k        c      fit k's D_k factors at o1_k      s   K values
 *   A_out  fit k's D_k x D_k block at o2_k              g_out  fit k's D_k values at o1_k       f_out   K values
 * rows, c and s are required; any output pointer may be NULL.  Fits are processed in groups when their residual rows
 * exceed the workspace budget (256 MiB; NMRFIT_LSQ_WORKSPACE_MB overrides): the grouping changes no bit of any result.
 * Every fit's A, g and f are bit-identical to nmrfit_jacobian's on a context of the same spectrum (DEFAULT variant).
 * NMRFIT_E_STATE while a reconstruction of the batch is in flight.  A failed call leaves the batch usable. */
int nmrfit_batch_normal_equations(nmrfit_batch *batch, const double *rows, const double *c, const double *s,
                                  double *A_out, double *g_out, double *f_out);

#ifdef __cplusplus
}
#endif
#endif /* NMRFIT_AMD_LSQ_H */

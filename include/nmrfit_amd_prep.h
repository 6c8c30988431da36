/*
 * nmrfit_amd_prep.h -- preparation stages of batched fits on the device (opt-in; found by symbol lookup like the other
 * entry points added within ABI 6: the version number does not change).  The product interface is nmrfit_amd.h; a
 * binding that uploads its own weights needs nothing here.  Same conventions as nmrfit_amd.h.
 *
 * The error weights of a fit (FitUtility._compute_weights, nmrfit/utils.py:191-224): every peak claims the grid points
 * between the two points nearest to its bounds at the level (tallest |height| / its |height|) ** expon, later peaks
 * overwrite earlier ones, unclaimed points weigh 1, and ten sweeps of equations.laplace1d (nmrfit/equations.py:215-238)
 * round the steps off.  Here for a ragged batch of S spectra laid out one after the other as in
 * nmrfit_batch_create_ragged: spectrum k has N[k] > 0 grid points of w (in ANY order: ascending, descending, unsorted,
 * with duplicates or NaN) and R[k] >= 0 regions; region r of the concatenated tables is
 *   edges[2 r], edges[2 r + 1]   the peak's bounds (b0, b1), in either order
 *   level[r]                     its level, formed by the CALLER with the scalar power the reference calls (the device
 *                                never calls pow)
 * The nearest point to a bound b is numpy's argmin_j |w[j] - b|: the lowest index on ties, the first NaN if there is one.
 * The weights are bit-identical to the host routine's for every spectrum, alone or in any batch.
 * Limits per call: S <= 65535 and N[0] + ... + N[S-1] <= 2^26, else NMRFIT_E_UNSUPPORTED (the Python layer cuts longer
 * lists into calls); a null pointer, S <= 0, N[k] <= 0 or R[k] < 0 is NMRFIT_E_INVALID, reported before any device work.
 */
#ifndef NMRFIT_AMD_PREP_H
#define NMRFIT_AMD_PREP_H

#include "nmrfit_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* grid points a workgroup of the fill-and-smooth kernel owns (it stages ten more on each side) */
#define NMRFIT_WEIGHTS_TILE 1024

/* weights of S spectra into weights_out (sum N doubles); first_last_out: NULL or 2 * sum R int64 (the index pairs
 * first <= last of every region).  edges and level may be NULL when every R[k] is 0. */
int nmrfit_weights_build(int device, int32_t S, const int64_t *N, const double *w, const int32_t *R,
                         const double *edges /* 2 * sum R */, const double *level /* sum R */,
                         double *weights_out, int64_t *first_last_out);

/* nmrfit_batch_create_ragged with the weights plane built on the device instead of uploaded: the same arguments with
 * (R, edges, level) of the K fits in place of `weights`; R[k] = 0: unit weights.  The batch is then used and destroyed
 * through the nmrfit_batch_* calls of nmrfit_amd.h. */
int nmrfit_batch_create_regions(int device, int32_t K, const int64_t *N, const double *w, const double *u,
                                const double *v, const int32_t *R, const double *edges, const double *level,
                                const int32_t *P, const double *lower, const double *upper, const int64_t *swarmsize,
                                const nmrfit_pso_params *params, int variant, int fit_im, nmrfit_batch **out);

#ifdef __cplusplus
}
#endif
#endif /* NMRFIT_AMD_PREP_H */

/*
 * nmrfit_amd_noise.h -- noise replicas of spectra on the device (opt-in; found by symbol lookup like the other entry
 * points added within ABI 6: the version number does not change).  The product interface is nmrfit_amd.h.  Same
 * conventions as nmrfit_amd.h.
 *
 * The classic uncertainty estimate of a fitted number refits noisy copies of the data (the reference's helpers for it
 * are utils.sample_noise -- the sigma of a signal-free stretch -- and utils.rnd_data -- data + sigma * normal deviates)
 * and reads the spread of the results.  Here the copies are made on the device, from a generator that is a pure function
 * of (seed, grid point), so a replica can be reproduced anywhere -- in another batch, alone, or without this library.
 *
 * THE DEVIATES.  For a fit with the 64-bit noise seed s, grid point j (its index in GRID ORDER, j = 0 .. N-1):
 *   o = Philox4x32-10( counter = (j lo32, j hi32, 0x4E4F4953, 0), key = (s lo32, s hi32) )     four 32-bit words x y z w
 *       (Salmon et al., SC'11: multipliers 0xD2511F53 / 0xCD9E8D57, key increments 0x9E3779B9 / 0xBB67AE85, ten rounds;
 *        the generator of the swarm's uniforms, whose counter word 2 is a particle index below 2^28: the tag
 *        0x4E4F4953 there keeps the two streams apart even under the same key)
 *   ua = o.y << 32 | o.x          ub = o.w << 32 | o.z
 *   a  = ((ua >> 11) + 1) * 2^-53           in (0, 1]: the logarithm is finite
 *   b  =  (ub >> 11)      * 2^-53           in [0, 1)
 *   r  = sqrt(-2 log(a))
 *   t  = 6.283185307179586 * b              (the rounded fp64 product is the argument)
 *   z_u = r cos(t)        z_v = r sin(t)    (Box-Muller: two independent standard normal deviates)
 * and the replica is
 *   u'[j] = u[j] + sigma_u * z_u            v'[j] = v[j] + sigma_v * z_v
 * each a rounded multiply followed by a rounded add (no fused multiply-add), in fp64 throughout, with correctly
 * rounded sqrt and the device's fp64 log / sin / cos (within a few ulp of the exact functions: two implementations of
 * this definition agree to that, not bit for bit; the same library gives the same bits for the same (s, j), in any
 * batch, through either entry point below).
 * A fit with sigma_u == 0 && sigma_v == 0 is not touched at all: its values keep their bits, the sign of a zero
 * included.  NaN in u or v passes through.
 */
#ifndef NMRFIT_AMD_NOISE_H
#define NMRFIT_AMD_NOISE_H

#include "nmrfit_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* counter word 2 of the noise stream ("NOIS") */
#define NMRFIT_NOISE_TAG 0x4E4F4953u

/* Replicas of K spectra laid out one after the other as in nmrfit_batch_create_ragged: spectrum k has N[k] > 0 points
 * of u and v, sigmas sigma_u[k], sigma_v[k] >= 0 (finite) and the noise seed seed[k]; u_out, v_out: sum N doubles each.
 * Host pointers in both directions.  Limits per call: K <= 65535 and N[0] + ... + N[K-1] <= 2^26, else
 * NMRFIT_E_UNSUPPORTED (the Python layer cuts longer lists into calls); a null pointer, K <= 0, N[k] <= 0 or a sigma
 * that is negative, NaN or infinite is NMRFIT_E_INVALID, reported before any device work. */
int nmrfit_noise_replicas(int device, int32_t K, const int64_t *N, const double *u, const double *v,
                          const double *sigma_u, const double *sigma_v, const uint64_t *seed, double *u_out,
                          double *v_out);

/* The same, in place on the resident spectra of a created batch: fit k's u and v become the replica (sigma_u[k],
 * sigma_v[k], seed[k]) of what was uploaded; the padding of the device arrays stays zero.  Allowed ONCE and only before
 * the first generation: NMRFIT_E_STATE after nmrfit_batch_step / nmrfit_batch_run, while a reconstruction is in flight,
 * or when noise was added before.  The sigmas are checked as above.  Synchronous.  A call that fails on the device
 * (NMRFIT_E_HIP) leaves the spectra undefined and counts as the one call: destroy the batch. */
int nmrfit_batch_add_noise(nmrfit_batch *batch, const double *sigma_u, const double *sigma_v, const uint64_t *seed);

/* The spectrum fit k is fitting, in grid order (u_out, v_out: N[k] doubles each; either may be NULL): what was uploaded,
 * or its replica after nmrfit_batch_add_noise.  Any state; a k outside 0 .. K-1 is NMRFIT_E_INVALID. */
int nmrfit_batch_spectrum(nmrfit_batch *batch, int32_t k, double *u_out, double *v_out);

#ifdef __cplusplus
}
#endif
#endif /* NMRFIT_AMD_NOISE_H */

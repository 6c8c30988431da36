/*
 * nmrfit_amd_fid_cond.h -- raw FIDs to spectra with the conditioning that sits between "FID in memory" and the
 * transform: the removal of a Bruker group delay, a window (apodisation, first-point scaling), both on the device
 * (opt-in; found by symbol lookup like the other entry points added within ABI 6: the version number does not change).
 * Everything from the zero filling on is nmrfit_amd_fid.h, by the same kernels, unchanged.  Same conventions.
 *
 * The reference's Bruker branch (core.load) runs nmrglue's remove_digital_filter between the reader and the transform.
 * nmrglue is not a dependency and no parity with it is claimed: the definition below is modelled on its rm_dig_filter
 * (the shift, skip = floor(g + 2), add = max(skip - 6, 0), the post_proc ramp) and is normative ON ITS OWN;
 * nmrfit_amd.fid.condition_host restates it in numpy.  Only a group delay given as a number (GRPDLY) is taken; the
 * DSPFVS / DECIM table of old firmware is out of scope.
 *
 * JOB.  A job of nmrfit_fid_transform -- T >= 1 traces of n_in >= 1 complex points, a transform length n = 2^m -- plus
 * three optional things: a group delay g > 0 (a double, used as given) with a FORM, and a WINDOW.
 *
 * RAMP.  rho_n(i) = exp(+2 pi i g i / n), i = 0 .. n - 1.
 *
 * G, FORM 1 ("fid": what core.load does).  Per trace x of s = n_in points, s a power of two, 2 .. 2^22, s >= 2 skip:
 *     X = the forward unscaled transform of x, length s (no zero fill)
 *     B[k] = X[k] rho_s(k),  k = 0 .. s - 1 in natural order: one complex product (a c - b d, a d + b c), each rounded
 *     y = the inverse transform of B including the exact 1 / s: y[j] = fft(B)[(-j) mod s] / s -- the forward kernels
 *         only; the division is a scaling by a power of two
 *     skip = floor(g + 2),  add = max(skip - 6, 0)
 *     fold: y[j] <- y[j] + y[s - 1 - j] for 0 <= j < add (one rounded sum per part)
 *     the conditioned trace is y[0 .. s - skip - 1]:  n_in' = s - skip
 * A length s that is not a power of two is refused (NMRFIT_E_UNSUPPORTED): use form 2.
 *
 * G, FORM 2 ("spectrum": any n_in).  The trace is not conditioned, n_in' = n_in.  After the main transform of length
 * n every centred value is multiplied by the ramp, Y_t[i] <- Y_t[i] rho_n(i), i = 0 .. n - 1 the centred index (one
 * complex product as above), BEFORE the normaliser is sought.  This differs from an exact shift of the signed
 * frequency, exp(2 pi i g (i - n/2) / n), by the constant factor e^{-i pi g}, which a zero-order phase p0 absorbs.
 *
 * W, WINDOW.  n_in' doubles.  The trace as it enters the main transform is x'[j] = y[j] W[j] (y = x without form 1):
 * one rounded product per part, after form 1's fold and truncation.  First-point scaling is W[0] = 0.5.  Windows are
 * made on the host (no device exp or sin); a call uploads each of its M windows once and jobs name theirs by index, -1
 * for none.
 *
 * Then x'[j] = 0 for n_in' <= j < n, the transform, centring, reversal, (form 2's ramp,) normaliser, quotient, sum
 * over traces and the row: nmrfit_amd_fid.h.
 *
 * RAMP VALUES.  The rule of nmrfit_amd_fid.h's twiddles: every rho used is within mu = 2^-53, absolute and as a complex
 * number, of the exact one, and nothing is computed by the device's sin / cos.  Per distinct (g, n) of a call two
 * tables of at most 2048 double-double entries, rho_n(2048 h) and rho_n(l); their product is formed in double-double
 * arithmetic and rounded once (csrc/fid_twiddle.h's split product, the index split at 2^11).  The host fills them
 * (csrc/fid_ramp.h) with g i / n reduced mod 1 exactly, in integer arithmetic on g's bits -- g i needs up to 75 bits;
 * a floating-point product has lost about 2^-36 of a turn at n = 2^22 -- then folded to an octant, then cosl / sinl.
 *
 * ERROR BOUND, first order, per trace (u = 2^-53, eta of nmrfit_amd_fid.h, gamma_2 = 2u / (1 - 2u)).  A complex product
 * with a factor of modulus 1 known to mu has error at most kappa |a|, kappa = mu + sqrt(2) gamma_2 (Higham, Lemma 3.5).
 * Form 1: the first transform is off by log2(s) eta ||X||_2 (Thm 24.2), the product adds kappa ||X||_2, the second
 * transform carries both through (sqrt(s), undone by 1 / s) and adds log2(s) eta of its own: with ||y||_2 = ||x||_2 (the
 * ramp is unitary)   || y^ - y ||_2 <= (2 log2(s) eta + kappa) ||x||_2.  The fold adds two entries: the error's norm
 * grows by at most F = sqrt(2) (F = 1 when add = 0), as ||y||_2 does, and the sum is rounded (u).  The window scales
 * by at most max|W| and rounds once more (u):
 *     || x'^ - x' ||_2 <= (2 log2(s) eta + kappa + 2u) F max|W| ||x||_2
 * (without form 1: u max|W| ||x||_2 with a window, 0 without).  The main transform carries that to the spectrum times
 * sqrt(n) and adds log2(n) eta; form 2's product adds kappa:
 *     || Y^ - Y ||_2 <= ([the bracket above] + log2(n) eta [+ kappa]) sqrt(n) F max|W| ||x||_2
 *
 * PURITY.  As nmrfit_amd_fid.h: a spectrum's outputs are a pure function of its own traces, g, form and window.  No
 * atomics; no dependence on K, on the position in the batch, on which other jobs share a ramp or a window, or on what
 * device memory held before the call.
 *
 * LAUNCHES.  At most 16 per call whatever K: form 1's two transforms (3 each: short, pass 1, pass 2) with the ramp
 * stage between them, its store, the window-only multiply, the main transform (3), form 2's ramp, the three finishing
 * launches.  Every launch is a flat list of work items over the spectra; a job contributes no items to a stage it does
 * not need, and a launch without items is not made: a call with no form and no window makes the launches of
 * nmrfit_fid_transform and gives its bits.
 */
#ifndef NMRFIT_AMD_FID_COND_H
#define NMRFIT_AMD_FID_COND_H

#include "nmrfit_amd_fid.h"

#ifdef __cplusplus
extern "C" {
#endif

#define NMRFIT_FID_FORM_NONE 0
#define NMRFIT_FID_FORM_FID 1
#define NMRFIT_FID_FORM_SPECTRUM 2

/* n_in, n, T, fid, u_out, v_out, rows_out, transform_out: as nmrfit_fid_transform takes them.  form[k]: 0 none, 1 fid,
 * 2 spectrum; g[k]: the group delay (read where form[k] != 0); window_of[k]: -1, or the index of the job's window among
 * the M windows of the call; window_len[m] doubles each, one after the other in `windows` (M = 0: both may be null).
 * conditioned_out: NULL, or the traces as they enter the main transform: natural order, n_in' points each (interleaved),
 * trace after trace, spectrum after spectrum.  Host pointers both ways.  Synchronous.  At most 16 launches.
 * Every refusal comes before any device work, with a message naming the spectrum.  Those of nmrfit_fid_transform
 * apply, with n[k] >= n_in' in place of n[k] >= n_in[k].  NMRFIT_E_INVALID as well: a null form, g or window_of; M < 0, or
 * M > 0 with a null window_len or windows; a form outside 0 .. 2; g not finite or <= 0 where a form is set; form 1 with
 * s < 2 skip; window_of[k] outside -1 .. M - 1; window_len[m] != n_in' of a job that names it; a window value that is not
 * finite.  NMRFIT_E_UNSUPPORTED as well: form 1 with n_in not a power of two in 2 .. 2^22 (the message names form 2);
 * T n summed over the spectra, plus T n_in over the form-1 spectra, above 2^26. */
int nmrfit_fid_condition_transform(int device, int32_t K, const int64_t *n_in, const int64_t *n, const int32_t *T,
                                   const double *fid, const int32_t *form, const double *g, const int32_t *window_of,
                                   int32_t M, const int64_t *window_len, const double *windows, double *u_out,
                                   double *v_out, double *rows_out, double *transform_out, double *conditioned_out);

#ifdef __cplusplus
}
#endif
#endif /* NMRFIT_AMD_FID_COND_H */

/*
 * nmrfit_amd_fid_any.h -- raw FIDs to spectra at ANY transform length: a chirp-z (Bluestein) transform on the device for
 * lengths that are not powers of two (opt-in; found by symbol lookup like the other entry points added within ABI 6: the
 * version number does not change).  core.load transforms a FID at the length it has (ng.proc_base.fft pads nothing, the
 * ppm grid has u.size points); nmrfit_amd_fid.h and nmrfit_amd_fid_cond.h take powers of two only.  Everything here is
 * built on their transform and finishing kernels, unchanged.  Same conventions.
 *
 * JOB.  A job of nmrfit_fid_condition_transform.  Its transform length n = N is either a power of two, 2 .. 2^22 -- then
 * everything is nmrfit_amd_fid_cond.h, by the same launches, with the same bits -- or any other length, 3 .. 2^21 - 1.
 * The rest of this header is about the second kind.  n_in' <= N points x' enter the transform (after form 1 and the
 * window, if any).
 *
 * DEFINITION.  With contraction off, every product and sum rounded once:
 *     c[k] = exp(-i pi k^2 / N),  k = 0 .. N - 1                                    (the chirp: CHIRP VALUES)
 *     M = 2^m, the smallest power of two >= 2 N - 1                                  (M <= 2^22)
 *     a[k] = x'[k] c[k] for k < n_in', 0 for n_in' <= k < M: one complex product (a c - b d, a d + b c), each part rounded
 *     b[k] = conj(c[k]) for k < N;  b[M - k] = conj(c[k]) for 1 <= k < N;  0 elsewhere
 *     A = fft_M(a),  B = fft_M(b): the forward unscaled transform of nmrfit_amd_fid.h, length M
 *     P[q] = A[q] B[q],  q = 0 .. M - 1: one complex product as above
 *     p[j] = fft_M(P)[(-j) mod M] / M: the inverse by the forward kernels; the division is a scaling by a power of two
 *     X[q] = p[q] c[q],  q = 0 .. N - 1: one complex product as above
 * X is the transform of x' zero filled to N: k q = (k^2 + q^2 - (q - k)^2) / 2, so X[q] = c[q] sum_k a[k] b[q - k], and
 * the circular convolution of length M >= 2 N - 1 does not wrap for 0 <= q < N.
 *
 * CENTRING AND REVERSAL are numpy's fftshift for any N:
 *     Y[i] = X[(i + N - floor(N / 2)) mod N],  i = 0 .. N - 1        (N even: the turn is N / 2; N odd: (N + 1) / 2, so
 *                                                                      X[0] lands on i = floor(N / 2) either way)
 *     the device holds and returns Z[j] = Y[N - 1 - j], as nmrfit_amd_fid.h does: output j is X[(2 N - 1 - j - floor(N / 2)) mod N]
 * Then the normaliser, the quotient, the sum over traces and the row: nmrfit_amd_fid.h's finishing stage, unchanged.
 *
 * FORMS.  Form 1 ("fid") and windows compose with any n >= n_in': the Bruker path of core.load is s = 2^m, n = s - skip.
 * Form 2 ("spectrum") with a length that is not a power of two is refused (NMRFIT_E_UNSUPPORTED): its ramp tables are
 * split at 2^11 for n = 2^lg.
 *
 * CHIRP VALUES.  The rule of the twiddles and the ramp: every c[k] used is within mu = 2^-53, absolute and as a complex
 * number, of the exact one, and nothing is computed by the device's sin / cos.  k^2 is not additive in k, so no split
 * tables: the host fills one table of N complex doubles per distinct N of a call (csrc/fid_chirp.h).  The angle is
 * reduced exactly in integers, r = k^2 mod 2 N (k^2 < 2^42), the fraction of a turn is r / 2 N; it is folded to an octant,
 * so that 1, -i, sqrt(1/2) (1 - i) and their kin are exact where 8 r is a multiple of 2 N; cosl / sinl are taken on at most
 * pi / 4 and each part is rounded once.  tests/fid/chirp_check.hip measures the bound against 113 bits.
 *
 * SHARING.  B depends on N alone: it is made once per distinct N of a call, on the device, as an ordinary job (T = 1) of
 * the launches that transform the a's.  It is a pure function of N.
 *
 * ERROR BOUND, first order, per trace (u, eta, kappa = mu + sqrt(2) gamma_2 as in nmrfit_amd_fid_cond.h; Higham Thm 24.2
 * and Lemma 3.5).  eps = log2(M) eta.  beta = max_k |B[k]|, a property of the definition (||B||_2 = sqrt(M (2 N - 1)), so
 * beta >= sqrt(2 N - 1)).  ||a||_2 = ||x'||_2, ||A||_2 = sqrt(M) ||x'||_2, max|A| <= ||a||_1 <= sqrt(n_in') ||x'||_2,
 * ||b||_2 = sqrt(2 N - 1).
 *     || A^ - A ||_2 <= (eps + kappa) sqrt(M) ||x'||_2                      the product, carried by the transform, and its own
 *     || B^ - B ||_2 <= (eps + mu) sqrt(M) sqrt(2 N - 1)                    the chirp's mu, carried, and the transform's own
 *     || P^ - P ||_2 <= beta ||dA||_2 + max|A| ||dB||_2 + sqrt(2) gamma_2 beta sqrt(M) ||x'||_2
 *     the inverse divides by sqrt(M) (sqrt(M) of the transform, undone by 1 / M) and adds eps ||P||_2 / sqrt(M) <= eps beta ||x'||_2
 *     the last product adds kappa ||p||_2 <= kappa beta ||x'||_2
 * Together
 *     || Y^ - Y ||_2 <= ( beta (2 eps + 2 kappa + sqrt(2) gamma_2) + (eps + mu) sqrt(n_in' (2 N - 1)) ) ||x'||_2
 * An error of the conditioned trace (form 1, the window: nmrfit_amd_fid_cond.h's || x'^ - x' ||_2) passes through the
 * same linear map and is carried by beta: + beta || x'^ - x' ||_2.  The max|A| ||dB||_2 term takes every error of B to
 * meet the largest value of A: it is pessimistic by about sqrt(N).  The derivation uses n_in' only through
 * max|A| <= ||a||_1 <= sqrt(n_in') ||x'||_2: for a trace with s non-zero points ||a||_1 <= sqrt(s) ||x'||_2, so the bound
 * holds with s in place of n_in' (tests/fid_lengths_support.py: sparse_bar).
 *
 * PURITY.  As nmrfit_amd_fid_cond.h: no atomics; no dependence on K, on the position in the batch, on which other jobs
 * share an N, a ramp or a window, or on what device memory held before the call.
 *
 * BUDGET.  The values of a call are
 *     sum_k T n  +  sum over form 1 of T n_in  +  sum over the jobs whose n is no power of two of 2 T M  +  sum over the
 *     distinct such n of 2 M
 * (a and P share one plane of T M values, A and fft(P) another; b and B are one plane of M each) and must stay within
 * 2^26.  As before, the planes between the two passes of the long transforms are not counted.
 *
 * LAUNCHES.  At most 27 per call whatever K: nmrfit_fid_condition_transform's 16, a fourth finishing launch (the partial
 * maxima of the rows whose n is no power of two: the point within a trace is a remainder there, not a mask) and ten of the
 * chirp path: (a), (b), the transforms of a and b (3), (c), the transform of P (3), (d).  A window without form 1 is
 * nmrfit_fid_condition_transform's window launch, before (a).  Every launch is a flat list of work items; a launch without
 * items is not made: a call whose lengths are all powers of two makes nmrfit_fid_condition_transform's launches and gives
 * its bits.
 */
#ifndef NMRFIT_AMD_FID_ANY_H
#define NMRFIT_AMD_FID_ANY_H

#include "nmrfit_amd_fid_cond.h"

#ifdef __cplusplus
extern "C" {
#endif

#define NMRFIT_FID_ANY_MIN 3
#define NMRFIT_FID_ANY_MAX 2097151 /* 2^21 - 1 */

/* Every argument as nmrfit_fid_condition_transform takes it; n[k] is a power of two in 2 .. 2^22 or any other length in
 * 3 .. 2^21 - 1.  Host pointers both ways.  Synchronous.  At most 27 launches.  Every refusal comes before any device
 * work, with a message naming the spectrum.  Those of nmrfit_fid_condition_transform apply, except that a length that is
 * no power of two is taken.  NMRFIT_E_UNSUPPORTED as well: n[k] = 1, a power of two above 2^22, or any other length above
 * 2^21 - 1; form 2 with a length that is no power of two (the message says "form 2"); the values of BUDGET above 2^26. */
int nmrfit_fid_transform_any(int device, int32_t K, const int64_t *n_in, const int64_t *n, const int32_t *T, const double *fid,
                             const int32_t *form, const double *g, const int32_t *window_of, int32_t M,
                             const int64_t *window_len, const double *windows, double *u_out, double *v_out,
                             double *rows_out, double *transform_out, double *conditioned_out);

#ifdef __cplusplus
}
#endif
#endif /* NMRFIT_AMD_FID_ANY_H */

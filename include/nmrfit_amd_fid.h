/*
 * nmrfit_amd_fid.h -- raw FIDs to spectra on the device: a batched fp64 Fourier transform with zero filling, the
 * centring and reversal of the reference's loader, its normalisation and its sum over traces (opt-in; found by symbol
 * lookup like the other entry points added within ABI 6: the version number does not change).  The product interface
 * is nmrfit_amd.h.  Same conventions as nmrfit_amd.h.
 *
 * The reference makes a spectrum in core.load, between the instrument file and containers.Data:
 *     data = fftshift(fft(data, axis=-1))       nmrglue's proc_base.fft
 *     data = data / np.max(data)                complex max (lexicographic), complex division
 *     u = data.real.sum(axis=0);  v = data.imag.sum(axis=0);  Data(w[::-1], u[::-1], v[::-1])
 * The file readers stay out of scope; the arithmetic from "complex FID in memory" to (u, v) is this header.
 *
 * JOB.  A job is one spectrum k: T >= 1 traces of n_in >= 1 complex points each (re, im interleaved), and a transform
 * length n = 2^m >= n_in, 1 <= m <= 22.  x_t[j] = 0 for n_in <= j < n (zero filling, done on the device: only n_in
 * points per trace are uploaded).
 *
 * TRANSFORM.  X_t[q] = sum_j x_t[j] exp(-2 pi i j q / n), q = 0 .. n-1: forward, unscaled.  Radix-4 Stockham stages (one
 * radix-2 stage first when m is odd) on an LDS-resident block of 4096 points; n <= 4096 is one such block, a longer
 * transform is n = n1 n2 (n1 = 2^floor(m/2), n2 = n / n1) in two passes through device memory: n2 column transforms of
 * length n1, each result times omega_n^(j2 q1), then n1 row transforms of length n2.  A complex product is
 * (a c - b d, a d + b c), four products and two sums, each rounded once; there is no fused multiply-add in the
 * butterflies.
 *
 * TWIDDLES.  Every twiddle omega is within mu = 2^-53 (one unit roundoff u, absolute, as a complex number) of the
 * exact root of unity.  The stage twiddles omega_4096^k are cos and sin evaluated in 64-bit long double on the host and
 * rounded once to fp64 (each part within 2^-54, the pair within sqrt(2) 2^-54 = 0.71 u).  The twiddle between the two
 * passes, omega_{2^22}^T, is the product of two table entries held as double-double values, formed in double-double
 * arithmetic and rounded once: the same bound.  Nothing is computed by the device's sin / cos.  With mu <= u the
 * first-order error bound of the transform (Higham, Accuracy and Stability of Numerical Algorithms, Thm 24.2) is
 *     || X^ - X ||_2 <= log2(n) eta || X ||_2,   eta = mu + gamma_4 (sqrt(2) + mu)  <  8 u       (u = 2^-53)
 *
 * PURITY.  The arithmetic of a trace is a pure function of (n_in, n, x_t): no atomics, no dependence on K, on the
 * trace's position in the batch, on T, or on what device memory held before the call.  u, v and the row of a spectrum
 * are a pure function of its traces.
 *
 * CENTRE AND REVERSE.  Y_t[i] = X_t[(i + n/2) mod n] (fftshift); the output index is j = n - 1 - i (the [::-1] of
 * core.load).  Both are index arithmetic in the last pass's store: the device holds Z_t[j] = Y_t[n - 1 - j].
 *
 * NORMALISER.  m = Y_t*[i*], the lexicographic maximum over all T n values of Y: the largest real part, ties by the
 * larger imaginary part, then the smallest flat index t n + i (np.max of a complex array; -0.0 == +0.0).
 *
 * QUOTIENT.  (a + i b) / m by Smith's rule, every operation rounded once, no fused multiply-add (mr = Re m, mi = Im m):
 *   |mr| >= |mi|:   rat = mi / mr;  scl = 1 / (mr + mi * rat);  q_re = (a + b * rat) * scl;  q_im = (b - a * rat) * scl
 *   otherwise:      rat = mr / mi;  scl = 1 / (mi + mr * rat);  q_re = (a * rat + b) * scl;  q_im = (b * rat - a) * scl
 *
 * OUTPUTS.  u[j] = sum_t q_re, v[j] = sum_t q_im of Z_t[j] / m: a running sum over t = 0 .. T-1 ascending that starts
 * from +0.0, as np.sum(axis=0) does.  For T = 1 that is the value itself, except that -0.0 comes out as +0.0 (the
 * imaginary part of m / m is often -0.0: the reference returns +0.0 there, and so does this).
 *
 * ROW.  NMRFIT_FID_ROW doubles per spectrum:
 *   0 status   1 Re m   2 Im m   3 the flat index t* n + i* of m (in Y's order)   4 n   5 T
 * status 0: transformed.  status 1: m == 0 (an all-zero FID); u and v are NaN, entries 1 .. 3 are as found.  status 2:
 * some value of the transform is not finite; u, v and entries 1 .. 3 are NaN.
 */
#ifndef NMRFIT_AMD_FID_H
#define NMRFIT_AMD_FID_H

#include "nmrfit_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* doubles per row */
#define NMRFIT_FID_ROW 6
/* log2 of the longest transform */
#define NMRFIT_FID_MAX_LOG2 22
/* log2 of the longest transform that is one LDS-resident block: 4096 points of 16 bytes are 64 KiB, two workgroups per
 * CU's 160 KiB */
#define NMRFIT_FID_LDS_LOG2 12

/* The spectra of K jobs from host arrays.  n_in[k], n[k], T[k] per spectrum; fid: the traces one after the other,
 * spectrum after spectrum, 2 n_in[k] doubles per trace.  u_out, v_out: n[0] + ... + n[K-1] doubles each, spectrum after
 * spectrum, in the output order j; rows_out: K rows; transform_out: NULL, or 2 (T[0] n[0] + ... ) doubles: Z, interleaved,
 * trace after trace -- Y in the output order j, the input of the finishing stage (Y_t[i] is entry n - 1 - i of trace
 * t).  Host pointers both ways.  Synchronous.  The number of kernel launches of a call is at most 6 whatever K and T.
 * NMRFIT_E_INVALID, reported before any device work: a null pointer (transform_out may be null), K <= 0, T[k] <= 0,
 * n_in[k] <= 0, n[k] < n_in[k].  NMRFIT_E_UNSUPPORTED: an n[k] that is not a power of two or outside 2 .. 2^22 (zero
 * fill to the next power of two: other lengths are refused, not emulated), K > 65535, T[0] n[0] + ... > 2^26. */
int nmrfit_fid_transform(int device, int32_t K, const int64_t *n_in, const int64_t *n, const int32_t *T,
                         const double *fid, double *u_out, double *v_out, double *rows_out, double *transform_out);

#ifdef __cplusplus
}
#endif
#endif /* NMRFIT_AMD_FID_H */

// fid_chirp.h -- where the chirp values of fid_any.hip come from (include/nmrfit_amd_fid_any.h, CHIRP VALUES).  Host code;
// tests/fid/chirp_check.hip compiles it and measures the bound the header states.
//   c[k] = exp(-i pi k^2 / N), k = 0 .. N - 1, N any length up to 2^21.  k^2 is not additive in k, so the hi * lo split
//   tables of fid_twiddle.h do not apply: one table of N values per distinct N of a call, each part rounded once from
//   long double.
//   THE ANGLE.  pi k^2 / N = 2 pi r / (2 N) with r = k^2 mod 2 N, exact in uint64_t (k^2 < 2^42).  4 r / N is the place in
//   eighths of a turn: its integer part is the octant, the rest (an integer below N, over N) folds into [0, 1/8] of a turn
//   as fid_unit_root folds, so that 1, -i, sqrt(1/2) (1 - i) and their kin are exact where 8 r is a multiple of 2 N and
//   every argument of cosl / sinl is at most pi / 4.
#pragma once
#include "fid_twiddle.h"

namespace nmrfit {

// cos and sin of -pi k^2 / N in long double; 0 <= k < 2^21, 1 <= N <= 2^21
inline void fid_chirp_root(int64_t k, int64_t N, long double *c, long double *s)
{
    const long double pi = 3.14159265358979323846264338327950288L;
    const uint64_t two_n = 2 * (uint64_t)N, r = ((uint64_t)k * (uint64_t)k) % two_n;
    const uint64_t eighths = 4 * r;                       // 4 r / N = oct + rem / N   (< 2^25)
    const int oct = (int)(eighths / (uint64_t)N);
    const uint64_t rem = eighths - (uint64_t)oct * (uint64_t)N;
    const bool odd = oct & 1;
    long double cc, ss;
    if (rem == 0) {                                       // a multiple of an eighth of a turn
        cc = odd ? 0.70710678118654752440084436210484904L : 1.0L;
        ss = odd ? 0.70710678118654752440084436210484904L : 0.0L;
    } else {
        const uint64_t rr = odd ? (uint64_t)N - rem : rem;
        const long double th = (long double)rr / (long double)N * (pi / 4.0L);
        cc = cosl(th);
        ss = sinl(th);
        if (odd) {
            const long double t = cc;
            cc = ss;
            ss = t;
        }
    }      // cos, sin of the angle within its quarter: (q pi/2 + a), a in [0, pi/2)
    long double C, S;
    switch (oct >> 1) {
    case 0: C = cc; S = ss; break;
    case 1: C = -ss; S = cc; break;
    case 2: C = -cc; S = -ss; break;
    default: C = ss; S = -cc; break;
    }
    *c = C;
    *s = -S;      // the negative angle
}

// c[0 .. N - 1], each part rounded once to fp64
inline void fid_fill_chirp_table(int64_t N, FidTw *c)
{
    for (int64_t k = 0; k < N; ++k) {
        long double re, im;
        fid_chirp_root(k, N, &re, &im);
        c[k].re = (double)re;
        c[k].im = (double)im;
    }
}

// M = 2^m, the smallest power of two >= 2 N - 1
inline int fid_chirp_log2(int64_t N)
{
    int m = 0;
    while (((int64_t)1 << m) < 2 * N - 1) ++m;
    return m;
}

}  // namespace nmrfit

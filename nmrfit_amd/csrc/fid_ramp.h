// fid_ramp.h -- where the ramp values of fid_cond.hip come from (include/nmrfit_amd_fid_cond.h, RAMP VALUES).  Host and
// device code; tests/fid/ramp_check.hip compiles it for the host and measures the bound the header states.
//   rho_n(i) = exp(+2 pi i g i / n), i = 0 .. n - 1, n = 2^lg, g a double as given (not a multiple of anything).
//   Per (g, n) two tables of double-double entries, as fid_twiddle.h's split tables are: hi[h] = rho_n(2048 h), h <
//   ceil(n / 2048), and lo[l] = rho_n(l), l < min(n, 2048).  rho_n(i) = hi[i >> 11] * lo[i & 2047] by fid_split_twiddle:
//   the product in double-double arithmetic, rounded once.
//   THE ANGLE.  g i / n is reduced mod 1 EXACTLY before cosl / sinl: g = m 2^e with m an integer below 2^53, so
//   g i / n = (m i) 2^(e - lg) with m i < 2^75 an exact integer in unsigned __int128; the fraction is its low (lg - e)
//   bits.  (A floating-point product g * i has lost 2^-36 of a turn at n = 2^22 before any reduction.)  The fraction's
//   top three bits are the octant, the rest folds into [0, 1/8] of a turn as fid_unit_root folds, so that the exact
//   values 0, +-1, +-sqrt(1/2) are exact and every argument of cosl / sinl is at most pi / 4.
#pragma once
#include "fid_twiddle.h"

namespace nmrfit {

// how many entries the two tables of a ramp over n = 2^lg points have
inline int fid_ramp_hi_count(int lg) { return lg <= kFidLgSplit ? 1 : 1 << (lg - kFidLgSplit); }
inline int fid_ramp_lo_count(int lg) { return lg <= kFidLgSplit ? 1 << lg : kFidSplit; }

// rho_n(i) of the device (and of the host check): i < n
NMRFIT_FID_HD FidTw fid_ramp_value(const FidTwDD *__restrict__ hi, const FidTwDD *__restrict__ lo, int i)
{
    return fid_split_twiddle(hi, lo, i);
}

// (host code from here on)
// cos and sin of +2 pi g i / 2^lg in long double; g finite and > 0, 0 <= i < 2^22, 0 <= lg <= 22
inline void fid_ramp_root(double g, int64_t i, int lg, long double *c, long double *s)
{
    const long double pi = 3.14159265358979323846264338327950288L;
    int ex = 0;
    const double fr = frexp(g, &ex);                        // g = fr 2^ex, 0.5 <= fr < 1
    const uint64_t m = (uint64_t)ldexp(fr, 53);             // (exact: 53 bits)
    const unsigned __int128 P = (unsigned __int128)m * (unsigned __int128)(uint64_t)i;   // < 2^75
    const int k = lg + 53 - ex;                             // g i / n = P 2^-k
    // the fraction of a turn as oct / 8 + rem 2^-kk, 0 <= rem < 2^(kk - 3)
    int oct;
    long double part;                                       // rem / 2^(kk - 3): the place within the octant, in [0, 1)
    bool zero;                                              // rem == 0
    if (k <= 0) {                                           // an integer number of turns
        oct = 0;
        part = 0.0L;
        zero = true;
    } else if (k > 120) {                                   // P 2^-k < 2^-45: in the first octant, no bits to cut
        oct = 0;
        part = ldexpl((long double)P, 3 - k);
        zero = P == 0;
    } else {
        unsigned __int128 r = P & ((((unsigned __int128)1) << k) - 1);
        int kk = k;
        if (kk < 3) {
            r <<= 3 - kk;
            kk = 3;
        }
        oct = (int)(r >> (kk - 3));
        const unsigned __int128 rem = r & ((((unsigned __int128)1) << (kk - 3)) - 1);
        zero = rem == 0;
        part = ldexpl((long double)rem, -(kk - 3));         // (rounded to 64 bits: relative 2^-64 of at most pi / 4)
    }
    const bool odd = oct & 1;
    long double cc, ss;
    if (zero) {                                             // a multiple of an eighth of a turn
        cc = odd ? 0.70710678118654752440084436210484904L : 1.0L;
        ss = odd ? 0.70710678118654752440084436210484904L : 0.0L;
    } else {
        const long double th = (odd ? 1.0L - part : part) * (pi / 4.0L);
        cc = cosl(th);
        ss = sinl(th);
        if (odd) {
            const long double t = cc;
            cc = ss;
            ss = t;
        }
    }      // cos, sin of the angle within its quarter: (q pi/2 + a), a in [0, pi/2)
    switch (oct >> 1) {
    case 0: *c = cc; *s = ss; break;
    case 1: *c = -ss; *s = cc; break;
    case 2: *c = -cc; *s = -ss; break;
    default: *c = ss; *s = -cc; break;
    }
}

inline void fid_fill_ramp_tables(double g, int lg, FidTwDD *hi, FidTwDD *lo)
{
    const auto put = [](FidTwDD *e, long double c, long double s) {
        e->ch = (double)c;
        e->cl = (double)(c - (long double)e->ch);
        e->sh = (double)s;
        e->sl = (double)(s - (long double)e->sh);
    };
    long double c, s;
    for (int h = 0; h < fid_ramp_hi_count(lg); ++h) {
        fid_ramp_root(g, (int64_t)h << kFidLgSplit, lg, &c, &s);
        put(hi + h, c, s);
    }
    for (int l = 0; l < fid_ramp_lo_count(lg); ++l) {
        fid_ramp_root(g, l, lg, &c, &s);
        put(lo + l, c, s);
    }
}

}  // namespace nmrfit

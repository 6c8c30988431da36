// fid_twiddle.h -- where the twiddles of fid.hip come from (include/nmrfit_amd_fid.h, TWIDDLES).  Host and device code;
// tests/fid/twiddle_check.hip compiles it for the host and measures the bound the header states.
//   stage table   omega_4096^k, k = 0 .. 4095: cos and sin in long double on the host, each rounded once to fp64.  A
//                 stage of an LDS-resident transform reads its twiddles from it, no product is formed.
//   split table   omega_{2^22}^T for the twiddle between the two passes of a long transform: T = 2048 hi + lo, one table of
//                 2048 entries each for hi and lo, every cos and sin held as an unevaluated sum of two doubles (the
//                 long double value, 64 bits).  The product of the two entries is formed in double-double arithmetic
//                 and rounded to fp64 at the end: as good as a directly rounded value, at 2 x 64 KiB of tables.
#pragma once
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define NMRFIT_FID_HD __host__ __device__ __forceinline__
#else
#define NMRFIT_FID_HD inline
#endif

namespace nmrfit {

constexpr int kFidLgStage = 12, kFidStage = 1 << kFidLgStage;   // the stage table's length: the LDS-resident capacity
constexpr int kFidLgMax = 22;                                   // the longest transform, 2^22
constexpr int kFidLgSplit = 11, kFidSplit = 1 << kFidLgSplit;   // the split tables' length (22 = 11 + 11)

struct FidTw {        // one stage twiddle
    double re, im;
};
struct FidTwDD {      // one split-table entry: cos = ch + cl, sin = sh + sl (of the NEGATIVE angle: forward transform)
    double ch, cl, sh, sl;
};

#pragma clang fp contract(off)   // (the error-free transformations below name their fused operations themselves)

// a c - b d with every operand a double-double, rounded once (to within 2^-100) at the end
NMRFIT_FID_HD double fid_dd_diff(double ah, double al, double ch, double cl, double bh, double bl, double dh, double dl)
{
    const double p = ah * ch, ep = fma(ah, ch, -p);
    const double q = bh * dh, eq = fma(bh, dh, -q);
    const double s = p - q, bb = s - p;
    const double es = (p - (s - bb)) + (-q - bb);   // two_sum(p, -q)
    const double lo = ((ah * cl + al * ch) - (bh * dl + bl * dh)) + (ep - eq);
    return s + (es + lo);
}

// omega_{2^22}^T = hi[T >> 11] * lo[T & 2047], T = 0 .. 2^22 - 1
NMRFIT_FID_HD FidTw fid_split_twiddle(const FidTwDD *__restrict__ hi, const FidTwDD *__restrict__ lo, int T)
{
    const FidTwDD a = hi[T >> kFidLgSplit], b = lo[T & (kFidSplit - 1)];
    FidTw w;
    w.re = fid_dd_diff(a.ch, a.cl, b.ch, b.cl, a.sh, a.sl, b.sh, b.sl);        // cos cos - sin sin
    w.im = fid_dd_diff(a.ch, a.cl, b.sh, b.sl, -a.sh, -a.sl, b.ch, b.cl);      // cos sin + sin cos
    return w;
}

// (host code from here on)
// cos and sin of -2 pi k / 2^lg in long double, by octant so that the exact values (0, +-1, +-sqrt(1/2)) are exact
inline void fid_unit_root(int64_t k, int lg, long double *c, long double *s)
{
    const long double pi = 3.14159265358979323846264338327950288L;
    const int64_t n = (int64_t)1 << lg, m = k & (n - 1);
    if (lg < 3) {      // n = 1, 2, 4: the roots are 1, -i, -1, i
        const int quarter = (int)(m * 4 / n);
        const long double cs[4] = {1.0L, 0.0L, -1.0L, 0.0L}, sn[4] = {0.0L, -1.0L, 0.0L, 1.0L};
        *c = cs[quarter];
        *s = sn[quarter];
        return;
    }
    const int64_t eighth = n >> 3;
    const int oct = (int)(m / eighth);
    const int64_t r = m - oct * eighth;      // the angle is (oct + r / eighth) pi / 4
    // fold into [0, pi/4]
    const bool odd = oct & 1;
    const int64_t rr = odd ? eighth - r : r;
    const long double th = (long double)rr / (long double)eighth * (pi / 4.0L);
    long double cc = cosl(th), ss = sinl(th);
    if (rr == eighth) cc = ss = 0.70710678118654752440084436210484904L;
    if (odd) {
        const long double t = cc;
        cc = ss;
        ss = t;
    }      // cos, sin of the angle within its quarter: (q pi/2 + a), a in [0, pi/2)
    const int quarter = oct >> 1;
    long double C, S;
    switch (quarter) {
    case 0: C = cc; S = ss; break;
    case 1: C = -ss; S = cc; break;
    case 2: C = -cc; S = -ss; break;
    default: C = ss; S = -cc; break;
    }
    *c = C;
    *s = -S;      // the negative angle
}

inline void fid_fill_stage_table(FidTw *tw)
{
    for (int k = 0; k < kFidStage; ++k) {
        long double c, s;
        fid_unit_root(k, kFidLgStage, &c, &s);
        tw[k].re = (double)c;
        tw[k].im = (double)s;
    }
}

inline void fid_fill_split_tables(FidTwDD *hi, FidTwDD *lo)
{
    for (int k = 0; k < kFidSplit; ++k) {
        long double c, s;
        fid_unit_root((int64_t)k << kFidLgSplit, kFidLgMax, &c, &s);
        hi[k].ch = (double)c;
        hi[k].cl = (double)(c - (long double)hi[k].ch);
        hi[k].sh = (double)s;
        hi[k].sl = (double)(s - (long double)hi[k].sh);
        fid_unit_root(k, kFidLgMax, &c, &s);
        lo[k].ch = (double)c;
        lo[k].cl = (double)(c - (long double)lo[k].ch);
        lo[k].sh = (double)s;
        lo[k].sl = (double)(s - (long double)lo[k].sh);
    }
}

}  // namespace nmrfit

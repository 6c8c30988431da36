// ramp_check.hip -- compiled for the HOST by tests/test_fid_cond_cpu.py: the ramp values of csrc/fid_ramp.h (the table
// filler and the double-double split product, as the kernels of fid_cond.hip form them) against a truth of 113 bits.
// For g in {0.3, 5.0, 67.9, 68.0, 67.98416137695312} and n in {2, 256, 2^13, 2^22} it prints one line "g n worst", the
// worst |rho^ - rho| in units of u = 2^-53 over every index up to n = 2^13, and over a stride plus 10^6 pseudo-random
// indices at 2^22.  With the argument "naive" the tables are filled from the angle reduced in fp64 instead
// (fmod(g * i / n, 1)): what the exact reduction is there to avoid.
// THE TRUTH.  g i / n mod 1 as an exact integer over 2^k (unsigned __int128), brought to [-1/8, 1/8] of a turn around the
// nearest quarter in integers, then cos and sin by their Taylor series in __float128 (113 bits; |theta| <= pi / 4, 16
// terms), pi as the sum of three doubles (161 bits).  Nothing of fid_ramp.h's reduction is reused.
#include "fid_ramp.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

using namespace nmrfit;
typedef __float128 quad;

static void truth(double g, int64_t i, int lg, quad *c, quad *s)
{
    int ex = 0;
    const double fr = frexp(g, &ex);
    const uint64_t m = (uint64_t)ldexp(fr, 53);
    const unsigned __int128 P = (unsigned __int128)m * (unsigned __int128)(uint64_t)i;
    int k = lg + 53 - ex;   // g i / n = P / 2^k
    if (k < 2 || k > 120) exit(4);
    const unsigned __int128 one = (unsigned __int128)1 << k, r = P & (one - 1);
    // the nearest quarter turn q, and the signed rest d / 2^k in [-1/8, 1/8]
    const unsigned __int128 quarter = one >> 2;
    const int q = (int)((r + (quarter >> 1)) / quarter);
    const unsigned __int128 centre = (unsigned __int128)q * quarter;
    const bool neg = r < centre;
    const unsigned __int128 d = neg ? centre - r : r - centre;
    static quad scale[128], inv_c[17], inv_s[17];   // 2^-k; 1 / ((2j - 1) 2j) and 1 / (2j (2j + 1))
    if (scale[0] == 0) {
        scale[0] = 1.0;
        for (int b = 1; b < 128; ++b) scale[b] = scale[b - 1] * (quad)0.5;
        for (int j = 1; j <= 16; ++j) {
            inv_c[j] = (quad)1.0 / (quad)((2 * j - 1) * (2 * j));
            inv_s[j] = (quad)1.0 / (quad)((2 * j) * (2 * j + 1));
        }
    }
    const quad f = (quad)d * scale[k];
    const quad pi = (quad)3.141592653589793116e+00 + (quad)1.224646799147353207e-16 + (quad)-2.994769809718339666e-33;
    const quad th = (neg ? -f : f) * ((quad)2.0 * pi), t2 = th * th;
    quad cs = 1.0, sn = th, term_c = 1.0, term_s = th;
    for (int j = 1; j <= 16; ++j) {   // (pi/4)^32 / 32! < 2^-120
        term_c = -term_c * t2 * inv_c[j];
        term_s = -term_s * t2 * inv_s[j];
        cs += term_c;
        sn += term_s;
    }
    switch (q & 3) {
    case 0: *c = cs; *s = sn; break;
    case 1: *c = -sn; *s = cs; break;
    case 2: *c = -cs; *s = -sn; break;
    default: *c = sn; *s = -cs; break;
    }
}

static void fill_naive(double g, int lg, FidTwDD *hi, FidTwDD *lo)
{
    const double n = (double)((int64_t)1 << lg);
    const long double two_pi = 6.28318530717958647692528676655900577L;
    const auto put = [&](FidTwDD *e, int64_t i) {
        const long double th = two_pi * (long double)fmod(g * (double)i / n, 1.0);
        const long double c = cosl(th), s = sinl(th);
        e->ch = (double)c;
        e->cl = (double)(c - (long double)e->ch);
        e->sh = (double)s;
        e->sl = (double)(s - (long double)e->sh);
    };
    for (int h = 0; h < fid_ramp_hi_count(lg); ++h) put(hi + h, (int64_t)h << kFidLgSplit);
    for (int l = 0; l < fid_ramp_lo_count(lg); ++l) put(lo + l, l);
}

int main(int argc, char **argv)
{
    const bool naive = argc > 1 && !strcmp(argv[1], "naive");
    const double gs[5] = {0.3, 5.0, 67.9, 68.0, 67.98416137695312};
    const int lgs[4] = {1, 8, 13, 22};
    const quad u = (quad)1.0 / (quad)9007199254740992.0;
    std::vector<FidTwDD> hi(kFidSplit), lo(kFidSplit);
    for (double g : gs)
        for (int lg : lgs) {
            if (naive) fill_naive(g, lg, hi.data(), lo.data());
            else fid_fill_ramp_tables(g, lg, hi.data(), lo.data());
            const int64_t n = (int64_t)1 << lg;
            quad worst2 = 0.0;
            const auto look = [&](int64_t i) {
                const FidTw w = fid_ramp_value(hi.data(), lo.data(), (int)i);
                quad c, s;
                truth(g, i, lg, &c, &s);
                const quad dr = (quad)w.re - c, di = (quad)w.im - s, e2 = dr * dr + di * di;
                if (e2 > worst2) worst2 = e2;
            };
            if (lg <= 13) {
                for (int64_t i = 0; i < n; ++i) look(i);
            } else {
                for (int64_t i = 0; i < n; i += 61) look(i);
                look(n - 1);
                uint64_t state = 88172645463325252ull;
                for (int r = 0; r < (naive ? 0 : 1000000); ++r) {   // (the stride alone shows the naive filler's loss)
                    state ^= state << 13;
                    state ^= state >> 7;
                    state ^= state << 17;
                    look((int64_t)(state & (uint64_t)(n - 1)));
                }
            }
            printf("%.17g %lld %.6Lf\n", g, (long long)n, sqrtl((long double)(worst2 / (u * u))));
        }
    // rho(0) = 1 exactly, and an integer g at a quarter of n gives the exact roots
    fid_fill_ramp_tables(5.0, 13, hi.data(), lo.data());
    const FidTw a = fid_ramp_value(hi.data(), lo.data(), 0), b = fid_ramp_value(hi.data(), lo.data(), 1 << 11);
    if (a.re != 1.0 || a.im != 0.0 || b.re != 0.0 || b.im != 1.0) return 2;   // exp(2 pi i 5 / 4) = i
    return 0;
}

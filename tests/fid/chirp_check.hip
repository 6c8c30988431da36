// chirp_check.hip -- compiled for the HOST by tests/test_fid_any_cpu.py: the chirp values of csrc/fid_chirp.h (the table
// fid_any.hip uploads) against a truth of 113 bits.  For N in {3, 7, 12, 1000, 4027, 4099, 65466, 2^21 - 1} it prints one
// line "N worst", the worst |c^ - c| in units of u = 2^-53 over every index up to N = 2^13, and over a stride plus 10^6
// pseudo-random indices beyond.  With the argument "naive" the table is filled from the angle formed in fp64 instead
// (pi * k * k / N): what the exact reduction is there to avoid.
// THE TRUTH.  k^2 mod 2 N in unsigned __int128, brought to [-1/8, 1/8] of a turn around the nearest quarter in integers,
// then cos and sin by their Taylor series in __float128 (113 bits; |theta| <= pi / 4, 16 terms), pi as the sum of three
// doubles (161 bits).  Nothing of fid_chirp.h's reduction is reused.
#include "fid_chirp.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

using namespace nmrfit;
typedef __float128 quad;

// cos and sin of -pi k^2 / N
static void truth(int64_t k, int64_t N, quad *c, quad *s)
{
    const unsigned __int128 turn = 2 * (unsigned __int128)N, r = ((unsigned __int128)k * (unsigned __int128)k) % turn;
    // the fraction of a turn is r / 2 N = 2 r / 4 N: the nearest quarter q, and the signed rest d / 4 N in [-1/8, 1/8]
    const int64_t two_r = (int64_t)(2 * r), q = (two_r + N / 2) / N, d = two_r - q * N;
    if (2 * (d < 0 ? -d : d) > N) exit(4);
    static quad inv_c[17], inv_s[17];   // 1 / ((2j - 1) 2j) and 1 / (2j (2j + 1))
    if (inv_c[1] == 0)
        for (int j = 1; j <= 16; ++j) {
            inv_c[j] = (quad)1.0 / (quad)((2 * j - 1) * (2 * j));
            inv_s[j] = (quad)1.0 / (quad)((2 * j) * (2 * j + 1));
        }
    const quad pi = (quad)3.141592653589793116e+00 + (quad)1.224646799147353207e-16 + (quad)-2.994769809718339666e-33;
    const quad th = (quad)d / (quad)(4 * N) * ((quad)2.0 * pi), t2 = th * th;
    quad cs = 1.0, sn = th, term_c = 1.0, term_s = th;
    for (int j = 1; j <= 16; ++j) {   // (pi/4)^32 / 32! < 2^-120
        term_c = -term_c * t2 * inv_c[j];
        term_s = -term_s * t2 * inv_s[j];
        cs += term_c;
        sn += term_s;
    }
    quad C, S;   // of the positive angle
    switch (q & 3) {
    case 0: C = cs; S = sn; break;
    case 1: C = -sn; S = cs; break;
    case 2: C = -cs; S = -sn; break;
    default: C = sn; S = -cs; break;
    }
    *c = C;
    *s = -S;
}

static void fill_naive(int64_t N, FidTw *c)
{
    const double pi = 3.14159265358979323846;
    for (int64_t k = 0; k < N; ++k) {
        const double th = pi * (double)k * (double)k / (double)N;
        c[k].re = (double)cosl((long double)th);
        c[k].im = (double)-sinl((long double)th);
    }
}

int main(int argc, char **argv)
{
    const bool naive = argc > 1 && !strcmp(argv[1], "naive");
    const int64_t lengths[8] = {3, 7, 12, 1000, 4027, 4099, 65466, ((int64_t)1 << 21) - 1};
    const quad u = (quad)1.0 / (quad)9007199254740992.0;
    for (int64_t N : lengths) {
        std::vector<FidTw> c((size_t)N);
        if (naive) fill_naive(N, c.data());
        else fid_fill_chirp_table(N, c.data());
        quad worst2 = 0.0;
        const auto look = [&](int64_t k) {
            quad cr, ci;
            truth(k, N, &cr, &ci);
            const quad dr = (quad)c[k].re - cr, di = (quad)c[k].im - ci, e2 = dr * dr + di * di;
            if (e2 > worst2) worst2 = e2;
        };
        if (N <= (1 << 13)) {
            for (int64_t k = 0; k < N; ++k) look(k);
        } else {
            for (int64_t k = 0; k < N; k += 61) look(k);
            look(N - 1);
            uint64_t state = 88172645463325252ull;
            for (int r = 0; r < (naive ? 0 : 1000000); ++r) {   // (the stride alone shows the naive filler's loss)
                state ^= state << 13;
                state ^= state >> 7;
                state ^= state << 17;
                look((int64_t)(state % (uint64_t)N));
            }
        }
        printf("%lld %.6Lf\n", (long long)N, sqrtl((long double)(worst2 / (u * u))));
    }
    // c[0] = 1 exactly, and N = 12: c[6] = exp(-3 pi i) = -1, c[2] = exp(-i pi / 3)'s neighbours aside, c[3] = exp(-3 i pi / 4)
    std::vector<FidTw> c(12);
    fid_fill_chirp_table(12, c.data());
    const double h = 0.70710678118654752440;
    if (c[0].re != 1.0 || c[0].im != 0.0 || c[6].re != -1.0 || c[6].im != 0.0 || c[3].re != -h || c[3].im != -h) return 2;
    return 0;
}

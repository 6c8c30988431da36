// twiddle_check.hip -- compiled for the HOST by tests/test_fid_cpu.py: the twiddles of csrc/fid_twiddle.h against cosl /
// sinl of the exact angle.  Prints two numbers in units of u = 2^-53: the worst |omega^ - omega| over the whole stage
// table, and over the split twiddle at every T that a transform of length 2^lg (argv: the lg values) can ask for with
// a stride that keeps the run short, plus a fixed pseudo-random sample.
#include "fid_twiddle.h"

#include <cstdio>
#include <cstdlib>
#include <vector>

using namespace nmrfit;

static long double err_of(double re, double im, int64_t k, int lg)
{
    const long double pi = 3.14159265358979323846264338327950288L;
    const long double th = -2.0L * pi * (long double)k / (long double)((int64_t)1 << lg);
    const long double dr = (long double)re - cosl(th), di = (long double)im - sinl(th);
    return sqrtl(dr * dr + di * di);
}

int main(int argc, char **argv)
{
    std::vector<FidTw> stage(kFidStage);
    std::vector<FidTwDD> hi(kFidSplit), lo(kFidSplit);
    fid_fill_stage_table(stage.data());
    fid_fill_split_tables(hi.data(), lo.data());
    const long double u = 1.0L / 9007199254740992.0L;
    long double worst_stage = 0.0L, worst_split = 0.0L;
    for (int k = 0; k < kFidStage; ++k) {
        const long double e = err_of(stage[k].re, stage[k].im, k, kFidLgStage);
        if (e > worst_stage) worst_stage = e;
    }
    // the exact roots are exact
    if (stage[0].re != 1.0 || stage[0].im != 0.0 || stage[kFidStage / 4].re != 0.0 || stage[kFidStage / 4].im != -1.0 ||
        stage[kFidStage / 2].re != -1.0 || stage[kFidStage / 2].im != 0.0)
        return 2;
    for (int a = 1; a < argc; ++a) {
        const int lg = atoi(argv[a]);
        if (lg < 1 || lg > kFidLgMax) return 3;
        const int64_t n = (int64_t)1 << lg, stride = n > 65536 ? 61 : 1;
        for (int64_t t = 0; t < n; t += stride) {
            const FidTw w = fid_split_twiddle(hi.data(), lo.data(), (int)(t << (kFidLgMax - lg)));
            const long double e = err_of(w.re, w.im, t, lg);
            if (e > worst_split) worst_split = e;
        }
    }
    uint64_t state = 88172645463325252ull;
    for (int i = 0; i < 2000000; ++i) {
        state ^= state << 13;
        state ^= state >> 7;
        state ^= state << 17;
        const int T = (int)(state & (((uint64_t)1 << kFidLgMax) - 1));
        const FidTw w = fid_split_twiddle(hi.data(), lo.data(), T);
        const long double e = err_of(w.re, w.im, T, kFidLgMax);
        if (e > worst_split) worst_split = e;
    }
    printf("%.6Lf %.6Lf\n", worst_stage / u, worst_split / u);
    return 0;
}

// objective_prologue.h -- the per-particle prologue of objective_body (objective_kernel.h): the per-peak constants of the
// particle's row staged in the wave's (or the workgroup's) LDS records, with the two flags that pick the chunk loop's forms.
#pragma once
#include "objective_math.h"

namespace nmrfit {
namespace {

// The stages that were lambdas of objective_body are structs of REFERENCES to its variables with a call operator --
// what a by-reference closure is, written out so that it can live in a header.  (Not functions taking the same things as
// arguments: the compiler inlines a closure's call after it has derived the aliasing facts of objective_body's own
// pointers, a function's before; the kernels' instruction streams differ between the two, and tools/isa_hash.py holds
// them to the streams they had.)

// Stage a particle's per-peak constants in the wave's LDS slices (x: the particle's row, in global memory or -- fused
// swarm update -- in this wave's LDS copy); peaks first_pass * 64 ... in steps of pass_stride * 64.
template <bool kFast, bool kRec>
struct StagePeakConstants {
    double &p0, &p1, &r, &yoff;
    const int &P;
    const int &lane;
    const double &w0, &wspan;
    PeakLor *&lor;
    PeakWin *&win;
    bool &fast_bad;   // some group of eight peaks may not take the two-operation pair form
    PeakFast *&lorf;
    const double &lane_step, &rec_devk;
    bool &rec_bad;    // some peak may not take the Gaussian recurrence
    double2 *&grec;
    __device__ void operator()(const double *x, const int first_pass, const int pass_stride) const
    {
        p0 = x[0], p1 = x[1], r = x[2], yoff = x[3];   // equations.py:177
        for (int kb0 = first_pass * kWave; kb0 < P; kb0 += pass_stride * kWave) {   // every lane iterates (the group sums below shuffle)
            const int k = kb0 + lane;
            const bool have = k < P;
            const int kx = have ? k : 0;
            const double width = x[4 + 3 * kx], loc = x[5 + 3 * kx], a = x[6 + 3 * kx];
            const double ihw = 2.0 / width;
            const double locc = loc - w0;
            // |t| <= 1e18 keeps the grouped denominators finite: a width below 2e-18 of the spectral span
            // (|2/width| > lim) is evaluated as the floor width 2/lim, the WHOLE record of it (amplitudes too),
            // so the line is consistent in both channels: its dispersion tail a/(pi (w-loc)) does not depend on
            // the width and stays exact; the real tail is that of the floor width (DESIGN.md "Needle widths")
            const double lim = 1.0e18 / (wspan + fabs(locc));
            // (width 0: the amplitudes stay infinite, f non-finite like the reference's)
            const double it = (fabs(ihw) > lim) ? copysign(lim, ihw) : ihw;
            const double ia = __builtin_isinf(ihw) ? ihw : it;
            PeakLor rec;
            rec.ihw = it;
            rec.c = -locc * it;
            rec.al = a * r * ia * kInvPi;                             // a*r*(2/(pi*width))
            rec.ag2 = 2.0 * a * (1.0 - r) * ia * kSqrtLn2OverPi;      // 2 * a*(1-r)*(2/width)*sqrt(ln2/pi)
            if (have) lor[k] = rec;
            // window bounds in f32, rounded outwards (a slightly wider window is still exact)
            const double gw = kGaussWindow * fabs(width);
            const double wlo = locc - gw, whi = locc + gw;
            if (have) win[k] = PeakWin{(float)(wlo - fabs(wlo) * 1.2e-7 - 1e-37), (float)(whi + fabs(whi) * 1.2e-7 + 1e-37)};
            if (kFast) {
                // exponent budget of the group's denominator: s' <= (1 + tmax^2)/al, s' >= 1/al
                const double al = rec.al;
                const double tmax = fabs(it) * (wspan + fabs(locc));
                const bool pos = al > 0.0 && al < 1.0e300;                  // false for NaN
                const double ia = pos ? 1.0 / al : 1.0;
                const double rs = pos ? sqrt(ia) : 1.0;
                int ehi = pos ? ilogb(__builtin_fma(tmax, tmax, 1.0) * ia) + 2 : 100000;
                int elo = pos ? ilogb(ia) : -100000;
                if (ehi > 100000) ehi = 100000;                              // inf / overflow
                if (!have) ehi = elo = 0;                                    // beyond the last peak: no factor
                // (sums over the aligned groups of eight lanes: ds_swizzle, lane l reads lane l ^ m)
                ehi += __builtin_amdgcn_ds_swizzle(ehi, (1 << 10) | 0x1f);
                elo += __builtin_amdgcn_ds_swizzle(elo, (1 << 10) | 0x1f);
                ehi += __builtin_amdgcn_ds_swizzle(ehi, (2 << 10) | 0x1f);
                elo += __builtin_amdgcn_ds_swizzle(elo, (2 << 10) | 0x1f);
                ehi += __builtin_amdgcn_ds_swizzle(ehi, (4 << 10) | 0x1f);
                elo += __builtin_amdgcn_ds_swizzle(elo, (4 << 10) | 0x1f);
                // every group of (up to) 8 peaks must have positive amplitudes and a denominator that
                // stays within 2^+-1000 for kBatchInv points; ONE flag per particle -- all groups
                // qualify or none does -- keeps the chunk loop free of a per-group branch (whose two
                // arms cost 16 register copies per group in phi moves: measured, it ate the gain)
                if (have && !(ehi < 1000 / kBatchInv && elo > -1000 / kBatchInv)) fast_bad = true;
                // cs from the ROUNDED ihs (one rounding, like c from ihw): the zero of t' then sits at
                // loc to the same accuracy as the zero of t
                const double ihs = it * rs;
                if (have) lorf[k] = PeakFast{ihs, -locc * ihs, ia, 0.0};
            }
            if (kRec) {
                const double d = lane_step * it;
                const bool ok = (lane_step != 0.0) && (fabs(d) <= 2.0) && (fabs(it) * rec_devk <= 1.0);
                if (have && !ok) rec_bad = true;
                if (have) grec[k] = make_double2(d, ok ? exp2_neg(-2.0 * d * d) : 0.0);
            }
        }
    }
};

}  // namespace
}  // namespace nmrfit

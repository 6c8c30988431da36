// objective_lds.h -- the ONE description of the objective kernel's dynamic LDS.  objective_body (objective_kernel.h)
// takes every pointer into it from objective_lds_layout, and resolve_lds (objective_plan.h) sizes the launch and picks
// the fallback variant from the same function's `end`: a piece added here is added on both sides.
//
// The pieces, in order (byte offsets from the start of the dynamic LDS):
//   lor    PeakLor[slices][P]        per-peak Lorentzian / Gaussian constants
//   win    PeakWin[slices][P]        Gaussian windows                                     (then 16-byte alignment)
//   seeds  double2[wpb][kMaxBlocks]  per-wave table of block seeds (<= 16 blocks per grid)
//   shr    kSharedPrologueBytes      shared-prologue area: rotation step, lane seeds L_lane[64] re / im, one flag per wave
//   lseed  double[wpb][2 * kWave]    per-wave lane seeds -- only when the waves hold different particles (slices != 1);
//                                    a workgroup that is one particle keeps its one copy inside `shr`
//   far    double[wpb][far_stride]   far-field / imaginary-sum scratch (FARFIELD, or fit_im == 2)
//   grec   double2[slices][P]        (d, C) of the Gaussian recurrence (objective launches of DEFAULT / FARFIELD)
//   lorf   PeakFast[slices][P]       scaled records of the two-operation pair form (DEFAULT)
//   tab    kDawTabCount doubles      Dawson table (fit_im != 0), 16-byte aligned: the kernels' `aux_off`
// `slices`: copies of the per-peak records in a workgroup -- 1 when its waves are segments of one particle, else wpb.
#pragma once
#include "objective_launch.h"
#include "objective_math.h"

namespace nmrfit {
namespace {

struct ObjectiveLds {
    static constexpr size_t lor = 0;   // the first piece starts the area
    size_t win, seeds, shr, lseed, far, grec, lorf, tab, end;
};

constexpr __host__ __device__ ObjectiveLds objective_lds_layout(int variant, bool residual, int fit_im, int P, int wpb, int slices)
{
    ObjectiveLds L{};
    L.win = (size_t)slices * P * sizeof(PeakLor);
    L.seeds = ((size_t)slices * P * (sizeof(PeakLor) + sizeof(PeakWin)) + 15) & ~(size_t)15;
    L.shr = L.seeds + (size_t)wpb * kMaxBlocks * sizeof(double2);
    L.lseed = L.shr + kSharedPrologueBytes;
    L.far = L.lseed + (slices == 1 ? 0 : (size_t)wpb * 2 * kWave * sizeof(double));
    L.grec = L.far + ((is_farfield(variant) || fit_im == 2) ? (size_t)wpb * far_stride(fit_im) * sizeof(double) : 0);
    const bool rec = !residual && (variant == NMRFIT_VARIANT_DEFAULT || is_farfield(variant));
    L.lorf = L.grec + (rec ? (size_t)slices * P * sizeof(double2) : 0);
    L.tab = (L.lorf + (variant == NMRFIT_VARIANT_DEFAULT ? (size_t)slices * P * sizeof(PeakFast) : 0) + 15) & ~(size_t)15;
    L.end = L.tab + (fit_im != 0 ? (size_t)kDawTabCount * sizeof(double) + 16 : 0);
    return L;
}

// The pair form (objective_pair.h: a four-wave workgroup is TWO particles, wave s holds segment s of both).  Its pieces:
//   lor    PeakLor[2][P]             the records of particle A, then of particle B -- like every piece with a [2]
//   lorf   PeakFast[2][P]
//   grec   double2[2][P]
//   win    PeakWin[2][P]                                                                  (then 16-byte alignment)
//   seeds  double2[2][4][kMaxBlocks] per-wave tables of block seeds
//   shr    [2] kSharedPrologueBytes  rotation step, lane seeds, one flag per wave
//   park   f64x2[4][4][kWave]        per wave: A's eight accumulators while B's model runs, [16-byte piece][lane]
//                                    (a lane's ds_*_b128 accesses of one piece are consecutive: conflict-free)
//   state  double[4][2][3][kWave]    per wave and particle: the phase recurrence (re, im) and the block's sum of squares
//                                    of every lane, between the particle's epilogues
struct ObjectivePairLds {
    static constexpr size_t lor = 0;
    size_t lorf, grec, win, seeds, shr, park, state, end;
};
constexpr int kPairParticles = 2;
constexpr size_t kPairParkBytes = (size_t)kPointsPerLane * sizeof(double) * kWave;   // per wave
constexpr size_t kPairStateBytes = (size_t)kPairParticles * 3 * sizeof(double) * kWave;   // per wave

constexpr __host__ __device__ ObjectivePairLds objective_pair_lds_layout(int P)
{
    ObjectivePairLds L{};
    const size_t n = (size_t)kPairParticles * P;
    L.lorf = n * sizeof(PeakLor);
    L.grec = L.lorf + n * sizeof(PeakFast);
    L.win = L.grec + n * sizeof(double2);
    L.seeds = (L.win + n * sizeof(PeakWin) + 15) & ~(size_t)15;
    L.shr = L.seeds + (size_t)kPairParticles * kWavesPerBlock * kMaxBlocks * sizeof(double2);
    L.park = L.shr + (size_t)kPairParticles * kSharedPrologueBytes;
    L.state = L.park + (size_t)kWavesPerBlock * kPairParkBytes;
    L.end = L.state + (size_t)kWavesPerBlock * kPairStateBytes;
    return L;
}
// the pair kernel's own __shared__: one wsums block per particle (+ alignment slack)
constexpr size_t kPairStaticLds = (size_t)kPairParticles * kWsumsCount * sizeof(double) + 64;
// Four workgroups per CU at the headline shape: records of 24 peaks, one fused row per particle, static LDS -- within a
// quarter of the CU's 160 KiB
static_assert(kSharedPrologueBytes % 16 == 0 && sizeof(PeakLor) % 16 == 0 && sizeof(PeakFast) % 16 == 0, "16-byte pieces");
static_assert(objective_pair_lds_layout(24).end + 16 + (size_t)kPairParticles * (4 + 3 * 24) * sizeof(double) + kPairStaticLds <= 40 * 1024,
              "pair form: four workgroups no longer fit on a CU at P = 24");

}  // namespace
}  // namespace nmrfit

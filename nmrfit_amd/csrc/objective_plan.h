// objective_plan.h -- the ONE place where the rules of an objective launch live: a pure function of plain values
// (plan_objective) that decides, in this order, the channels, the segments per particle, the kernel variant that fits in
// LDS, the workgroup form (four waves, eight waves, or the pair form), the workgroups, where the fused swarm rows lie,
// how much of a swarm generation rides in the launch, and where f is written.  Host arithmetic only, no pointers, no
// HIP call: launch_objective (objective.hip) builds the input, calls the plan and carries it out, and
// tests/launch_plan/plan_sweep.hip walks the plan over millions of shapes on a machine without a GPU.
// Every rule stands here next to the measurement that justified it.
#pragma once
#include "objective_launch.h"
#include "objective_lds.h"

#include <algorithm>

namespace nmrfit {
namespace {

// ---- the kernel variant that fits, and the dynamic LDS of its records ------------------------------------------------
// The kernel variant a launch actually runs (the requested one may not fit in LDS, or may not
// implement the imaginary part) and the dynamic LDS its per-wave records need.
constexpr size_t kStaticLds = kObjectiveStaticLds;   // objective_kernel's own __shared__ (wsums) + alignment slack
static_assert(kObjectiveStaticLds == (size_t)kWsumsCount * sizeof(double) + 64, "objective_launch.h and objective_math.h disagree");
struct ResolvedLds {
    int variant;
    size_t lds;
    unsigned aux_off;
};
// Every size is the `end` of the kernel's own layout (objective_lds.h); here is only the fallback rule.
// `slices`: copies of the per-peak records in a workgroup (1 when its waves are segments of one particle, else wpb);
// `rows`: copies of the updated row kept for a fused swarm generation (0: none)
constexpr ResolvedLds resolve_lds(int variant, int32_t P, bool residual, int fit_im, int wpb, int slices, int rows)
{
    // the mixed-precision far-field kernel exists for objective launches without the imaginary channel; everything else
    // of a context set to it runs the fp64 far-field kernel (same records, same LDS)
    const bool want32 = variant == NMRFIT_VARIANT_FARFIELD32;
    if (want32) variant = NMRFIT_VARIANT_FARFIELD;
    const int np = P > 1 ? P : 1;
    // what a workgroup may take of a CU's 160 KiB for the records sized here: everything but the kernel's static
    // LDS and (swarm generations) the per-wave copies of the updated rows that plan_objective appends
    const size_t room = kCuLdsBytes - kStaticLds -
                        (rows ? (size_t)rows * (size_t)(4 + 3 * (int64_t)P) * sizeof(double) + 16 : 0);
    // (the imaginary channel exists in DEFAULT, NOREC and FARFIELD; the A/B variants fail in launch_variant)
    if (variant == NMRFIT_VARIANT_FARFIELD && objective_lds_layout(variant, residual, fit_im, np, wpb, slices).end + 16 > room)
        variant = NMRFIT_VARIANT_DEFAULT;   // P > ~600
    if (variant == NMRFIT_VARIANT_DEFAULT && objective_lds_layout(variant, residual, fit_im, np, wpb, slices).end + 16 > room)
        variant = NMRFIT_VARIANT_NOREC;     // P > ~450: no room for the recurrence / scaled records
    const ObjectiveLds at = objective_lds_layout(variant, residual, fit_im, np, wpb, slices);
    if (want32 && variant == NMRFIT_VARIANT_FARFIELD && !residual && fit_im == 0) variant = NMRFIT_VARIANT_FARFIELD32;
    return ResolvedLds{variant, at.end, fit_im != 0 ? (unsigned)at.tab : 0u};
}
// The totals of the hand-added formula this function replaced, on both sides of every switch: a change of the layout
// that moves the host's answer by a byte does not compile.  Columns: objective / residual launch x fit_im 0, 1, 2 x
// (4 waves: one copy of the records, four; 8 waves: one copy, eight), no fused rows.
struct LdsPin {
    int variant, P;
    size_t lds[24];
};
constexpr LdsPin kLdsPins[] = {
    {NMRFIT_VARIANT_DEFAULT, 1, {2224, 6576, 3248, 12048, 7968, 12320, 8992, 17792, 43808, 48160, 80672, 89472, 2208, 6512, 3232, 11920, 7952, 12256, 8976, 17664, 43792, 48096, 80656, 89344}},
    {NMRFIT_VARIANT_DEFAULT, 6, {2656, 8336, 3680, 15568, 8400, 14080, 9424, 21312, 44240, 49920, 81104, 92992, 2560, 7952, 3584, 14800, 8304, 13696, 9328, 20544, 44144, 49536, 81008, 92224}},
    {NMRFIT_VARIANT_DEFAULT, 32, {4944, 17488, 5968, 33872, 10688, 23232, 11712, 39616, 46528, 59072, 83392, 111296, 4432, 15440, 5456, 29776, 10176, 21184, 11200, 35520, 46016, 57024, 82880, 107200}},
    {NMRFIT_VARIANT_DEFAULT, 33, {5040, 17840, 6064, 34576, 10784, 23584, 11808, 40320, 46624, 59424, 83488, 112000, 4512, 15728, 5536, 30352, 10256, 21472, 11280, 36096, 46096, 57312, 82960, 107776}},
    {NMRFIT_VARIANT_DEFAULT, 132, {13744, 52688, 14768, 104272, 19488, 58432, 20512, 110016, 55328, 94272, 92192, 131008, 11632, 44240, 12656, 87376, 17376, 49984, 18400, 93120, 53216, 85824, 90080, 131008}},
    {NMRFIT_VARIANT_DEFAULT, 133, {13840, 53040, 14864, 104976, 19584, 58784, 20608, 110720, 55424, 94624, 92288, 131328, 11712, 44528, 12736, 87952, 17456, 50272, 18480, 93696, 53296, 86112, 90160, 131328}},
    {NMRFIT_VARIANT_DEFAULT, 452, {41904, 78544, 42928, 155984, 47648, 84288, 48672, 161728, 83488, 120128, 120352, 233408, 34672, 136400, 35696, 155984, 40416, 142144, 41440, 161728, 76256, 120128, 113120, 233408}},
    {NMRFIT_VARIANT_DEFAULT, 606, {55456, 103184, 56480, 205264, 61200, 108928, 62224, 211008, 97040, 144768, 133904, 282688, 45760, 103184, 46784, 205264, 51504, 108928, 52528, 211008, 87344, 144768, 124208, 282688}},
    {NMRFIT_VARIANT_DEFAULT, 960, {86608, 159824, 87632, 318544, 92352, 165568, 93376, 324288, 128192, 201408, 118976, 395968, 71248, 159824, 72272, 318544, 76992, 165568, 78016, 324288, 112832, 201408, 149696, 395968}},
    {NMRFIT_VARIANT_FARFIELD, 1, {37008, 41264, 72848, 81424, 42752, 47008, 78592, 87168, 43776, 48032, 80640, 89216, 36992, 41200, 72832, 81296, 42736, 46944, 78576, 87040, 43760, 47968, 80624, 89088}},
    {NMRFIT_VARIANT_FARFIELD, 6, {37280, 42384, 73120, 83664, 43024, 48128, 78864, 89408, 44048, 49152, 80912, 91456, 37184, 42000, 73024, 82896, 42928, 47744, 78768, 88640, 43952, 48768, 80816, 90688}},
    {NMRFIT_VARIANT_FARFIELD, 32, {38736, 48208, 74576, 95312, 44480, 53952, 80320, 101056, 45504, 54976, 82368, 103104, 38224, 46160, 74064, 91216, 43968, 51904, 79808, 96960, 44992, 52928, 81856, 99008}},
    {NMRFIT_VARIANT_FARFIELD, 33, {38800, 48432, 74640, 95760, 44544, 54176, 80384, 101504, 45568, 55200, 82432, 103552, 38272, 46320, 74112, 91536, 44016, 52064, 79856, 97280, 45040, 53088, 81904, 99328}},
    {NMRFIT_VARIANT_FARFIELD, 132, {44336, 70608, 80176, 140112, 50080, 76352, 85920, 145856, 51104, 77376, 87968, 147904, 42224, 62160, 78064, 123216, 47968, 67904, 83808, 128960, 48992, 68928, 85856, 131008}},
    {NMRFIT_VARIANT_FARFIELD, 133, {44400, 70832, 80240, 140560, 50144, 76576, 85984, 146304, 51168, 77600, 88032, 148352, 42272, 62320, 78112, 123536, 48016, 68064, 83856, 129280, 49040, 69088, 85904, 131328}},
    {NMRFIT_VARIANT_FARFIELD, 452, {62256, 142288, 98096, 155984, 68000, 148032, 103840, 161728, 69024, 149056, 105888, 233408, 55024, 113360, 90864, 155984, 60768, 119104, 96608, 161728, 61792, 120128, 98656, 233408}},
    {NMRFIT_VARIANT_FARFIELD, 606, {70880, 103184, 106720, 205264, 76624, 108928, 112464, 211008, 77648, 144768, 114512, 282688, 61184, 138000, 97024, 205264, 66928, 143744, 102768, 211008, 67952, 144768, 104816, 282688}},
    {NMRFIT_VARIANT_FARFIELD, 960, {90704, 159824, 126544, 318544, 96448, 165568, 132288, 324288, 97472, 201408, 134336, 395968, 75344, 159824, 111184, 318544, 81088, 165568, 116928, 324288, 82112, 201408, 118976, 395968}},
    {NMRFIT_VARIANT_NOREC, 1, {2176, 6384, 3200, 11664, 7920, 12128, 8944, 17408, 43760, 47968, 80624, 89088, 2176, 6384, 3200, 11664, 7920, 12128, 8944, 17408, 43760, 47968, 80624, 89088}},
    {NMRFIT_VARIANT_NOREC, 6, {2368, 7184, 3392, 13264, 8112, 12928, 9136, 19008, 43952, 48768, 80816, 90688, 2368, 7184, 3392, 13264, 8112, 12928, 9136, 19008, 43952, 48768, 80816, 90688}},
    {NMRFIT_VARIANT_NOREC, 32, {3408, 11344, 4432, 21584, 9152, 17088, 10176, 27328, 44992, 52928, 81856, 99008, 3408, 11344, 4432, 21584, 9152, 17088, 10176, 27328, 44992, 52928, 81856, 99008}},
    {NMRFIT_VARIANT_NOREC, 33, {3456, 11504, 4480, 21904, 9200, 17248, 10224, 27648, 45040, 53088, 81904, 99328, 3456, 11504, 4480, 21904, 9200, 17248, 10224, 27648, 45040, 53088, 81904, 99328}},
    {NMRFIT_VARIANT_NOREC, 132, {7408, 27344, 8432, 53584, 13152, 33088, 14176, 59328, 48992, 68928, 85856, 131008, 7408, 27344, 8432, 53584, 13152, 33088, 14176, 59328, 48992, 68928, 85856, 131008}},
    {NMRFIT_VARIANT_NOREC, 133, {7456, 27504, 8480, 53904, 13200, 33248, 14224, 59648, 49040, 69088, 85904, 131328, 7456, 27504, 8480, 53904, 13200, 33248, 14224, 59648, 49040, 69088, 85904, 131328}},
    {NMRFIT_VARIANT_NOREC, 452, {20208, 78544, 21232, 155984, 25952, 84288, 26976, 161728, 61792, 120128, 98656, 233408, 20208, 78544, 21232, 155984, 25952, 84288, 26976, 161728, 61792, 120128, 98656, 233408}},
    {NMRFIT_VARIANT_NOREC, 606, {26368, 103184, 27392, 205264, 32112, 108928, 33136, 211008, 67952, 144768, 104816, 282688, 26368, 103184, 27392, 205264, 32112, 108928, 33136, 211008, 67952, 144768, 104816, 282688}},
    {NMRFIT_VARIANT_NOREC, 960, {40528, 159824, 41552, 318544, 46272, 165568, 47296, 324288, 82112, 201408, 118976, 395968, 40528, 159824, 41552, 318544, 46272, 165568, 47296, 324288, 82112, 201408, 118976, 395968}},
};
constexpr bool lds_pins_hold()
{
    for (const LdsPin &p : kLdsPins) {
        int c = 0;
        for (int residual = 0; residual < 2; ++residual)
            for (int fit_im = 0; fit_im < 3; ++fit_im)
                for (int wpb = kWavesPerBlock; wpb <= kWideWaves; wpb += kWavesPerBlock)
                    for (int slices = 1; slices <= wpb; slices += wpb - 1)
                        if (resolve_lds(p.variant, p.P, residual != 0, fit_im, wpb, slices, 0).lds != p.lds[c++]) return false;
    }
    return true;
}
static_assert(lds_pins_hold(), "objective_lds() moved: the layout of objective_lds.h no longer adds up to the pinned totals");

// ---- what a launch is asked for, and what is decided ------------------------------------------------------------------
struct ObjectivePlanInput {
    int64_t S = 0;                 // particles
    int32_t P = 0;                 // peaks
    int64_t N = 0;                 // grid points (nmrfit_ctx::N)
    // of the context
    int compute_units = 0;
    int64_t target_waves = 0;      // launch-geometry override (0 = the rules below)
    int variant = NMRFIT_VARIANT_DEFAULT;
    int fit_im = 0;
    bool wide_workgroups = true;
    int pair_waves = -1;
    // of the call
    bool residual = false;         // residual rows are asked for (dR)
    int rows_fit_im = 0;           // ... of both channels (1 or 2)
    bool defer = false;            // an ObjectiveDeferred record was passed
    bool fused = false;            // a PsoFused record was passed ...
    bool fused_rows = false;       // ... and asks for the swarm update (x_in)
    bool pbest = false, tail = false, pending = false;   // ... its pbest / tail / pending, as flags
    int seg_rule = 4;              // NMRFIT_SEG_RULE (A/B knob): 3 = the round-3 rule (~16 tasks per SIMD)
};

// the translation unit whose kernel runs (objective_launch.h: launch_objective_*)
enum ObjectiveUnit { kUnitNone = -1, kUnitDefault, kUnitFarfield, kUnitFarfield32, kUnitNorec, kUnitRowsIm, kUnitPair, kUnitAB };

struct ObjectivePlan : ObjectiveGeometry {
    int code = NMRFIT_OK;          // not NMRFIT_OK: `message` is the error text and nothing else holds
    const char *message = nullptr;
    ObjectiveUnit unit = kUnitNone;   // kUnitNone: nothing is launched (no particles, or need_flush)
    int variant = NMRFIT_VARIANT_DEFAULT;   // the variant that runs (kUnitAB: the A/B library's BASELINE / NOSKIP, an error in the product)
    unsigned xrow_off = 0;         // byte offset of the fused swarm rows in dynamic LDS (PsoFused::xrow_off)
    int rows = 0;                  // ... and how many copies of a row
    bool pbest = false;            // the personal bests ride in the launch
    bool tail = false;             // ... and the whole generation (PsoFused::tail)
    bool need_flush = false;       // a fold waits that this launch cannot do: the caller folds and comes back
    bool direct_f = false;         // the kernel writes f; else per-block sums go to the partial buffer
    int64_t partial_doubles = 0;   // what the partial buffer must hold (0 when direct_f)
    int64_t waves = 0;             // as nmrfit_last_launch reports them
};

// ---- segments per particle --------------------------------------------------------------------------------------------
// Segmenting: a wave is one (particle, segment) task; a segment is a whole number of blocks.  Swarms that already
// supply enough waves get nseg = 1 and the wave writes f directly.  (Rounds 1-3 aimed at ~16 tasks per SIMD so that
// the hardware dispatcher load-balances -- C3: 4096 one-per-particle waves 1.81 ms, 16384 waves 1.74 ms; the
// round-4 rule below replaces it unless NMRFIT_SEG_RULE=3 or an explicit target is set.)
constexpr int64_t plan_segments(const ObjectivePlanInput &in, const BlockPlan &bp)
{
    const int64_t S = in.S, n_chunks = bp.n_chunks, n_blocks = bp.n_blocks;
    int64_t target_waves = (int64_t)in.compute_units * 4 * 16;
    if (in.target_waves > 0) target_waves = in.target_waves;
    int64_t nseg = std::max<int64_t>(1, std::min<int64_t>(n_blocks, (target_waves + S - 1) / S));
    if (in.target_waves == 0 && in.seg_rule != 3) {
        // Round 4 (the selectable kernels now run four waves per SIMD): as few segments as fill the chip ONCE -- every
        // further segment repeats a wave's prologue and cuts its chunk loop shorter (1024 x 16384 x 12: 16 segments
        // 69 us, 4 segments 60 us; 4096 x 4096 x 6: 4 segments 56 us, 1 segment 49 us) -- but four where a wave then
        // still has 16 chunks or more: the prologue no longer counts there, and four segments make the workgroup
        // the particle (f and the personal best finished in the launch)
        const int64_t slots = (int64_t)in.compute_units * 4 * 4;
        nseg = std::max<int64_t>(1, std::min<int64_t>(n_blocks, (slots + S - 1) / S));
        if (n_chunks / 4 >= 16) nseg = std::max<int64_t>(nseg, std::min<int64_t>(4, n_blocks));
    }
    // Short grids: a wave's own prologue (block seeds, pointers, the barrier of the shared part) still
    // costs a good fraction of a chunk, so prefer >= 2 chunks per wave as long as two waves per SIMD
    // remain (measured on C2, S=1024 N=4096, with the per-workgroup prologue: 8 segments 25.0 us,
    // 4 segments 22.7 us, 2 segments 23.3 us; round 1, prologue per wave: 8 -> 26.2, 2 -> 22.2).
    if (in.target_waves == 0) {
        const int64_t simds = (int64_t)in.compute_units * 4;
        while (nseg > 1 && n_chunks / nseg < 2 && S * ((nseg + 1) / 2) >= 2 * simds) nseg = (nseg + 1) / 2;
        // a small swarm whose waves just miss fitting on the chip at once (three per SIMD) while half
        // as many would leave it well filled: take the half (204 x 16384 x 12: 16 segments 30.4 us per
        // generation, 8 segments 28.5; tools/archive/nseg_generation_ab.py)
        if (nseg > 1 && S * nseg > 3 * simds && S * (nseg / 2) < 2 * simds && n_chunks / nseg <= 2) nseg /= 2;
    }
    return nseg;
}

// ---- the workgroup forms ----------------------------------------------------------------------------------------------
// the swarms the two whole-generation forms of a fused launch take (PsoFused::tail), by waves per workgroup
constexpr bool tail_fits(const ObjectivePlanInput &in, int wpb)
{
    return in.tail && in.S <= (int64_t)kDeferredPerLane * kWave * wpb;
}
// What a workgroup is, and the LDS it takes before the fused rows are appended.
struct ObjectiveForm {
    int wpb;             // waves per workgroup
    int rows;            // copies of the updated row of a fused swarm generation
    int variant;         // the variant whose records fit beside them
    size_t lds;          // dynamic LDS of the records
    unsigned aux_off;
    size_t static_lds;   // the kernel's own __shared__
    bool pair;
};
// The single form: a workgroup of `wpb` waves, each a (particle, segment).
// LDS copies: per-peak records once per workgroup when its waves are segments of ONE particle (nseg a multiple of
// the waves per workgroup), else once per wave; the updated row of a fused swarm generation likewise, plus two
// more rows (g, the winner's row) when the workgroup may finish the generation (objective_finish.h, personal_best)
constexpr ObjectiveForm single_form(const ObjectivePlanInput &in, int64_t nseg, int fit_im, int wpb)
{
    const bool one_particle = (nseg % wpb == 0);   // (objective_body: `shared`)
    const int slices = one_particle ? 1 : wpb;
    const int rows = !in.fused_rows ? 0 : !one_particle ? wpb : (nseg == wpb && tail_fits(in, wpb)) ? 3 : 1;
    const ResolvedLds r = resolve_lds(in.variant, in.P, in.residual, fit_im, wpb, slices, rows);
    return ObjectiveForm{wpb, rows, r.variant, r.lds, r.aux_off, kStaticLds, false};
}
// The pair form (objective_pair.h): a four-wave workgroup is TWO particles cut into four segments, and a wave fetches
// every chunk of the grid once for both.  Its own records and static LDS, the rows of both particles, no Dawson table.
constexpr ObjectiveForm pair_form(const ObjectivePlanInput &in, const ObjectiveForm &four)
{
    return ObjectiveForm{kWavesPerBlock, kPairParticles * four.rows, NMRFIT_VARIANT_DEFAULT,
                         objective_pair_lds_layout(in.P > 1 ? in.P : 1).end, 0u, kPairStaticLds, true};
}

// one translation unit per selectable variant (they compile in parallel); every other variant is the A/B library's
constexpr ObjectiveUnit unit_of(int variant, bool rows_im, bool pair)
{
    if (rows_im) return kUnitRowsIm;
    switch (variant) {
        case NMRFIT_VARIANT_DEFAULT: return pair ? kUnitPair : kUnitDefault;
        case NMRFIT_VARIANT_FARFIELD: return kUnitFarfield;
        case NMRFIT_VARIANT_FARFIELD32: return kUnitFarfield32;
        case NMRFIT_VARIANT_NOREC: return kUnitNorec;
        default: return kUnitAB;
    }
}

constexpr ObjectivePlan plan_error(int code, const char *message)
{
    ObjectivePlan p{};
    p.code = code;
    p.message = message;
    return p;
}

// ---- the plan ---------------------------------------------------------------------------------------------------------
constexpr ObjectivePlan plan_objective(const ObjectivePlanInput &in)
{
    ObjectivePlan p{};
    const int64_t S = in.S, N = in.N;

    // 1. Channels.  Residual rows see the real channel alone, except in the one call that asks for both (nmrfit_internal.h)
    const bool rows_im = in.residual && in.rows_fit_im != 0;
    if (rows_im && (in.defer || in.fused || (in.rows_fit_im != 1 && in.rows_fit_im != 2)))
        return plan_error(NMRFIT_E_INVALID, "launch_objective: residual rows of both channels take fit_im 1 or 2 and no swarm update");
    const int fit_im = rows_im ? in.rows_fit_im : in.residual ? 0 : in.fit_im;
    p.fit_im = fit_im;
    if (S == 0) return p;

    // 2. Blocks: the unit of the canonical summation / phase re-seeding, a function of N only
    // (at most 16 per grid), so that results do not depend on S or on sharding.
    const BlockPlan bp = block_plan(N);
    p.blk_chunks = bp.blk_chunks;
    p.n_blocks = (int)bp.n_blocks;

    // 3. Segments per particle, each a whole number of blocks
    const int64_t asked = plan_segments(in, bp);
    p.seg_len = ((bp.n_blocks + asked - 1) / asked) * bp.blk_len;
    const int64_t nseg = (N + p.seg_len - 1) / p.seg_len;
    p.nseg = (int)nseg;
    p.seg_blocks = (int)(p.seg_len / bp.blk_len);
    const int64_t waves = S * nseg;

    // 4. The variant: the four-wave form's, after the fallback of resolve_lds
    // (the context's own variant too: a FARFIELD context whose records no longer fit resolves to DEFAULT)
    const ObjectiveForm four = single_form(in, nseg, fit_im, kWavesPerBlock);
    p.variant = four.variant;
    if (rows_im && (p.variant != NMRFIT_VARIANT_DEFAULT || in.variant != NMRFIT_VARIANT_DEFAULT))
        return plan_error(NMRFIT_E_UNSUPPORTED, "residual rows with the imaginary channel exist for the DEFAULT kernel variant only (and while its LDS records fit)");

    // 5. The workgroup form
    const size_t xrow_bytes = in.fused_rows ? (size_t)(4 + 3 * (int64_t)in.P) * sizeof(double) : 0;
    ObjectiveForm form = four;
    // Eight segments per particle (small swarms on short grids -- the reference's default 204 x 4096): an EIGHT-wave
    // workgroup is the particle, as the four-wave workgroup is for four segments: one prologue per particle, block
    // sums through LDS, f (and, in a swarm generation, the personal best) finished in this launch.
    if (nseg == kWideWaves && !in.residual && fit_im == 0 && has_eight_wave_form(p.variant) && in.wide_workgroups) {
        const ObjectiveForm eight = single_form(in, nseg, fit_im, kWideWaves);
        if (eight.variant == p.variant && lds_fits(eight.lds, eight.static_lds, (size_t)eight.rows * xrow_bytes)) form = eight;
    }
    // The pair form, for objective launches of the DEFAULT kernel whose pairs still fill the
    // chip's four-waves-per-SIMD slots once (smaller swarms keep a workgroup per particle: more of them to spread);
    // NMRFIT_PAIR_WAVES=0 / 1: never / wherever the geometry allows (A/B knob, nmrfit_ctx::pair_waves).
    if (p.variant == NMRFIT_VARIANT_DEFAULT && !in.residual && fit_im == 0 && nseg == kWavesPerBlock && form.wpb == kWavesPerBlock &&
        in.pair_waves != 0 && (in.pair_waves > 0 || (S / 2) * kWavesPerBlock >= (int64_t)in.compute_units * 4 * 4)) {
        const ObjectiveForm two = pair_form(in, four);
        if (lds_fits(two.lds, two.static_lds, (size_t)two.rows * xrow_bytes)) form = two;
    }
    p.wpb = form.wpb;
    p.pair = form.pair;
    p.rows = form.rows;
    p.lds = form.lds;
    p.aux_off = form.aux_off;

    // 6. Workgroups, and the two limits of a launch
    p.blocks = form.pair ? (S + 1) / 2 : (waves + form.wpb - 1) / form.wpb;
    if (p.blocks > 0x7fffffffLL) return plan_error(NMRFIT_E_INVALID, "swarm too large for one launch");
    if (!lds_fits(form.lds, form.static_lds, (size_t)form.rows * xrow_bytes))
        return plan_error(NMRFIT_E_UNSUPPORTED, "too many peaks for the kernel's LDS records (with the imaginary model / the fused swarm update)");

    // 7. Fused swarm update: the copies of the particle's updated row, after everything else
    if (in.fused_rows) {
        if (in.residual || (4 + 3 * (int64_t)in.P) > kFusedMaxD)
            return plan_error(NMRFIT_E_INVALID, "fused swarm update: objective launches with D <= kFusedMaxD only");
        p.lds = (p.lds + 15) & ~(size_t)15;
        p.xrow_off = (unsigned)p.lds;
        p.lds += (size_t)form.rows * (size_t)(4 + 3 * (int64_t)in.P) * sizeof(double);
    }

    // 8. Where f is written.  nseg == 1: the wave writes f; nseg == 4 (or 8, wide form): the waves of a workgroup are the
    // particle's segments and the workgroup writes f (block sums through LDS); otherwise per-block sums go to a
    // buffer and finalize_kernel (or the swarm's select kernel) adds them.  Same summation order in all.
    p.direct_f = (nseg == 1 || nseg == form.wpb);
    p.partial_doubles = p.direct_f ? 0 : S * bp.n_blocks * (fit_im ? 2 : 1);

    // 9. How much of the generation rides in the launch: the personal bests only when ONE workgroup holds the whole
    // particle (else the caller's kernel); the whole generation only on top of the personal bests
    p.pbest = in.fused_rows && in.pbest && nseg == form.wpb;
    p.tail = p.pbest && tail_fits(in, form.wpb);
    if (in.fused && in.tail && in.pending && !p.tail) {
        // a generation waits to be folded and this launch cannot do it (the variant or fit_im changed between two
        // generations): nothing is launched, the caller folds in a launch of its own and comes back
        if (!in.defer) return plan_error(NMRFIT_E_STATE, "launch_objective: pending fold without a deferred-launch record");
        p.need_flush = true;
        return p;
    }

    // 10. The kernel unit
    p.unit = unit_of(p.variant, rows_im, form.pair);
    p.waves = form.pair ? p.blocks * form.wpb : waves;   // (the pair form: a wave holds a segment of two particles)
    return p;
}

// The headline swarm generation (4096 x 65536 x 24 on 256 CUs) takes the pair form with everything in the launch; the
// reference's default fit (204 x 4096 x 6) is eight segments in an eight-wave workgroup.
constexpr ObjectivePlanInput swarm_generation(int64_t S, int64_t N, int32_t P)
{
    ObjectivePlanInput in{};
    in.S = S, in.N = N, in.P = P, in.compute_units = 256;
    in.defer = in.fused = in.fused_rows = in.pbest = in.tail = true;
    return in;
}
static_assert(plan_objective(swarm_generation(4096, 65536, 24)).unit == kUnitPair && plan_objective(swarm_generation(4096, 65536, 24)).pbest &&
              !plan_objective(swarm_generation(4096, 65536, 24)).tail, "the headline launch left the pair form");
static_assert(plan_objective(swarm_generation(204, 4096, 6)).wpb == kWideWaves && plan_objective(swarm_generation(204, 4096, 6)).tail,
              "the default fit's generation is no longer one launch of eight-wave workgroups");

}  // namespace
}  // namespace nmrfit

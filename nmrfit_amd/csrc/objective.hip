// objective.hip -- host side of the hot path: launch geometry (segments per particle, waves per workgroup), the LDS
// budget that picks the kernel form, and the launch itself (launch_objective); plus the small kernels around it
// (block-sum finalisation, grid preparation; the post-fit reconstruction is result.hip).  The objective kernel is
// objective_kernel.h; its instantiations live in objective_{default,farfield,norec}.hip, the DEFAULT kernel's pair form
// (two particles per workgroup) in objective_pair.h / objective_pair.hip.
#include "objective_launch.h"
#include "objective_lds.h"
#include "objective_math.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>

namespace nmrfit {
namespace {

// f[i] = sqrt( (sum of the particle's per-block sums, in grid order) / N ); with the imaginary
// part: the mean of the real and imaginary RMSE (two sums per block)
__global__ void finalize_kernel(const double *__restrict__ partial, int64_t S, int64_t n_chunks, int64_t N,
                                int fit_im, double *__restrict__ f)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= S) return;
    f[i] = finalize_value(partial + i * n_chunks * (fit_im ? 2 : 1), n_chunks, N, fit_im);
}

// residual rows of both channels (launch_objective, rows_fit_im): the two RMSEs of every row from the same per-block
// sums in the same order -- 0.5 * (f2[2 i] + f2[2 i + 1]) is what finalize_kernel gives
__global__ void finalize_rows_im_kernel(const double *__restrict__ partial, int64_t S, int64_t n_blocks, int64_t N,
                                        double *__restrict__ f2)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= S) return;
    const double *p = partial + i * n_blocks * 2;
    double ss = 0.0, si = 0.0;
    for (int64_t c = 0; c < n_blocks; ++c) {
        ss += p[2 * c];
        si += p[2 * c + 1];
    }
    f2[2 * i] = sqrt(ss / (double)N);
    f2[2 * i + 1] = sqrt(si / (double)N);
}

// per-chunk (min, max) of the centred grid: one wave per chunk
__global__ void chunk_minmax_kernel(const double *__restrict__ wc, int64_t N, int64_t n_chunks,
                                    double2 *__restrict__ out)
{
    const int64_t c = (int64_t)blockIdx.x * (blockDim.x / kWave) + (threadIdx.x >> 6);
    if (c < n_chunks) chunk_minmax_wave(wc, N, c, threadIdx.x & (kWave - 1), out);
}

__global__ void centre_kernel(const double *__restrict__ w, int64_t N, double w0, double *__restrict__ wc)
{
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j < N) wc[grid_slot(j)] = w[j] - w0;
}

__global__ void scatter_grid_kernel(const double *__restrict__ src, int64_t N, double *__restrict__ dst)
{
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j < N) dst[grid_slot(j)] = src[j];
}

}  // namespace

// Builds the derived device arrays of a context (centred grid, chunk table).
int prepare_grid(nmrfit_ctx *ctx, const double *d_w_raw)
{
    const int64_t N = ctx->N;
    hipLaunchKernelGGL(centre_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, ctx->stream, d_w_raw, N,
                       ctx->w0, ctx->d_wc);
    NMRFIT_HIP(hipGetLastError());
    const int waves_per_block = 4;
    hipLaunchKernelGGL(chunk_minmax_kernel, dim3((unsigned)((ctx->n_chunks + waves_per_block - 1) / waves_per_block)),
                       dim3(kWave * waves_per_block), 0, ctx->stream, ctx->d_wc, N, ctx->n_chunks, ctx->d_chunk);
    NMRFIT_HIP(hipGetLastError());
    return NMRFIT_OK;
}

int scatter_grid(nmrfit_ctx *ctx, const double *d_src, double *d_dst)
{
    const int64_t N = ctx->N;
    hipLaunchKernelGGL(scatter_grid_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, ctx->stream, d_src, N, d_dst);
    NMRFIT_HIP(hipGetLastError());
    return NMRFIT_OK;
}

// The kernel variant a launch actually runs (the requested one may not fit in LDS, or may not
// implement the imaginary part) and the dynamic LDS its per-wave records need.
constexpr size_t kStaticLds = kObjectiveStaticLds;   // objective_kernel's own __shared__ (wsums) + alignment slack
static_assert(kObjectiveStaticLds == (size_t)kWsumsCount * sizeof(double) + 64, "objective_launch.h and objective_math.h disagree");
namespace {
struct ResolvedLds {
    int variant;
    size_t lds;
    unsigned aux_off;
};
// Every size is the `end` of the kernel's own layout (objective_lds.h); here is only the fallback rule.
constexpr ResolvedLds resolve_lds(int variant, int32_t P, bool residual, int fit_im, int wpb, int slices, int rows)
{
    // the mixed-precision far-field kernel exists for objective launches without the imaginary channel; everything else
    // of a context set to it runs the fp64 far-field kernel (same records, same LDS)
    const bool want32 = variant == NMRFIT_VARIANT_FARFIELD32;
    if (want32) variant = NMRFIT_VARIANT_FARFIELD;
    const int np = P > 1 ? P : 1;
    // what a workgroup may take of a CU's 160 KiB for the records sized here: everything but the kernel's static
    // LDS and (swarm generations) the per-wave copies of the updated rows that launch_objective appends
    const size_t room = 160 * 1024 - kStaticLds -
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
}  // namespace
// `slices`: copies of the per-peak records in a workgroup (1 when its waves are segments of one particle, else wpb);
// `rows`: copies of the updated row kept for a fused swarm generation (0: none)
size_t objective_lds(int variant, int32_t P, bool residual, int fit_im, int *variant_out, unsigned *aux_off, int wpb,
                     int slices, int rows)
{
    const ResolvedLds r = resolve_lds(variant, P, residual, fit_im, wpb, slices, rows);
    *variant_out = r.variant;
    *aux_off = r.aux_off;
    return r.lds;
}

int launch_objective(nmrfit_ctx *ctx, int64_t S, int32_t P, const double *dX, double *df, double *dR,
                     ObjectiveDeferred *defer, const PsoFused *fused, int rows_fit_im)
{
    if (defer) *defer = ObjectiveDeferred{};
    // residual rows see the real channel alone, except in the one call that asks for both (nmrfit_internal.h)
    const bool rows_im = dR && rows_fit_im != 0;
    if (rows_im && (defer || fused || (rows_fit_im != 1 && rows_fit_im != 2))) {
        set_error("launch_objective: residual rows of both channels take fit_im 1 or 2 and no swarm update");
        return NMRFIT_E_INVALID;
    }
    const int fit_im = rows_im ? rows_fit_im : dR ? 0 : ctx->fit_im;
    if (S == 0) return NMRFIT_OK;
    const int64_t N = ctx->N;
    // Segmenting: a wave is one (particle, segment) task; a segment is a whole number of blocks.  Swarms that already
    // supply enough waves get nseg = 1 and the wave writes f directly.  (Rounds 1-3 aimed at ~16 tasks per SIMD so that
    // the hardware dispatcher load-balances -- C3: 4096 one-per-particle waves 1.81 ms, 16384 waves 1.74 ms; the
    // round-4 rule below replaces it unless NMRFIT_SEG_RULE=3 or an explicit target is set.)
    int64_t target_waves = (int64_t)ctx->compute_units * 4 * 16;
    if (ctx->target_waves > 0) target_waves = ctx->target_waves;
    // Blocks: the unit of the canonical summation / phase re-seeding, a function of N only
    // (at most 16 per grid), so that results do not depend on S or on sharding.
    const BlockPlan bp = block_plan(N);
    const int64_t n_chunks = bp.n_chunks, n_blocks = bp.n_blocks, blk_len = bp.blk_len;
    const int blk_chunks = bp.blk_chunks;
    int64_t nseg = std::max<int64_t>(1, std::min<int64_t>(n_blocks, (target_waves + S - 1) / S));
    static const bool seg_rule_r4 = [] {
        const char *e = getenv("NMRFIT_SEG_RULE");   // A/B knob: 3 = the round-3 rule (~16 tasks per SIMD)
        return !(e && atoi(e) == 3);
    }();
    if (ctx->target_waves == 0 && seg_rule_r4) {
        // Round 4 (the selectable kernels now run four waves per SIMD): as few segments as fill the chip ONCE -- every
        // further segment repeats a wave's prologue and cuts its chunk loop shorter (1024 x 16384 x 12: 16 segments
        // 69 us, 4 segments 60 us; 4096 x 4096 x 6: 4 segments 56 us, 1 segment 49 us) -- but four where a wave then
        // still has 16 chunks or more: the prologue no longer counts there, and four segments make the workgroup
        // the particle (f and the personal best finished in the launch)
        const int64_t slots = (int64_t)ctx->compute_units * 4 * 4;
        nseg = std::max<int64_t>(1, std::min<int64_t>(n_blocks, (slots + S - 1) / S));
        if (n_chunks / 4 >= 16) nseg = std::max<int64_t>(nseg, std::min<int64_t>(4, n_blocks));
    }
    // Short grids: a wave's own prologue (block seeds, pointers, the barrier of the shared part) still
    // costs a good fraction of a chunk, so prefer >= 2 chunks per wave as long as two waves per SIMD
    // remain (measured on C2, S=1024 N=4096, with the per-workgroup prologue: 8 segments 25.0 us,
    // 4 segments 22.7 us, 2 segments 23.3 us; round 1, prologue per wave: 8 -> 26.2, 2 -> 22.2).
    if (ctx->target_waves == 0) {
        const int64_t simds = (int64_t)ctx->compute_units * 4;
        while (nseg > 1 && n_chunks / nseg < 2 && S * ((nseg + 1) / 2) >= 2 * simds) nseg = (nseg + 1) / 2;
        // a small swarm whose waves just miss fitting on the chip at once (three per SIMD) while half
        // as many would leave it well filled: take the half (204 x 16384 x 12: 16 segments 30.4 us per
        // generation, 8 segments 28.5; tools/archive/nseg_generation_ab.py)
        if (nseg > 1 && S * nseg > 3 * simds && S * (nseg / 2) < 2 * simds && n_chunks / nseg <= 2) nseg /= 2;
    }
    int64_t seg_len = ((n_blocks + nseg - 1) / nseg) * blk_len;
    nseg = (N + seg_len - 1) / seg_len;
    const int64_t waves = S * nseg;
    int variant = NMRFIT_VARIANT_DEFAULT;
    unsigned aux_off = 0;
    const bool fused_rows = fused && fused->x_in;
    // LDS copies: per-peak records once per workgroup when its waves are segments of ONE particle (nseg a multiple of
    // the waves per workgroup), else once per wave; the updated row of a fused swarm generation likewise, plus two
    // more rows (g, the winner's row) when the workgroup may finish the generation (objective.hip, personal_best)
    // swarms the two whole-generation forms of a fused launch take (PsoFused::tail), by waves per workgroup
    auto tail_fits = [&](unsigned tail, int w) {
        return tail != 0u && S <= (int64_t)kDeferredPerLane * kWave * w;
    };
    auto copies = [&](int w, int *slices, int *rows) {
        const bool one_particle = (nseg % w == 0);   // (objective_body: `shared`)
        *slices = one_particle ? 1 : w;
        *rows = !fused_rows ? 0 : !one_particle ? w : (nseg == w && tail_fits(fused->tail, w)) ? 3 : 1;
    };
    int wpb = kWavesPerBlock, slices = 0, rows = 0;
    copies(wpb, &slices, &rows);
    size_t lds = objective_lds(ctx->variant, P, dR != nullptr, fit_im, &variant, &aux_off, wpb, slices, rows);
    // (the context's own variant too: a FARFIELD context whose records no longer fit resolves to DEFAULT above)
    if (rows_im && (variant != NMRFIT_VARIANT_DEFAULT || ctx->variant != NMRFIT_VARIANT_DEFAULT)) {
        set_error("residual rows with the imaginary channel exist for the DEFAULT kernel variant only (and while its LDS records fit)");
        return NMRFIT_E_UNSUPPORTED;
    }
    // Eight segments per particle (small swarms on short grids -- the reference's default 204 x 4096): an EIGHT-wave
    // workgroup is the particle, as the four-wave workgroup is for four segments: one prologue per particle, block
    // sums through LDS, f (and, in a swarm generation, the personal best) finished in this launch.
    const size_t xrow_bytes = fused_rows ? (size_t)(4 + 3 * (int64_t)P) * sizeof(double) : 0;
    if (nseg == kWideWaves && !dR && fit_im == 0 && has_eight_wave_form(variant) && ctx->wide_workgroups) {
        int v8 = variant, s8 = 0, r8 = 0;
        unsigned aux8 = 0;
        copies(kWideWaves, &s8, &r8);
        const size_t lds8 = objective_lds(ctx->variant, P, false, fit_im, &v8, &aux8, kWideWaves, s8, r8);
        if (v8 == variant && lds8 + kStaticLds + 16 + (size_t)r8 * xrow_bytes <= 160 * 1024) {
            wpb = kWideWaves;
            slices = s8;
            rows = r8;
            lds = lds8;
            aux_off = aux8;
        }
    }
    // The pair form (objective_pair.h): a four-wave workgroup is TWO particles cut into four segments, and a wave fetches
    // every chunk of the grid once for both.  For objective launches of the DEFAULT kernel whose pairs still fill the
    // chip's four-waves-per-SIMD slots once (smaller swarms keep a workgroup per particle: more of them to spread);
    // NMRFIT_PAIR_WAVES=0 / 1: never / wherever the geometry allows (A/B knob, nmrfit_ctx::pair_waves).
    bool pair = false;
    if (variant == NMRFIT_VARIANT_DEFAULT && !dR && fit_im == 0 && nseg == kWavesPerBlock && wpb == kWavesPerBlock &&
        ctx->pair_waves != 0 && (ctx->pair_waves > 0 || (S / 2) * kWavesPerBlock >= (int64_t)ctx->compute_units * 4 * 4)) {
        const size_t lds2 = objective_pair_lds_layout(P > 1 ? P : 1).end;
        if (lds2 + kPairStaticLds + 16 + (size_t)kPairParticles * rows * xrow_bytes <= 160 * 1024) {
            pair = true;
            lds = lds2;
            rows *= kPairParticles;
            aux_off = 0;
        }
    }
    const size_t static_lds = pair ? kPairStaticLds : kStaticLds;
    const int64_t blocks = pair ? (S + 1) / 2 : (waves + wpb - 1) / wpb;
    if (blocks > 0x7fffffffLL) {
        set_error("swarm too large for one launch");
        return NMRFIT_E_INVALID;
    }
    if (lds + static_lds + 16 + (size_t)rows * xrow_bytes > 160 * 1024) {
        set_error("too many peaks for the kernel's LDS records (with the imaginary model / the fused swarm update)");
        return NMRFIT_E_UNSUPPORTED;
    }
    // fused swarm update: one copy of the particle's updated row per wave, after everything else
    PsoFused upd{};
    if (fused && fused->x_in) {
        if (dR || (4 + 3 * (int64_t)P) > kFusedMaxD) {
            set_error("fused swarm update: objective launches with D <= kFusedMaxD only");
            return NMRFIT_E_INVALID;
        }
        upd = *fused;
        lds = (lds + 15) & ~(size_t)15;
        upd.xrow_off = (unsigned)lds;
        lds += (size_t)rows * (size_t)(4 + 3 * (int64_t)P) * sizeof(double);
    }
    // nseg == 1: the wave writes f; nseg == 4 (or 8, wide form): the waves of a workgroup are the particle's
    // segments and the workgroup writes f (block sums through LDS); otherwise per-block sums go to a
    // buffer and finalize_kernel (or the swarm's select kernel) adds them.  Same summation order in all.
    const bool direct_f = (nseg == 1 || nseg == wpb);
    if (nseg != wpb) upd.pbest = 0u;   // (only when ONE workgroup holds the whole particle; else the caller's kernel)
    if (upd.pbest == 0u || !tail_fits(upd.tail, wpb)) upd.tail = 0u;   // (the whole generation in this launch: only on top of the personal bests)
    if (fused && fused->tail != 0u && fused->pending != 0u && upd.tail == 0u) {
        // a generation waits to be folded and this launch cannot do it (the variant or fit_im changed between two
        // generations): nothing is launched, the caller folds in a launch of its own and comes back
        if (!defer) {
            set_error("launch_objective: pending fold without a deferred-launch record");
            return NMRFIT_E_STATE;
        }
        defer->need_flush = true;
        return NMRFIT_OK;
    }
    double *out = df;
    if (!direct_f) {
        int rc = ensure(ctx, &ctx->d_partial, &ctx->cap_partial, S * n_blocks * (fit_im ? 2 : 1));
        if (rc != NMRFIT_OK) return rc;
        out = ctx->d_partial;
    }
    ObjectiveLaunch la{};
    la.ctx = ctx;
    la.S = S;
    la.P = P;
    la.dX = dX;
    la.out = out;
    la.dR = dR;
    la.nseg = (int)nseg;
    la.seg_len = seg_len;
    la.blk_chunks = blk_chunks;
    la.seg_blocks = (int)(seg_len / blk_len);
    la.n_blocks = (int)n_blocks;
    la.blocks = blocks;
    la.lds = lds;
    la.fit_im = fit_im;
    la.upd = upd;
    la.aux_off = aux_off;
    la.wpb = wpb;
    la.pair = pair;
    int rc;
    if (rows_im) {
        rc = launch_objective_rows_im(la);
        if (rc != NMRFIT_OK) return rc;
        if (!direct_f) {
            hipLaunchKernelGGL(finalize_rows_im_kernel, dim3((unsigned)((S + 255) / 256)), dim3(256), 0, ctx->stream,
                               ctx->d_partial, S, n_blocks, N, df);
            NMRFIT_HIP(hipGetLastError());
        }
        ctx->last.waves = waves;
        ctx->last.waves_per_workgroup = wpb;
        ctx->last.nseg = (int32_t)nseg;
        ctx->last.seg_len = seg_len;
        return NMRFIT_OK;
    }
    switch (variant) {   // one translation unit per selectable variant (they compile in parallel)
        case NMRFIT_VARIANT_DEFAULT: rc = pair ? launch_objective_pair(la) : launch_objective_default(la); break;
        case NMRFIT_VARIANT_FARFIELD: rc = launch_objective_farfield(la); break;
        case NMRFIT_VARIANT_FARFIELD32: rc = launch_objective_farfield32(la); break;
        case NMRFIT_VARIANT_NOREC: rc = launch_objective_norec(la); break;
        default:
#ifdef NMRFIT_AB_BUILD
            rc = launch_objective_ab(variant, la);
#else
            set_error("this kernel variant exists in A/B builds of the library only (-DNMRFIT_AB_BUILD)");
            rc = NMRFIT_E_UNSUPPORTED;
#endif
            break;
    }
    if (rc != NMRFIT_OK) return rc;
    if (defer) defer->pbest_done = upd.x_in != nullptr && upd.pbest != 0u;
    if (defer) defer->tail_done = defer->pbest_done && upd.tail != 0u;
    if (!direct_f && defer) {   // the caller's own kernel adds the per-block sums (pso_tail_kernel)
        defer->needed = true;
        defer->partial = ctx->d_partial;
        defer->n_blocks = n_blocks;
        defer->fit_im = fit_im;
    } else if (!direct_f) {
        hipLaunchKernelGGL(finalize_kernel, dim3((unsigned)((S + 255) / 256)), dim3(256), 0, ctx->stream,
                           ctx->d_partial, S, n_blocks, N, fit_im, df);
        NMRFIT_HIP(hipGetLastError());
    }
    ctx->last.waves = pair ? blocks * wpb : waves;   // (the pair form: a wave holds a segment of two particles)
    ctx->last.waves_per_workgroup = wpb;
    ctx->last.nseg = (int32_t)nseg;
    ctx->last.seg_len = seg_len;
    return NMRFIT_OK;
}

}  // namespace nmrfit

// objective_kernel.h -- the hot path: the batched nmrfit objective / residual kernel for gfx950 (CDNA4), a template over
// (kernel variant, residual rows, imaginary-channel mode, waves per workgroup).  objective_body reads top to bottom: carve
// the dynamic LDS (objective_lds.h: the layout the host sizes the launch with), locate the particle and segment, prologue
// (objective_prologue.h), chunk loop (objective_chunk_stages.h on objective_farfield.h and objective_chunk.h), finish
// (objective_finish.h).  Instantiated by objective_default.hip /
// objective_farfield.hip / objective_norec.hip -- the variants nmrfit_amd.fit() can select -- and, in -DNMRFIT_AB_BUILD
// builds only, by objective_ab.hip (the A/B forms); launched through objective.hip (launch_objective).
//
// What it computes (reference: nmrfit/equations.py:152-212 `objective`, :115-149 `voigt`,
// nmrfit/proc_autophase.py:9-36 `ps2`), for every particle i of a swarm X[S, 4+3P]:
//
//     phi_j   = p0 + (p1*j)/N                                    proc_autophase.py:31
//     Vd_j    = cos(phi_j)*u_j - sin(phi_j)*v_j                  proc_autophase.py:35 (real part)
//     Vf_j    = sum_k [ yoff + a_k*( r*L_k(w_j) + (1-r)*G_k(w_j) ) ]   equations.py:141-147,195
//     f_i     = sqrt( mean_j ( weights_j*(Vd_j - Vf_j) )^2 )     equations.py:202
//
// MI355X mapping (no MFMA: there is no contraction here; the kernel is bound by the fp64
// vector-ALU issue rate):
//   * one WAVE owns one (particle, grid-segment); its 64 lanes stride the grid points so
//     the w/u/v/weights reads are coalesced 512-B rows that stay L2-resident (the four
//     arrays are shared by every particle: <= 2 MiB at N = 65536);
//   * each lane register-blocks 8 grid points, so the per-peak constants are fetched once
//     per 8 points.  They are wave-uniform and live in LDS (48 B per peak; the main loop
//     reads 24 B of it with broadcast ds_reads), staged once per wave from the particle's
//     row of X;
//   * algebra (derived from equations.py:141-147, exact in real arithmetic): with
//     t = (w-loc)*(2/width), s = 1 + t^2:  L = (2/(pi*width))/s  and
//     exp(-((w-loc)/(width/(2 sqrt(ln2))))^2) = 2^(-t^2) = 2*2^(-s), so one fma chain per
//     point and peak: t = fma(wc, ihw, c); s = fma(t, t, 1); acc += AL*rcp(s) + AG2*exp2(-s);
//   * the Lorentzians of eight peaks share one reciprocal (common denominator, combined up
//     a binary tree of (numerator, denominator) pairs); rcp: v_rcp_f64 + one Newton step
//     (relative error 2.2e-15);
//     exp2(-s): round-to-nearest split + degree-11 polynomial + v_ldexp_f64 (<= 3e-16);
//   * the Gaussian term is < 2^-64 of its amplitude once |w-loc| > 3.97*width; a wave
//     skips it for a whole 512-point chunk when the chunk's [min,max] of w (precomputed
//     at context creation) misses that window -- a wave-uniform branch, exact to fp64
//     rounding, and the common case (a line is ~100x narrower than the spectrum);
//   * the phase ramp is a complex rotation recurrence z <- z*rho (4 fp64 ops per point),
//     re-seeded at the start of each of <= 16 blocks of the grid;
//   * sum of squares: per-lane fp64 accumulation over a block, then a wave64 shuffle tree.
//     With one segment per particle the wave writes f directly; otherwise a tiny second
//     kernel adds the per-block sums in grid order (deterministic, no atomics, and the same
//     order whatever the segmentation: f does not depend on launch geometry or on sharding).
#pragma once
#include "objective_chunk_stages.h"
#include "objective_finish.h"
#include "objective_launch.h"
#include "objective_lds.h"
#include "objective_prologue.h"
#include "swarm_prologue.h"

namespace nmrfit {
namespace {

// ---- the kernel ----------------------------------------------------------------------------
// VARIANT: NMRFIT_VARIANT_DEFAULT  8 Lorentzians per reciprocal + Gaussian window skip (+ on uniform
//                                  grids the Gaussian recurrence, objective launches only)
//          NMRFIT_VARIANT_NOREC    the same without the recurrence
//          NMRFIT_VARIANT_BASELINE IEEE divide and libdevice exp2 per unit, no skip: the
//                                  obviously-right form the tuned ones are A/B-checked against
//          NMRFIT_VARIANT_NOSKIP   8 per reciprocal, Gaussian evaluated everywhere
//          NMRFIT_VARIANT_FARFIELD Lorentzian tails of distant peaks through a shared Taylor
//                                  expansion per chunk (opt-in; objective_farfield.h)
// Wave g = blockIdx.x*4 + wave  ->  particle g / nseg, segment g % nseg;
// a segment is seg_len (multiple of 512) consecutive grid points.
// FIT_IM: 0 real part only (reference default); 1 reference-compatible fit_im=True -- the
// imaginary model is the LAST peak's dispersion only, because equations.py:199 assigns
// instead of accumulating; 2 the imaginary model is the sum over all peaks.
// WRITE_R with FIT_IM != 0 (objective_rows_im.hip, DEFAULT only; include/nmrfit_amd_lsq_im.h): the imaginary residual
// ei = weights*(Id - If) is stored next to e, in a second plane of R_out ([2][S][N]), and `out` receives the two RMSEs of
// every row ([S][2]) instead of their mean -- in all three geometries (one segment, workgroup = particle, partial sums +
// finalize_rows_im_kernel).  Every statement of it sits under `if constexpr (WRITE_R && FIT_IM != 0)`: the other
// instantiations compile to what they compiled to before.  Residual launches with FIT_IM of the other variants are
// refused (NMRFIT_E_UNSUPPORTED).
// Registers and occupancy of the selectable kernels (tools/kernel_resources.py, checked by
// tests/test_kernel_resources_cpu.py; figures of the round-6 build): the headline objective kernel <DEFAULT, real part
// only, four waves per workgroup> 127 VGPRs -- FOUR waves per SIMD, no scratch -- with the 8-peak group's 24 constants,
// the 8-point register block and the batch inversion's intermediates live together; FARFIELD 119.
// FIT_IM == 1 evaluates the last peak's dispersion line at the chunk's points in the epilogue (dispersion_points, Dawson
// coefficients from LDS): three waves per SIMD (DEFAULT 131 VGPRs, FARFIELD 142).  FIT_IM == 2 holds eight more
// accumulators and the imaginary far-field sums: the direct kernel 156 VGPRs, the far-field one 162 -- three waves per
// SIMD both, no scratch (round 6: up to round 5 the far-field kernel took the general expansion path with the imaginary
// sum, 190 VGPRs and two waves; it now makes the expansions of two chunks at once there too, real and imaginary).
// Launch bounds (waves per SIMD the compiler must leave room for), by variant and imaginary-channel mode: the direct
// kernels with the imaginary sum run at three waves per SIMD with the bound left at two -- asked for three the compiler
// stops at 160 registers and schedules worse (2.86 against 2.57 ms at C3, round 4); the far-field kernels with the
// imaginary channel keep the bound at two as well (they reach three by themselves: asked for three, the all-peak form
// is 2.32 instead of 2.04 ms).
#ifndef NMRFIT_IM2_FAR_WAVES
#define NMRFIT_IM2_FAR_WAVES 2   // (A/B knob)
#endif
constexpr int objective_min_waves(int variant, int fit_im)
{
    const bool tuned = variant == NMRFIT_VARIANT_DEFAULT || variant == NMRFIT_VARIANT_NOSKIP || is_farfield(variant) || variant == NMRFIT_VARIANT_NOREC;
    return (fit_im == 2 && is_farfield(variant)) ? NMRFIT_IM2_FAR_WAVES : (fit_im != 0 && is_farfield(variant)) ? 2 : (fit_im == 2) ? 2 : tuned ? kMinWaves : 4;
}
// WAVE_SWARM (device-batched fits, objective_batch.hip): every WAVE holds a whole particle (one segment) and does
// the particle's whole swarm step by itself -- deferred fold, update, evaluation, personal best (swarm_prologue.h).
// pblock: the particle of this workgroup when its waves are the particle's segments (blockIdx.x in a plain launch).
template <int VARIANT, bool WRITE_R, int FIT_IM, int WPB, bool WAVE_SWARM = false>
__device__ __forceinline__ void objective_body(
    unsigned char *lds_raw, const int64_t g, const int64_t pblock,
    const double *__restrict__ wc, const double *__restrict__ u, const double *__restrict__ v,
    const double *__restrict__ wt, const double2 *__restrict__ chunk_minmax,
    const double *__restrict__ X, int64_t S, int P, int64_t N, double w0, double wspan, int nseg,
    int64_t seg_len, int blk_chunks, int seg_blocks /* blocks per segment */, int n_blocks_i /* blocks per grid */,
    double lane_step, double rec_devk,
    double *__restrict__ out,       // nseg == 1: f[S];  else per-block sums [S * n_blocks] (x2 with FIT_IM)
                                    // (WRITE_R with FIT_IM: the two RMSEs of every row, [S][2], where f would go)
    double *__restrict__ R_out,     // WRITE_R: residual rows [S*N] (with FIT_IM: [2][S*N], the imaginary rows second)
    unsigned long long *__restrict__ clk,   // profiling only (else null): shader / reference clock of workgroup 0
    const PsoFused &upd,            // swarm generations: advance the particle first (x_in != null), X is then unused
    const unsigned aux_off,         // FIT_IM != 0: byte offset of the Dawson table in dynamic LDS
    double *wsums)                  // [2 * kMaxBlocks] in LDS: the particle's block sums when one workgroup owns it
{
    // WPB: waves per workgroup = LDS slices.  Four (one per SIMD of a CU) everywhere except for particles cut into
    // EIGHT segments (small swarms on short grids: the reference's default 204 particles x 4096 points), where an
    // eight-wave workgroup holds the whole particle: one prologue, f and the personal best finished in this launch.
    const int lane = threadIdx.x & (kWave - 1);
    // (the wave index through v_readfirstlane: the compiler then KNOWS that everything derived from it -- particle,
    // segment, chunk bases, the chunk table's address -- is wave-uniform, keeps it in scalar registers and fetches the
    // chunk table with scalar loads instead of a vector load on the critical path at the top of every chunk)
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    // When every wave of the workgroup evaluates a segment of the SAME particle (nseg a multiple of
    // the waves per workgroup) the particle's prologue is done once per workgroup instead of once
    // per wave: one copy of the per-peak records (slice 0), the position update by wave 0, the
    // per-peak constants by the waves in turn (64 peaks a pass), the phase seeds by the last wave --
    // and a workgroup barrier.  For a short grid the prologue is as long as a chunk or two, so this
    // is what makes four or eight segments per particle affordable (C2: 17.7 -> see DESIGN.md).
    const bool shared = (nseg % WPB == 0);
    const int slice = shared ? 0 : wave;
    // (one copy of every per-peak record per workgroup when its waves share a particle, else one per wave: the
    // dynamic LDS is sized accordingly by objective_lds() -- at C3 that is what lets a fourth workgroup onto a CU)
    const int nslices = shared ? 1 : WPB;
    // Every pointer into the dynamic LDS comes from the one layout the host sizes the launch with (objective_lds.h):
    // the first piece at the area's start, every later one a step from the piece before it.  (Steps, and `lor` ahead of
    // the layout, because the order in which these addresses are formed shows in the kernels' instruction streams.)
    PeakLor *lor = reinterpret_cast<PeakLor *>(lds_raw + ObjectiveLds::lor) + (size_t)slice * P;
    const ObjectiveLds at = objective_lds_layout(VARIANT, WRITE_R, FIT_IM, P, WPB, nslices);
    PeakWin *win = reinterpret_cast<PeakWin *>(lds_raw + at.win) + (size_t)slice * P;
    unsigned char *const seeds_at = lds_raw + at.seeds, *const shr_at = seeds_at + (at.shr - at.seeds),
                        *const lseed_at = shr_at + (at.lseed - at.shr);
    double2 *seeds = reinterpret_cast<double2 *>(seeds_at) + (size_t)wave * kMaxBlocks;
    double *shr = reinterpret_cast<double *>(shr_at);   // rho, L_lane[64] re / im
    int *sflag = reinterpret_cast<int *>(shr + 2 + 2 * kWave);     // one per wave
    // per-lane phase seeds L_lane: in `shr` when the workgroup is one particle, else one copy per wave right behind
    // it; read back at the start of every block instead of living in four VGPRs across the chunk loop
    double *lseed = shared ? shr + 2 : reinterpret_cast<double *>(lseed_at) + (size_t)wave * (2 * kWave);
    // FARFIELD: per-wave scratch [kFarTerms][kFarPad] for the cross-peak coefficient sums
    unsigned char *const far_at = lseed_at + (at.far - at.lseed), *const grec_at = far_at + (at.grec - at.far);
    double *ffs = reinterpret_cast<double *>(far_at) + (size_t)wave * far_stride(FIT_IM);
    // FIT_IM == 2: where the even chunk of a pair parks the odd chunk's 16 coefficient sums (expand_sums).  Without the
    // imaginary sum they wait in slots 16..31 of the scratch's first row; the all-peak imaginary pass uses every row of
    // the scratch for its own expansions, so there they wait in a row of their own behind it.
    // (at ffs + kFarTerms * kFarPad)

    // objective launches of DEFAULT / FARFIELD: per-peak (d, C) of the Gaussian recurrence, after
    // everything else (residual rows are evaluated point by point: they feed finite differences)
    constexpr bool kRec = !WRITE_R && (VARIANT == NMRFIT_VARIANT_DEFAULT || is_farfield(VARIANT));
    double2 *grec = reinterpret_cast<double2 *>(grec_at) + (size_t)slice * P;

    // DEFAULT: scaled Lorentzian constants for the two-operation pair form, after grec
    constexpr bool kFast = (VARIANT == NMRFIT_VARIANT_DEFAULT);
    PeakFast *lorf = reinterpret_cast<PeakFast *>(grec_at + (at.lorf - at.grec)) + (size_t)slice * P;

    // FIT_IM != 0: Dawson table (64 quarter intervals x 11 coefficients for the gathered evaluation, then the 12 of the
    // asymptotic series), one copy per workgroup; the barrier after the staging below makes it visible
    double *dtab = reinterpret_cast<double *>(lds_raw + aux_off);
    if constexpr (FIT_IM != 0)   // kTab[64][11], then kFar[12]
        for (int i = threadIdx.x; i < kDawTabCount; i += WPB * kWave)
            dtab[i] = (i < kDawTabFar) ? (&dawson::kTab[0][0])[i] : dawson::kFar[i - kDawTabFar];
    phase_stamp(clk, 0);
    if (clk && g == 0 && lane == 0) {   // nmrfit_prof_*: ticks of the core clock and of the 100 MHz reference
        clk[0] = __builtin_amdgcn_s_memtime();
        clk[1] = __builtin_amdgcn_s_memrealtime();
    }
    // (no 64-bit division on the way: the GPU has none, a software one is ~80 instructions on the critical path of a
    // wave that may have a single chunk to work on -- the two geometries swarm generations use need none, and the
    // block arithmetic below works from host-computed counts, seg_blocks and n_blocks)
    const bool active = g < S * nseg;
    int64_t particle = 0;
    int seg = 0;
    if (active) {
        if (nseg == 1) {
            particle = g;
        } else if (nseg == WPB) {   // the workgroup is the particle, its waves the segments
            particle = pblock;
            seg = wave;
        } else {
            particle = g / nseg;
            seg = (int)(g - particle * nseg);
        }
    }
    const int64_t D = 4 + 3 * (int64_t)P;
    double p0, p1, r, yoff;
    bool fast_bad = false, rec_bad = false;
    // the particle's per-peak constants into the wave's LDS slices (objective_prologue.h)
    const StagePeakConstants<kFast, kRec> stage_peaks{p0, p1, r, yoff, P, lane, w0, wspan, lor, win, fast_bad, lorf, lane_step, rec_devk, rec_bad, grec};
    bool fused = false;
    if constexpr (!WRITE_R) fused = upd.x_in != nullptr;
    // (the row is staged from global memory or from LDS by two separate calls: one pointer that may
    // be either makes this compiler's address-space inference crash, and would cost flat loads)
    // (WAVE_SWARM: three rows per wave -- the new position, g, the old personal best -- and the old fp behind them)
    double *const xrow = reinterpret_cast<double *>(lds_raw + upd.xrow_off) + (size_t)slice * (WAVE_SWARM ? 3 * D + 2 : D);
    auto stage_row = [&](const int first_pass, const int pass_stride) {
        if (fused)
            stage_peaks(xrow, first_pass, pass_stride);
        else
            stage_peaks(X + particle * D, first_pass, pass_stride);
    };
    if (fused) {
        // swarm generation: the particle moves HERE, in the prologue of the kernel that evaluates it (swarm_prologue.h)
        if constexpr (WAVE_SWARM) {
            if (swarm_prologue_wave(upd, xrow, D, S, particle, active, lane)) return;
        } else {
            if (swarm_prologue<WPB>(upd, xrow, D, S, particle, seg, active, shared, wave, lane, wsums, clk)) return;
        }
    }
    double rr = 1.0, ri = 0.0;   // rotation step exp(i p1 64/N) (the lane seeds exp(i (p0 + p1 lane/N)): lseed, in LDS)
    const double invN = 1.0 / (double)N;
    bool fast_all, rec_all;
    if (shared) {
        stage_row(wave, WPB);                          // wave w: peaks 64w..64w+63, 64(w+WPB).., usually wave 0 alone
        if (wave == WPB - 1) {                         // meanwhile the last wave makes the phase seeds
            double sr, si, tr, ti;
            sincos_fast((p1 * 64.0) * invN, &si, &sr);
            sincos_fast(p0 + (p1 * (double)lane) * invN, &ti, &tr);
            if (lane == 0) {
                shr[0] = sr;
                shr[1] = si;
            }
            shr[2 + lane] = tr;
            shr[2 + kWave + lane] = ti;
        }
        const int fl = (__ballot(fast_bad) != 0ull ? 1 : 0) | (__ballot(rec_bad) != 0ull ? 2 : 0);
        if (lane == 0) sflag[wave] = fl;
        __syncthreads();
        int all = 0;
#pragma unroll
        for (int w2 = 0; w2 < WPB; ++w2) all |= sflag[w2];
        fast_all = kFast && !(all & 1);
        rec_all = kRec && !(all & 2);
        rr = wave_uniform(shr[0]);
        ri = wave_uniform(shr[1]);
    } else {
        stage_row(0, 1);
        // wave-uniform: every group of this particle may take the two-operation pair form
        fast_all = kFast && (__ballot(fast_bad) == 0ull);
        rec_all = kRec && (__ballot(rec_bad) == 0ull);   // every peak may take the Gaussian recurrence
        __syncthreads();
    }
    if (!active) return;
    phase_stamp(clk, 2);   // per-peak constants and phase seeds staged

    const int64_t j0 = (int64_t)seg * seg_len;
    const int64_t j1 = (j0 + seg_len < N) ? j0 + seg_len : N;
    const int64_t n_chunks = (N + kChunk - 1) / kChunk;

    // phase ramp: z = exp(i*phi_j) for this lane's current point, rho = exp(i*p1*64/N)
    // z is re-seeded at the start of every block of blk_chunks chunks as E_b * L_lane with
    // E_b = exp(i*p1*(b*blk_len)/N) (wave-uniform, tabulated in LDS for this segment's blocks)
    // and L_lane = exp(i*(p0 + p1*lane/N)): both depend on the GLOBAL block index and the lane
    // only, never on where the segment starts.
    double zr = 1.0, zi = 0.0;
    const int64_t blk_len = (int64_t)blk_chunks * kChunk;
    if (!shared) {   // (shared prologue: made once per workgroup above; the rotation step comes with the block seeds below)
        double lr, li;
        sincos_fast(p0 + (p1 * (double)lane) * invN, &li, &lr);
        lseed[lane] = lr;
        lseed[kWave + lane] = li;
    }
    {
        const int64_t n_blocks = n_blocks_i;
        const int64_t b0 = (int64_t)seg * seg_blocks;
        const int64_t nb = (seg_blocks < n_blocks - b0) ? seg_blocks : n_blocks - b0;   // blocks of [j0, j1)
        if (shared) {
            if (lane < nb) {
                double er, ei;
                sincos_fast((p1 * (double)((b0 + lane) * blk_len)) * invN, &ei, &er);
                seeds[lane] = make_double2(er, ei);
            }
        } else {
            // ... and, one particle per wave, the rotation step exp(i p1 64/N) in the same call: lane nb (<= 16) takes it.
            // The same function of the same argument as a call of its own: the same bits.
            const double m = (lane < nb) ? (double)((b0 + lane) * blk_len) : 64.0;
            double er, ei;
            sincos_fast((p1 * m) * invN, &ei, &er);
            if (lane < nb) seeds[lane] = make_double2(er, ei);
            const int rl = (nb > 0) ? (int)nb : 0;   // (a segment without blocks: every lane took the step)
            rr = __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(er), rl), __builtin_amdgcn_readlane(__double2loint(er), rl));
            ri = __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(ei), rl), __builtin_amdgcn_readlane(__double2loint(ei), rl));
        }
        wave_lds_fence();   // same-wave LDS write -> read
    }
    const int64_t n_blocks = n_blocks_i;
    double bs = 0.0, bs_im = 0.0;             // per-lane sums of squares of the current block
    const int64_t blk0 = (int64_t)seg * seg_blocks;   // global index of this segment's first block
    int cib = 0, bidx = 0;                     // chunk within block, block within segment
    const double base = wave_uniform((double)P * yoff);   // yoff is added once per peak (equations.py:147,195)
    double ss = 0.0, ss_im = 0.0;

    unsigned even_near = 0, even_hits = 0;     // FARFIELD, P <= 32: near-peak and Gaussian-window masks of the even ...
    unsigned pend_near = 0, pend_hits = 0;     // ... and of the odd chunk of the current pair (ExpandPair)
    unsigned even_near_im = 0, pend_near_im = 0, pair_far_im = 0;   // FIT_IM == 2, P <= 32: the same for the imaginary model (ExpandPairIm)

    // The chunk loop exists twice, once per Lorentzian group form, chosen ONCE per wave: inside one
    // copy the accumulators never meet the other form's registers (a merge of the two forms per
    // chunk costs the compiler 8-16 register copies per chunk).
    auto chunk_loop = [&](auto fast_tag) {
        constexpr bool kFastLoop = decltype(fast_tag)::value;
        // The stages of a chunk (objective_farfield.h, objective_chunk_stages.h), each bound to this wave's state.
        const ExpandPair expand_pair{chunk_minmax, j1, lane, P, lor, win, ffs, even_near, even_hits, pend_near, pend_hits};
        const ExpandSums<FIT_IM> expand_sums{ffs, lane};
        const ImRows im_rows{ffs, lane};
        const ExpandPairIm<FIT_IM> expand_pair_im{chunk_minmax, j1, lane, P, lor, even_near_im, pend_near_im, pair_far_im, im_rows, expand_sums};
        // ... and the chunk body twice more, for full chunks and for the one ragged chunk at the end of
        // the grid: `full` is a compile-time constant inside, so the predicated and the unpredicated
        // loads never merge (each merge is eight register copies).
        const ObjectiveChunk<VARIANT, WRITE_R, FIT_IM, WPB, kFastLoop> chunk{
            lane, cib, seeds, bidx, lseed, zr, zi, wc, j1, base, P, lor, chunk_minmax, expand_pair, expand_sums,
            pend_near, even_near, pend_hits, even_hits, ffs, rec_all, grec, win, lorf, expand_pair_im,
            pair_far_im, pend_near_im, even_near_im, dtab, im_rows, u, v, wt, bs, bs_im, R_out, S, particle, N,
            rr, ri, blk_chunks, nseg, ss, ss_im, wsums, blk0, out, n_blocks};
        int64_t jb = j0;
        if constexpr (is_farfield(VARIANT)) {   // chunks alternate even / odd from the segment start
            for (; jb + 2 * kChunk <= j1; jb += 2 * kChunk) {
                chunk(jb, std::true_type{}, std::false_type{});
                chunk(jb + kChunk, std::true_type{}, std::true_type{});
            }
            if (jb + kChunk <= j1) {
                chunk(jb, std::true_type{}, std::false_type{});
                jb += kChunk;
                if (jb < j1) chunk(jb, std::false_type{}, std::true_type{});
            } else if (jb < j1) {
                chunk(jb, std::false_type{}, std::false_type{});
            }
        } else {
            for (; jb + kChunk <= j1; jb += kChunk) chunk(jb, std::true_type{}, std::false_type{});
            if (jb < j1) chunk(jb, std::false_type{}, std::false_type{});
        }
    };
    if (kFast && fast_all)
        chunk_loop(std::integral_constant<bool, kFast>{});
    else
        chunk_loop(std::false_type{});

    phase_stamp(clk, 3);   // chunk loop done
    if (clk && g == 0 && lane == 0) {
        clk[2] = __builtin_amdgcn_s_memtime();
        clk[3] = __builtin_amdgcn_s_memrealtime();
    }
    const PersonalBest<WRITE_R> personal_best{wsums, P, pblock, lds_raw, clk};
    if (nseg == 1) {
        const double f = finish_wave<WRITE_R, FIT_IM>(ss, ss_im, N, particle, lane, out);
        // (no fused personal best here in a plain launch: one wave per particle means >= 16384 particles, where the swarm's
        // own select kernels are noise next to the objective -- and the call cost the headline kernel 12 bytes of scratch)
        if constexpr (WAVE_SWARM && !WRITE_R) {   // device-batched fits: the wave finishes its particle's step
            if (fused) personal_best_wave(upd, xrow, D, S, particle, lane, wave_uniform(f));
        }
    }
    if (nseg == WPB && nseg > 1) {
        // One workgroup = one particle (segment = wave): the block sums are added here, in grid order
        // like finalize_value does -- the same canonical order, bit-identical f -- and the launch needs
        // neither the partial-sum buffer nor a finalize pass after it.  (All its waves get here: a
        // workgroup is active or inactive as a whole, and a stopped swarm returned before the loop.)
        __syncthreads();
        if (threadIdx.x == 0) {
            double t = 0.0, ti = 0.0;
            for (int64_t c = 0; c < n_blocks; ++c) {
                t += wsums[c];
                if (FIT_IM != 0) ti += wsums[kMaxBlocks + c];
            }
            const double f = (FIT_IM == 0) ? sqrt(t / (double)N) : 0.5 * (sqrt(t / (double)N) + sqrt(ti / (double)N));
            if constexpr (WRITE_R && FIT_IM != 0) {   // (the same sums, each channel's RMSE on its own)
                out[2 * particle] = sqrt(t / (double)N);
                out[2 * particle + 1] = sqrt(ti / (double)N);
            } else {
                out[particle] = f;
            }
            wsums[2 * kMaxBlocks] = f;
        }
        if constexpr (!WRITE_R) {
            // (wave 0 alone goes on: f travels from its lane 0 through the same LDS word, no second workgroup barrier)
            if ((threadIdx.x >> 6) == 0) {
                wave_lds_fence();
                phase_stamp(clk, 4);   // f known
                personal_best(wsums[2 * kMaxBlocks]);
            }
        }
    }
}

template <int VARIANT, bool WRITE_R, int FIT_IM, int WPB = kWavesPerBlock>
__global__ __launch_bounds__(kWave *WPB, (WPB == kWavesPerBlock) ? objective_min_waves(VARIANT, FIT_IM) : 2) void objective_kernel(
    const double *__restrict__ wc, const double *__restrict__ u, const double *__restrict__ v,
    const double *__restrict__ wt, const double2 *__restrict__ chunk_minmax, const double *__restrict__ X, int64_t S,
    int P, int64_t N, double w0, double wspan, int nseg, int64_t seg_len, int blk_chunks, int seg_blocks, int n_blocks,
    double lane_step, double rec_devk, double *__restrict__ out, double *__restrict__ R_out,
    unsigned long long *__restrict__ clk, const PsoFused upd, const unsigned aux_off)
{
    extern __shared__ __align__(16) unsigned char lds_raw[];
    // block sums (x2 with the imaginary channel); then f; then what the fused personal-best step needs at the very
    // end of the kernel (flag, p, S, the row's LDS offset), parked here by the prologue
    __shared__ double wsums[kWsumsCount];
    if (threadIdx.x == 0) {   // first thing in the kernel, while nothing else is live (a barrier follows the staging)
        const bool pbest = !WRITE_R && upd.x_in != nullptr && upd.pbest != 0u;
        wsums[2 * kMaxBlocks + 1] = pbest ? 1.0 : 0.0;
        wsums[2 * kMaxBlocks + 2] = __longlong_as_double((long long)(uintptr_t)upd.p);
        wsums[2 * kMaxBlocks + 3] = __longlong_as_double((long long)S);
        wsums[2 * kMaxBlocks + 4] = __longlong_as_double((long long)upd.xrow_off);
        // this particle's personal-best value, requested NOW: a memory round trip off the end of the kernel's
        // critical path (nobody else writes it in this launch)
        if (pbest && nseg == WPB) wsums[2 * kMaxBlocks + 5] = upd.p[S * (4 + 3 * (int64_t)P) + blockIdx.x];
        // deferred fold: where the other (p, fp) buffer is (never 0 then) -- read back by the personal-best step
        wsums[2 * kMaxBlocks + 7] = __longlong_as_double((pbest && upd.tail != 0u) ? (long long)upd.pflip : 0LL);
    }
    const int64_t g = (int64_t)blockIdx.x * WPB + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    objective_body<VARIANT, WRITE_R, FIT_IM, WPB>(lds_raw, g, (int64_t)blockIdx.x, wc, u, v, wt, chunk_minmax, X, S, P, N, w0, wspan, nseg, seg_len,
                                             blk_chunks, seg_blocks, n_blocks, lane_step, rec_devk, out, R_out, clk, upd, aux_off, wsums);
}

template <int VARIANT>
int launch_variant(const ObjectiveLaunch &a)
{
    nmrfit_ctx *const ctx = a.ctx;
    const int64_t S = a.S, seg_len = a.seg_len, blocks = a.blocks;
    const int32_t P = a.P;
    const double *const dX = a.dX;
    double *const out = a.out, *const dR = a.dR;
    const int nseg = a.nseg, blk_chunks = a.blk_chunks, fit_im = a.fit_im, wpb = a.wpb;
    const size_t lds = a.lds;
    const PsoFused &upd = a.upd;
    const unsigned aux_off = a.aux_off;
#define NMRFIT_LAUNCH_W(WR, FI, W)                                                                              \
    hipLaunchKernelGGL((objective_kernel<VARIANT, WR, FI, W>), dim3((unsigned)blocks), dim3(kWave *(W)), lds,  \
                       ctx->stream, ctx->d_wc, ctx->d_u, ctx->d_v, ctx->d_wt, ctx->d_chunk, dX, S, (int)P,     \
                       ctx->N, ctx->w0, ctx->wspan, nseg, seg_len, blk_chunks, a.seg_blocks, a.n_blocks,      \
                       ctx->lane_step, ctx->grid_dev * 11.0e10, out, dR, clk, upd, aux_off)
#define NMRFIT_LAUNCH(WR, FI) NMRFIT_LAUNCH_W(WR, FI, kWavesPerBlock)
    // nmrfit_prof_enable: HIP events on the launch stream around this kernel alone
    const bool prof = ctx->prof_cap > 0 && ctx->prof_nk < ctx->prof_cap;
    unsigned long long *clk = prof ? ctx->d_clk : nullptr;
    if (prof) NMRFIT_HIP(hipEventRecord(ctx->prof_k0[(size_t)ctx->prof_nk], ctx->stream));
    if constexpr (VARIANT == NMRFIT_VARIANT_FARFIELD32) {   // (objective launches without the imaginary channel only:
        if (dR || fit_im != 0) {                             // launch_objective sends everything else to FARFIELD)
            set_error("internal: FARFIELD32 launch with residual rows or the imaginary channel");
            return NMRFIT_E_STATE;
        }
        if (wpb == kWideWaves)
            NMRFIT_LAUNCH_W(false, 0, kWideWaves);
        else
            NMRFIT_LAUNCH(false, 0);
    } else if (dR && fit_im != 0) {
        // (residual rows of both channels: objective_rows_im.hip, DEFAULT only; launch_objective never comes here with them)
        set_error("residual rows with the imaginary channel exist for the DEFAULT kernel variant only");
        return NMRFIT_E_UNSUPPORTED;
    } else if (dR) {
        NMRFIT_LAUNCH(true, 0);
    } else if (fit_im == 0) {
        if constexpr (has_eight_wave_form(VARIANT)) {
            if (wpb == kWideWaves)
                NMRFIT_LAUNCH_W(false, 0, kWideWaves);
            else
                NMRFIT_LAUNCH(false, 0);
        } else {
            NMRFIT_LAUNCH(false, 0);
        }
    } else if constexpr (VARIANT == NMRFIT_VARIANT_DEFAULT || VARIANT == NMRFIT_VARIANT_FARFIELD || VARIANT == NMRFIT_VARIANT_NOREC) {
        if (fit_im == 1)
            NMRFIT_LAUNCH(false, 1);
        else
            NMRFIT_LAUNCH(false, 2);
    } else {
        set_error("fit_im is implemented for the DEFAULT, NOREC and FARFIELD kernel variants only");
        return NMRFIT_E_UNSUPPORTED;
    }
#undef NMRFIT_LAUNCH
#undef NMRFIT_LAUNCH_W
    NMRFIT_HIP(hipGetLastError());
    if (prof) {
        NMRFIT_HIP(hipEventRecord(ctx->prof_k1[(size_t)ctx->prof_nk], ctx->stream));
        ++ctx->prof_nk;
    }
    return NMRFIT_OK;
}

}  // namespace
}  // namespace nmrfit

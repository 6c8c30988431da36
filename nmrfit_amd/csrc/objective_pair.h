// objective_pair.h -- the pair form of the DEFAULT objective kernel: a four-wave workgroup is TWO particles (A = 2 *
// workgroup, B = A + 1) and wave s holds segment s of both, so that a wave fetches the four grid arrays of a chunk ONCE
// for two particle-chunks.  Objective launches only: real channel, no residual rows, four segments per particle
// (launch_objective picks it; objective_pair.hip instantiates it).  Every particle's arithmetic is the single form's,
// operation for operation in the same order (objective_chunk_stages.h, the direct form; objective_kernel.h, the
// shared prologue and the workgroup's ending), so every value has the single form's bits.
//
// A chunk: load w; A's model; A's accumulators to LDS (park); B's model; load u, v, weights; B's epilogue; A's accumulators
// back; A's epilogue.  Between its epilogues a particle's per-lane state (phase recurrence, block sum) waits in LDS as
// well: through B's model the wave holds what the single form holds, and fits the same 128 registers.
// A pair of which one particle may not take the scaled Lorentzian form runs its particles one after the other, each in
// its own form, through the same chunk function (nothing is shared on that rare path); a last workgroup without a B
// skips B's stages.
//
// (The model and the epilogue are written out here, not called from ObjectiveChunk: moved into functions that both
// forms call, they change the single form's instruction streams, which tools/isa_hash.py holds to what they were.)
#pragma once
#include "objective_chunk.h"
#include "objective_finish.h"
#include "objective_launch.h"
#include "objective_lds.h"
#include "objective_prologue.h"
#include "swarm_prologue.h"

#include <type_traits>

namespace nmrfit {
namespace {

// One particle's records and per-wave tables in the pair layout.
struct PairSide {
    PeakLor *lor;
    PeakFast *lorf;
    double2 *grec;
    PeakWin *win;
    double2 *seeds;    // this wave's block seeds
    double *shr;       // rotation step, lane seeds (re | im), flags
    double *state;     // this wave's [3][kWave]: zr, zi, bs of every lane
    double *wsums;     // the particle's block sums and parked values
    double base;       // P * yoff
    bool rec_all;
};

// The direct form's model of one particle at the lane's eight points of a chunk (objective_chunk_stages.h: DEFAULT).
template <bool FAST, bool FULL>
__device__ __forceinline__ void pair_model(const PairSide &s, const int P, const int lane, const double2 mm,
                                           const double (&wv)[kPointsPerLane], double (&acc)[kPointsPerLane])
{
    const double base = s.base;
    int k = 0;
    {
        const int kend0 = (P < kWave) ? P : kWave;
        if (kGroupSize <= kend0) {
            if constexpr (FAST)
                lorentz_group_fast<kGroupSize, true>(s.lorf, wv, acc, base);
            else
                lorentz_group<kGroupSize, true>(s.lor, wv, acc, base);
            k = kGroupSize;
        } else if (kend0 > 0) {
            if constexpr (FAST)
                lorentz_tail_fast<true>(kend0, s.lorf, wv, acc, base);
            else
                lorentz_tail<kGroupSize, true>(kend0, s.lor, wv, acc, base);
            k = kend0;
        } else {
#pragma unroll
            for (int q = 0; q < kPointsPerLane; ++q) acc[q] = base;
        }
    }
    for (int kb = 0; kb < P; kb += kWave) {
        const int kend = (P < kb + kWave) ? P : kb + kWave;
        bool h = false;
        if (kb + lane < P) {
            const PeakWin wn = s.win[kb + lane];
            h = (mm.y >= (double)wn.lo) && (mm.x <= (double)wn.hi);
        }
        unsigned long long hits = __ballot(h);
        if (kb != 0) k = kb;
        if constexpr (FAST) {
            for (; k + kGroupSize <= kend; k += kGroupSize) lorentz_group_fast<kGroupSize>(s.lorf + k, wv, acc);
            if (k < kend) lorentz_tail_fast(kend - k, s.lorf + k, wv, acc);
        } else {
            for (; k + kGroupSize <= kend; k += kGroupSize) lorentz_group<kGroupSize>(s.lor + k, wv, acc);
            if (k < kend) lorentz_tail<kGroupSize>(kend - k, s.lor + k, wv, acc);
        }
        if (kend - kb < kWave) hits &= (1ull << (kend - kb)) - 1ull;
        const bool rec = FULL && s.rec_all;
        for (unsigned long long m = rec ? hits : 0ull; m; m &= m - 1) {
            const int k1 = kb + __builtin_ctzll(m);
            gauss_add_rec(s.lor + k1, s.grec + k1, wv, acc);
        }
        for (unsigned long long m = rec ? 0ull : hits; m; m &= m - 1) gauss_add<true>(s.lor + kb + __builtin_ctzll(m), wv, acc);
    }
}

// A particle's per-lane state between its epilogues: the phase recurrence and the block's sum of squares.
struct PairState {
    double zr, zi, bs;
};
__device__ __forceinline__ PairState pair_state(const PairSide &s, const int lane, const bool first, const int bidx)
{
    PairState st;
    if (first) {   // first chunk of a block: the recurrence is re-seeded
        const double2 e = s.seeds[bidx];
        const double lr = s.shr[2 + lane], li = s.shr[2 + kWave + lane];
        st.zr = __builtin_fma(e.x, lr, -(e.y * li));
        st.zi = __builtin_fma(e.x, li, e.y * lr);
    } else {
        st.zr = s.state[lane];
        st.zi = s.state[kWave + lane];
    }
    st.bs = s.state[2 * kWave + lane];
    return st;
}

// ... and its data epilogue: rotation, squared residuals into the block's sum, the block-end reduction into the
// particle's wsums; the state goes back to LDS.
__device__ __forceinline__ void pair_epilogue(const PairSide &s, const int lane, const PairState &st, const bool last, const int slot,
                                              const double (&acc)[kPointsPerLane], const double (&uq)[kPointsPerLane],
                                              const double (&vq)[kPointsPerLane], const double (&tq)[kPointsPerLane])
{
    double zr = st.zr, zi = st.zi, bs = st.bs;
    const double rr = s.shr[0], ri = s.shr[1];   // (the same in every lane; in vector registers for the epilogue's length only)
#pragma unroll
    for (int q = 0; q < kPointsPerLane; ++q) {
        const double vd = __builtin_fma(zr, uq[q], -(zi * vq[q]));
        const double e = tq[q] * (vd - acc[q]);
        bs = __builtin_fma(e, e, bs);
        const double nzr = __builtin_fma(zr, rr, -(zi * ri));
        zi = __builtin_fma(zr, ri, zi * rr);
        zr = nzr;
    }
    if (last) {
        const double cs = wave_sum(bs);
        bs = 0.0;
        if (lane == 0) s.wsums[slot] = cs;
    }
    s.state[lane] = zr;
    s.state[kWave + lane] = zi;
    s.state[2 * kWave + lane] = bs;
}

template <int WPB>
__device__ __forceinline__ void objective_pair_body(
    unsigned char *lds_raw, double *wsums2, const double *__restrict__ wc, const double *__restrict__ u,
    const double *__restrict__ v, const double *__restrict__ wt, const double2 *__restrict__ chunk_minmax,
    const double *__restrict__ X, int64_t S, int P, int64_t N, double w0, double wspan, int64_t seg_len, int blk_chunks,
    int seg_blocks, int n_blocks_i, double lane_step, double rec_devk, double *__restrict__ out,
    unsigned long long *__restrict__ clk, const PsoFused &upd)
{
    static_assert(WPB == kWavesPerBlock, "the pair layout is sized for four-wave workgroups");
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const ObjectivePairLds at = objective_pair_lds_layout(P);
    int64_t part[kPairParticles] = {2 * (int64_t)blockIdx.x, 2 * (int64_t)blockIdx.x + 1};
    const bool hasB = part[1] < S;   // (an odd swarm's last workgroup: no B)
    const int64_t D = 4 + 3 * (int64_t)P;
    const bool fused = upd.x_in != nullptr;
    const int rows = (upd.tail != 0u) ? 3 : 1;   // row copies per particle (launch_objective)
    double *xrow[kPairParticles];
    PairSide side[kPairParticles];
    int *sflag[kPairParticles];
#pragma unroll
    for (int h = 0; h < kPairParticles; ++h) {
        side[h].lor = reinterpret_cast<PeakLor *>(lds_raw + ObjectivePairLds::lor) + (size_t)h * P;
        side[h].lorf = reinterpret_cast<PeakFast *>(lds_raw + at.lorf) + (size_t)h * P;
        side[h].grec = reinterpret_cast<double2 *>(lds_raw + at.grec) + (size_t)h * P;
        side[h].win = reinterpret_cast<PeakWin *>(lds_raw + at.win) + (size_t)h * P;
        side[h].seeds = reinterpret_cast<double2 *>(lds_raw + at.seeds) + ((size_t)h * WPB + wave) * kMaxBlocks;
        side[h].shr = reinterpret_cast<double *>(lds_raw + at.shr + (size_t)h * kSharedPrologueBytes);
        side[h].state = reinterpret_cast<double *>(lds_raw + at.state + (size_t)wave * kPairStateBytes) + (size_t)h * 3 * kWave;
        side[h].wsums = wsums2 + (size_t)h * kWsumsCount;
        sflag[h] = reinterpret_cast<int *>(side[h].shr + 2 + 2 * kWave);
        xrow[h] = reinterpret_cast<double *>(lds_raw + upd.xrow_off) + (size_t)h * rows * D;
    }
    f64x2 *const park = reinterpret_cast<f64x2 *>(lds_raw + at.park + (size_t)wave * kPairParkBytes);
    phase_stamp(clk, 0);
    if (clk && blockIdx.x == 0 && wave == 0 && lane == 0) {
        clk[0] = __builtin_amdgcn_s_memtime();
        clk[1] = __builtin_amdgcn_s_memrealtime();
    }
    if (fused) {
        // the particles move here, one after the other, each with the single form's prologue (a stop is the same for
        // both: B's rows are carried over before anybody returns)
        const bool stopped = swarm_prologue<WPB>(upd, xrow[0], D, S, part[0], wave, true, true, wave, lane, side[0].wsums, clk);
        if (hasB) swarm_prologue<WPB>(upd, xrow[1], D, S, part[1], wave, true, true, wave, lane, side[1].wsums, clk);
        if (stopped) return;
    }
    // per-peak constants and phase seeds: A's by the waves in turn from wave 0 on, its seeds by the last wave; B's
    // from wave 2 on, its seeds by wave 1 -- up to 64 peaks the four jobs have a wave each
    const double invN = 1.0 / (double)N;
    double p1[kPairParticles] = {0.0, 0.0};
#pragma unroll
    for (int h = 0; h < kPairParticles; ++h) {
        if (h == 1 && !hasB) break;
        double p0, r, yoff;
        bool fast_bad = false, rec_bad = false;
        const StagePeakConstants<true, true> stage_peaks{p0, p1[h], r, yoff, P, lane, w0, wspan, side[h].lor, side[h].win, fast_bad,
                                                         side[h].lorf, lane_step, rec_devk, rec_bad, side[h].grec};
        const int turn = (wave + 2 * h) & (WPB - 1);
        if (fused)
            stage_peaks(xrow[h], turn, WPB);
        else
            stage_peaks(X + part[h] * D, turn, WPB);
        if (turn == WPB - 1) {
            double sr, si, tr, ti;
            sincos_fast((p1[h] * 64.0) * invN, &si, &sr);
            sincos_fast(p0 + (p1[h] * (double)lane) * invN, &ti, &tr);
            if (lane == 0) {
                side[h].shr[0] = sr;
                side[h].shr[1] = si;
            }
            side[h].shr[2 + lane] = tr;
            side[h].shr[2 + kWave + lane] = ti;
        }
        const int fl = (__ballot(fast_bad) != 0ull ? 1 : 0) | (__ballot(rec_bad) != 0ull ? 2 : 0);
        if (lane == 0) sflag[h][wave] = fl;
        side[h].base = wave_uniform((double)P * yoff);
    }
    __syncthreads();
    bool fast_all[kPairParticles] = {true, true};
#pragma unroll
    for (int h = 0; h < kPairParticles; ++h) {
        side[h].rec_all = false;
        if (h == 1 && !hasB) break;
        int all = 0;
#pragma unroll
        for (int w2 = 0; w2 < WPB; ++w2) all |= sflag[h][w2];
        fast_all[h] = !(all & 1);
        side[h].rec_all = !(all & 2);
    }
    phase_stamp(clk, 2);

    const int seg = wave;
    const int64_t j0 = (int64_t)seg * seg_len;
    const int64_t j1 = (j0 + seg_len < N) ? j0 + seg_len : N;
    const int64_t blk_len = (int64_t)blk_chunks * kChunk;
    const int64_t n_blocks = n_blocks_i;
    const int64_t b0 = (int64_t)seg * seg_blocks;
    const int64_t nb = (seg_blocks < n_blocks - b0) ? seg_blocks : n_blocks - b0;
#pragma unroll
    for (int h = 0; h < kPairParticles; ++h) {
        if (h == 1 && !hasB) break;
        if (lane < nb) {
            double er, ei;
            sincos_fast((p1[h] * (double)((b0 + lane) * blk_len)) * invN, &ei, &er);
            side[h].seeds[lane] = make_double2(er, ei);
        }
        side[h].state[2 * kWave + lane] = 0.0;   // the block's sum of squares starts empty
    }
    wave_lds_fence();
    const int blk0 = (int)b0;
    int cib = 0, bidx = 0;

    // One chunk for the particles asked for (wave-uniform).  FAST: the Lorentzian form; FULL: all 512 points lie in the grid.
    auto chunk = [&](const int64_t jb, const bool doA, const bool doB, auto fast_tag, auto full_tag) {
        constexpr bool kFastLoop = decltype(fast_tag)::value;
        constexpr bool full = decltype(full_tag)::value;
        const int64_t jl = jb + lane;
        double wv[kPointsPerLane], accA[kPointsPerLane], accB[kPointsPerLane];
        double uq[kPointsPerLane], vq[kPointsPerLane], tq[kPointsPerLane];
        if (full) {
            const global_pairs wp = lane_ptr(wc + jb, lane);
#pragma unroll
            for (int m = 0; m < kPointsPerLane / 2; ++m) {
                const f64x2 d = wp[m * kWave];
                wv[2 * m] = d.x;
                wv[2 * m + 1] = d.y;
            }
        } else {
#pragma unroll
            for (int q = 0; q < kPointsPerLane; ++q)
                wv[q] = (jl + q * kWave < j1) ? wc[jb + (q >> 1) * (2 * kWave) + 2 * lane + (q & 1)] : 0.0;
        }
        const double2 mm = global_table(chunk_minmax, jb / kChunk);
        if (doA) {
            pair_model<kFastLoop, full>(side[0], P, lane, mm, wv, accA);
#pragma unroll
            for (int m = 0; m < kPointsPerLane / 2; ++m) park[m * kWave + lane] = f64x2{accA[2 * m], accA[2 * m + 1]};
        }
        if (doB) pair_model<kFastLoop, full>(side[1], P, lane, mm, wv, accB);
        // keep the u/v/weights loads below the models: hoisted, they would hold 48 VGPRs across them
        asm volatile("" ::: "memory");
        if (full) {
            const global_pairs up = lane_ptr(u + jb, lane), vp = lane_ptr(v + jb, lane), tp = lane_ptr(wt + jb, lane);
#pragma unroll
            for (int m = 0; m < kPointsPerLane / 2; ++m) {
                const f64x2 du = up[m * kWave], dv = vp[m * kWave], dt = tp[m * kWave];
                uq[2 * m] = du.x;
                uq[2 * m + 1] = du.y;
                vq[2 * m] = dv.x;
                vq[2 * m + 1] = dv.y;
                tq[2 * m] = dt.x;
                tq[2 * m + 1] = dt.y;
            }
        } else {
#pragma unroll
            for (int q = 0; q < kPointsPerLane; ++q) {
                const bool ok = jl + q * kWave < j1;
                const int64_t js = jb + (q >> 1) * (2 * kWave) + 2 * lane + (q & 1);
                uq[q] = ok ? u[js] : 0.0;
                vq[q] = ok ? v[js] : 0.0;
                tq[q] = ok ? wt[js] : 0.0;
            }
        }
        const bool first = cib == 0;
        const bool last = (cib + 1 == blk_chunks) || (jb + kChunk >= j1);
        if (doB) pair_epilogue(side[1], lane, pair_state(side[1], lane, first, bidx), last, blk0 + bidx, accB, uq, vq, tq);
        if (doA) {
            // (A's accumulators and state come back AFTER B's epilogue: fetched ahead of it they cost 137 registers,
            // three waves per SIMD -- or, held to four, 60 bytes of scratch)
            wave_lds_fence();
#pragma unroll
            for (int m = 0; m < kPointsPerLane / 2; ++m) {
                const f64x2 d = park[m * kWave + lane];
                accA[2 * m] = d.x;
                accA[2 * m + 1] = d.y;
            }
            pair_epilogue(side[0], lane, pair_state(side[0], lane, first, bidx), last, blk0 + bidx, accA, uq, vq, tq);
        }
        wave_lds_fence();
        ++cib;
        if (last) {
            cib = 0;
            ++bidx;
        }
    };
    auto chunk_loop = [&](const bool doA, const bool doB, auto fast_tag) {
        cib = 0;
        bidx = 0;
        int64_t jb = j0;
        for (; jb + kChunk <= j1; jb += kChunk) chunk(jb, doA, doB, fast_tag, std::true_type{});
        if (jb < j1) chunk(jb, doA, doB, fast_tag, std::false_type{});
    };
    if (fast_all[0] && fast_all[1]) {
        chunk_loop(true, hasB, std::true_type{});
    } else {
        // one of the two may not take the scaled form: one after the other, each in its own form
        if (fast_all[0])
            chunk_loop(true, false, std::true_type{});
        else
            chunk_loop(true, false, std::false_type{});
        if (hasB) {
            if (fast_all[1])
                chunk_loop(false, true, std::true_type{});
            else
                chunk_loop(false, true, std::false_type{});
        }
    }

    phase_stamp(clk, 3);
    if (clk && blockIdx.x == 0 && wave == 0 && lane == 0) {
        clk[2] = __builtin_amdgcn_s_memtime();
        clk[3] = __builtin_amdgcn_s_memrealtime();
    }
    // The ending, once per particle with the single form's code: block sums added in grid order, f, the fused personal
    // best -- A's by wave 0, B's by wave 1.
    __syncthreads();
#pragma unroll
    for (int h = 0; h < kPairParticles; ++h) {
        if (wave != h || (h == 1 && !hasB)) continue;
        double *wsums = side[h].wsums;
        if (lane == 0) {
            double t = 0.0;
            for (int64_t c = 0; c < n_blocks; ++c) t += wsums[c];
            const double f = sqrt(t / (double)N);
            out[part[h]] = f;
            wsums[2 * kMaxBlocks] = f;
        }
        wave_lds_fence();
        phase_stamp(clk, 4);
        const PersonalBest<false> personal_best{wsums, P, part[h], lds_raw, clk};
        personal_best(wsums[2 * kMaxBlocks]);
    }
}

// (The name starts with `objective_kernel`: bench.py and the profiling tools pick the objective launches out of a
// counter trace by that string.)
template <int WPB = kWavesPerBlock>
__global__ __launch_bounds__(kWave *WPB, kMinWaves) void objective_kernel_pair(
    const double *__restrict__ wc, const double *__restrict__ u, const double *__restrict__ v,
    const double *__restrict__ wt, const double2 *__restrict__ chunk_minmax, const double *__restrict__ X, int64_t S,
    int P, int64_t N, double w0, double wspan, int64_t seg_len, int blk_chunks, int seg_blocks, int n_blocks,
    double lane_step, double rec_devk, double *__restrict__ out, unsigned long long *__restrict__ clk, const PsoFused upd)
{
    extern __shared__ __align__(16) unsigned char lds_raw[];
    // per particle: block sums; then f; then what the fused personal-best step needs at the kernel's end (objective_kernel)
    __shared__ double wsums2[kPairParticles * kWsumsCount];
    if (threadIdx.x < kPairParticles) {
        const int h = threadIdx.x;
        double *wsums = wsums2 + h * kWsumsCount;
        const int64_t particle = 2 * (int64_t)blockIdx.x + h;
        const int64_t D = 4 + 3 * (int64_t)P;
        const bool pbest = upd.x_in != nullptr && upd.pbest != 0u;
        wsums[2 * kMaxBlocks + 1] = pbest ? 1.0 : 0.0;
        wsums[2 * kMaxBlocks + 2] = __longlong_as_double((long long)(uintptr_t)upd.p);
        wsums[2 * kMaxBlocks + 3] = __longlong_as_double((long long)S);
        wsums[2 * kMaxBlocks + 4] = __longlong_as_double((long long)(upd.xrow_off + (unsigned)h * (upd.tail != 0u ? 3u : 1u) * (unsigned)(D * sizeof(double))));
        if (pbest && particle < S) wsums[2 * kMaxBlocks + 5] = upd.p[S * D + particle];
        wsums[2 * kMaxBlocks + 7] = __longlong_as_double((pbest && upd.tail != 0u) ? (long long)upd.pflip : 0LL);
    }
    objective_pair_body<WPB>(lds_raw, wsums2, wc, u, v, wt, chunk_minmax, X, S, P, N, w0, wspan, seg_len, blk_chunks, seg_blocks,
                             n_blocks, lane_step, rec_devk, out, clk, upd);
}

}  // namespace
}  // namespace nmrfit

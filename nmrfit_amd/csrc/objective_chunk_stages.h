// objective_chunk_stages.h -- one 512-point chunk of the objective kernel's loop (objective_kernel.h): the model at the
// lane's eight points (direct, far-field or plain form; objective_chunk.h, objective_farfield.h), the imaginary model,
// then the data epilogue -- loads of u, v and weights, rotation, accumulation, row stores, block-end reduction.
// (A struct of references with a call operator: see objective_prologue.h.)
#pragma once
#include "objective_chunk.h"
#include "objective_farfield.h"
#include "objective_launch.h"

namespace nmrfit {
namespace {

// FAST_LOOP: the Lorentzian groups take the two-operation pair form (the chunk loop exists once per form).
template <int VARIANT, bool WRITE_R, int FIT_IM, int WPB, bool FAST_LOOP>
struct ObjectiveChunk {
    static constexpr bool kSkip = (VARIANT != NMRFIT_VARIANT_NOSKIP && VARIANT != NMRFIT_VARIANT_BASELINE);
    static constexpr bool kFar = is_farfield(VARIANT);
    static constexpr bool kRec = !WRITE_R && (VARIANT == NMRFIT_VARIANT_DEFAULT || is_farfield(VARIANT));
    static constexpr bool kFastLoop = FAST_LOOP;
    const int &lane;
    int &cib;
    double2 *&seeds;
    int &bidx;
    double *&lseed;
    double &zr, &zi;          // the phase recurrence: exp(i phi) at the lane's current point
    const double *__restrict__ &wc;
    const int64_t &j1;
    const double &base;
    const int &P;
    PeakLor *&lor;
    const double2 *__restrict__ &chunk_minmax;
    const ExpandPair &expand_pair;
    const ExpandSums<FIT_IM> &expand_sums;
    unsigned &pend_near, &even_near, &pend_hits, &even_hits;
    double *&ffs;
    bool &rec_all;
    double2 *&grec;
    PeakWin *&win;
    PeakFast *&lorf;
    const ExpandPairIm<FIT_IM> &expand_pair_im;
    unsigned &pair_far_im, &pend_near_im, &even_near_im;
    double *&dtab;
    const ImRows &im_rows;
    const double *__restrict__ &u;
    const double *__restrict__ &v;
    const double *__restrict__ &wt;
    double &bs, &bs_im;       // per-lane sums of squares of the current block
    double *__restrict__ &R_out;
    const int64_t &S;
    int64_t &particle;
    const int64_t &N;
    double &rr, &ri;          // the rotation step exp(i p1 64/N)
    const int &blk_chunks;
    const int &nseg;
    double &ss, &ss_im;       // one segment per particle: the sums of the blocks so far
    double *&wsums;
    const int64_t &blk0;
    double *__restrict__ &out;
    const int64_t &n_blocks;
    template <class FULL, class ODD>
    __device__ void operator()(const int64_t jb, FULL, ODD) const
    {
        constexpr bool ff_odd = ODD::value;   // FARFIELD, P <= 32: the second chunk of a pair
        constexpr bool full = FULL::value;    // all 512 points lie inside the segment
        const int64_t jl = jb + lane;
        // A block = blk_chunks consecutive chunks, a function of N only; segments are whole
        // blocks.  Everything that carries state from point to point restarts at block
        // boundaries -- the phase recurrence is re-seeded here, the sums of squares are reduced
        // at the block's end -- so every value, and hence f, is bit-identical for any
        // segmentation of the grid and any sharding of the swarm.
        if (cib == 0) {   // first chunk of a block (segments start on block boundaries)
            const double2 e = seeds[bidx];
            const double lr = lseed[lane], li = lseed[kWave + lane];
            zr = __builtin_fma(e.x, lr, -(e.y * li));
            zi = __builtin_fma(e.x, li, e.y * lr);
        }
        double wv[kPointsPerLane], acc[kPointsPerLane];
        double uq[kPointsPerLane], vq[kPointsPerLane], tq[kPointsPerLane];
        if (full) {
            // (grid_slot order: the lane's points 2m, 2m+1 are one 16-byte pair -> global_load_dwordx4)
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
        // (the accumulators are not set here: whatever touches them first in this chunk starts them from `base`)
        if (VARIANT == NMRFIT_VARIANT_BASELINE) {
#pragma unroll
            for (int q = 0; q < kPointsPerLane; ++q) acc[q] = base;
            for (int k = 0; k < P; ++k) {
                const PeakLor rec = lor[k];
#pragma unroll
                for (int q = 0; q < kPointsPerLane; ++q) {
                    const double t = __builtin_fma(wv[q], rec.ihw, rec.c);
                    const double s = __builtin_fma(t, t, 1.0);
                    acc[q] = __builtin_fma(rec.al, 1.0 / s, acc[q]);
                    acc[q] = __builtin_fma(rec.ag2, exp2(-s), acc[q]);
                }
            }
        } else {
            double2 mm = make_double2(0.0, 0.0);
            if (kSkip) mm = global_table(chunk_minmax, jb / kChunk);
            if constexpr (kFar) {
                // ---- far-field form --------------------------------------------------------
                // For a peak whose centre is far from this chunk (rho = chunk half-span /
                // |distance to the pole of 1/(1+t^2)| <= 0.1) the Lorentzian is summed through a
                // Taylor expansion about the chunk centre: 1/(1+(tc+tau)^2) = Im sum_n
                // (-tau)^n q^(n+1), q = 1/(tc - i).  The expansions of ALL far peaks share one
                // set of kFarTerms coefficients in u = (w - centre)/half-span, so their cost per
                // point is one degree-15 Horner instead of ~6 ops per peak; truncation
                // <= 0.1^16 of each peak's term.  Near peaks are evaluated directly.
                const double wcen = wave_uniform(0.5 * (mm.x + mm.y));
                const double hw = wave_uniform(0.5 * (mm.y - mm.x));
                double cf[kFarTerms];
                bool horner_done = false;
                if (P <= 32) {
                    // Half a wave of peaks: the even chunks of a segment work out the expansions
                    // of TWO chunks at once -- lanes 0..31 for this chunk, lanes 32..63 for the
                    // next -- and park the second set (sums in LDS, masks in SGPRs) for the odd
                    // chunk that follows.  Either half runs the same operations in the same
                    // order, so a chunk's coefficients do not depend on which half made them.
                    if (!ff_odd) {
                        expand_pair(jb);
                        expand_sums(kFarTerms * kFarPad);
                    }
                    const unsigned near_c = ff_odd ? pend_near : even_near;
                    const unsigned hits_c = ff_odd ? pend_hits : even_hits;
                    wave_lds_fence();
                    const double *src = ffs + (ff_odd ? (FIT_IM == 2 ? kFarTerms * kFarPad : kFarTerms) : 0);
#pragma unroll
                    for (int n = 0; n < kFarTerms; ++n) cf[n] = src[n];
                    {
                        // The shared polynomial FIRST, straight into the accumulators (the offset P*yoff rides in its constant
                        // term): its 16 coefficients are dead before the near peaks and Gaussians need their registers,
                        // and the accumulators need neither initialising nor a separate add per point.
                        const double ihw1 = (hw > 0.0) ? rcp64(hw) : 0.0;
                        const double c0 = cf[0] + base;
                        if constexpr (VARIANT == NMRFIT_VARIANT_FARFIELD32) {
                            // Mixed precision, opt-in: orders 1..15 of the shared polynomial in PACKED
                            // fp32 -- v_pk_fma_f32, two points per instruction -- the constant term and the last step in
                            // fp64.  What is rounded to fp32 is the VARIATION of the far peaks' tails across the chunk
                            // (rho <= 0.1: first order <= a tenth of their sum), never a near peak, a Gaussian or the
                            // data: f moves by <= 5e-12 relative on the reference-generated goldens and on dense spectra
                            // (profiles/r05/farfield_f32_horner.txt), -5.5 % kernel time at C3.
                            typedef float f32x2 __attribute__((ext_vector_type(2)));
                            float cff[kFarTerms];
#pragma unroll
                            for (int n = 1; n < kFarTerms; ++n) cff[n] = (float)cf[n];
#pragma unroll
                            for (int q = 0; q < kPointsPerLane; q += 2) {
                                const double u0 = (wv[q] - wcen) * ihw1, u1 = (wv[q + 1] - wcen) * ihw1;
                                const f32x2 uf = {(float)u0, (float)u1};
                                f32x2 pz = {cff[kFarTerms - 1], cff[kFarTerms - 1]};
#pragma unroll
                                for (int n = kFarTerms - 2; n >= 1; --n) {
                                    const f32x2 cn = {cff[n], cff[n]};
                                    pz = __builtin_elementwise_fma(pz, uf, cn);
                                }
                                acc[q] = __builtin_fma((double)pz.x, u0, c0);         // the constant term and the last step: fp64
                                acc[q + 1] = __builtin_fma((double)pz.y, u1, c0);
                            }
                        } else
#pragma unroll
                        for (int q = 0; q < kPointsPerLane; ++q) {
                            const double uu = (wv[q] - wcen) * ihw1;
                            double pz = cf[kFarTerms - 1];
#pragma unroll
                            for (int n = kFarTerms - 2; n >= 1; --n) pz = __builtin_fma(pz, uu, cf[n]);
                            acc[q] = __builtin_fma(pz, uu, c0);
                        }
                        horner_done = true;
                    }
                    for (unsigned m = near_c; m; m &= m - 1) lorentz_one(lor + __builtin_ctz(m), wv, acc);
                    // (one loop after the other, the mask to one of them: see the direct form below)
                    const bool rec = kRec && full && rec_all;
                    for (unsigned m = rec ? hits_c : 0u; m; m &= m - 1) gauss_add_rec(lor + __builtin_ctz(m), grec + __builtin_ctz(m), wv, acc);
                    for (unsigned m = rec ? 0u : hits_c; m; m &= m - 1) gauss_add<true>(lor + __builtin_ctz(m), wv, acc);
                } else {
#pragma unroll
                    for (int q = 0; q < kPointsPerLane; ++q) acc[q] = base;   // (more than 32 peaks: the near peaks come before the polynomial)
                    double csum = 0.0;    // lane l: coefficient of order l >> 2 (all 4 lanes of a quad)
                    for (int kb = 0; kb < P; kb += kWave) {
                        const int k = kb + lane;
                        const bool act = k < P;
                        bool far = false, ghit = false;
                        double zr = 0.0, zi = 0.0, mr = 0.0, mi = 0.0, al = 0.0;
                        if (act) {
                            const PeakLor rec = lor[k];
                            const PeakWin wn = win[k];
                            ghit = (mm.y >= (double)wn.lo) && (mm.x <= (double)wn.hi);
                            const double tc = __builtin_fma(wcen, rec.ihw, rec.c);
                            const double hk = hw * rec.ihw;
                            const double den = __builtin_fma(tc, tc, 1.0);
                            far = den >= 100.0 * hk * hk;            // rho^2 <= 0.01 (false for NaN)
                            const double rq = rcp64(den);
                            zr = tc * rq;                             // q = (tc + i)/(tc^2 + 1)
                            zi = rq;
                            mr = -hk * zr;                            // multiplier -hk*q per order
                            mi = -hk * zi;
                            al = rec.al;
                        }
                        const unsigned long long farmask = __ballot(far);
                        const unsigned long long nearmask = __ballot(act && !far);
                        const unsigned long long hits = __ballot(ghit);
                        if (farmask) {
                            // order n carries al * Im(q m^n), m = -hk q.  Both roots of the real
                            // recurrence y[n+1] = 2 Re(m) y[n] - |m|^2 y[n-1] have modulus |m|, so
                            // it is as stable as the complex product and costs two operations a term.
                            const double a2 = far ? mr + mr : 0.0;       // lanes without a far peak carry exact zeros
                            const double b2 = far ? -__builtin_fma(mr, mr, mi * mi) : 0.0;
                            double y0 = far ? al * zi : 0.0;
                            double y1 = far ? al * __builtin_fma(zr, mi, zi * mr) : 0.0;
                            double *dst = ffs + lane + (lane >> 4);
#pragma unroll
                            for (int n = 0; n < kFarTerms; ++n) {
                                dst[n * kFarPad] = y0;
                                const double y2 = __builtin_fma(a2, y1, b2 * y0);
                                y0 = y1;
                                y1 = y2;
                            }
                            wave_lds_fence();   // same-wave LDS write -> read
                            // lane l sums order l>>2 over 16 peaks of this pass (quarters padded to
                            // 17: each lane of a read group its own bank), then the quad combines
                            double part = 0.0;
                            const double *row = ffs + (lane >> 2) * kFarPad + (lane & 3) * 17;
#pragma unroll
                            for (int j = 0; j < 16; ++j) part += row[j];
                            part += __shfl_xor(part, 1, kWave);
                            part += __shfl_xor(part, 2, kWave);
                            csum += part;
                            wave_lds_fence();   // reads done before the next pass overwrites
                        }
                        for (unsigned long long m = nearmask; m; m &= m - 1)
                            lorentz_one(lor + kb + __builtin_ctzll(m), wv, acc);
                        for (unsigned long long m = hits; m; m &= m - 1) {
                            const int k1 = kb + __builtin_ctzll(m);
                            if (kRec && full && rec_all)
                                gauss_add_rec(lor + k1, grec + k1, wv, acc);
                            else
                                gauss_add<true>(lor + k1, wv, acc);
                        }
                    }
                    // broadcast the kFarTerms sums through LDS and evaluate them at the lane's points
                    if ((lane & 3) == 0) ffs[lane >> 2] = csum;
                    wave_lds_fence();
#pragma unroll
                    for (int n = 0; n < kFarTerms; ++n) cf[n] = ffs[n];
                }
                if (!horner_done) {
                    const double ihwc = (hw > 0.0) ? rcp64(hw) : 0.0;
#pragma unroll
                    for (int q = 0; q < kPointsPerLane; ++q) {
                        const double uu = (wv[q] - wcen) * ihwc;
                        double pz = cf[kFarTerms - 1];
#pragma unroll
                        for (int n = kFarTerms - 2; n >= 0; --n) pz = __builtin_fma(pz, uu, cf[n]);
                        acc[q] += pz;
                    }
                }
                wave_lds_fence();
            } else {
                // The chunk's FIRST Lorentzian call starts the accumulators (INIT, objective_chunk.h): it takes `base` as the
                // addend of its final FMAs instead of finding it in accumulators set by eight moves beforehand.  Which call
                // that is is decided here, once per chunk, ahead of the pass loop: the first full group, or the short group
                // of a particle with fewer peaks than one.  Without a peak the accumulators are the offset alone.
                int k = 0;
                {
                    const int kend0 = (P < kWave) ? P : kWave;
                    if (kGroupSize <= kend0) {
                        if constexpr (kFastLoop)
                            lorentz_group_fast<kGroupSize, true>(lorf, wv, acc, base);
                        else
                            lorentz_group<kGroupSize, true>(lor, wv, acc, base);
                        k = kGroupSize;
                    } else if (kend0 > 0) {
                        if constexpr (kFastLoop)
                            lorentz_tail_fast<true>(kend0, lorf, wv, acc, base);
                        else
                            lorentz_tail<kGroupSize, true>(kend0, lor, wv, acc, base);
                        k = kend0;
                    } else {
#pragma unroll
                        for (int q = 0; q < kPointsPerLane; ++q) acc[q] = base;
                    }
                }
                for (int kb = 0; kb < P; kb += kWave) {
                    const int kend = (P < kb + kWave) ? P : kb + kWave;
                    // which of peaks kb..kb+63 have their Gaussian window inside this chunk's
                    // [min,max] of w: lane i tests peak kb+i, the ballot is a scalar bit mask
                    unsigned long long hits = ~0ull;
                    if (kSkip) {
                        bool h = false;
                        if (kb + lane < P) {
                            const PeakWin wn = win[kb + lane];
                            h = (mm.y >= (double)wn.lo) && (mm.x <= (double)wn.hi);
                        }
                        hits = __ballot(h);
                    }
                    // Lorentzians first, in straight-line groups; then the (few) Gaussians whose
                    // window touches this chunk, one scalar loop over the set bits of the mask
                    if (kb != 0) k = kb;   // (the first pass: behind the call that started the accumulators)
                    if constexpr (kFastLoop) {
                        for (; k + kGroupSize <= kend; k += kGroupSize) lorentz_group_fast<kGroupSize>(lorf + k, wv, acc);
                        if (k < kend) lorentz_tail_fast(kend - k, lorf + k, wv, acc);
                    } else {
                        for (; k + kGroupSize <= kend; k += kGroupSize) lorentz_group<kGroupSize>(lor + k, wv, acc);
                        if (k < kend) lorentz_tail<kGroupSize>(kend - k, lor + k, wv, acc);   // one smaller group
                    }
                    if (kend - kb < kWave) hits &= (1ull << (kend - kb)) - 1ull;
                    // (two loops one after the other, each an update of the accumulators in place, and the mask goes to one of
                    // them: as the two arms of a branch they met in a second set of the eight accumulators, filled by eight
                    // moves per chunk whether a peak hit or not)
                    const bool rec = kRec && full && rec_all;
                    for (unsigned long long m = rec ? hits : 0ull; m; m &= m - 1) {
                        const int k1 = kb + __builtin_ctzll(m);
                        gauss_add_rec(lor + k1, grec + k1, wv, acc);
                    }
                    for (unsigned long long m = rec ? 0ull : hits; m; m &= m - 1) gauss_add<kSkip>(lor + kb + __builtin_ctzll(m), wv, acc);
                }
            }
        }

        // ---- imaginary model, all peaks (FIT_IM == 2: what generate_result builds, utils.py:271-277) ----
        // I(w) = sum_k [ al_k t/(1+t^2) + (ag2_k/sqrt(pi)) D(sqrt(ln2) t) ]: the Hilbert partner of the
        // pseudo-Voigt sum.  It decays only like 1/t, so there is no window to skip; instead every peak
        // that is FAR from this chunk (the chunk spans <= 0.1 of its distance to the pole, and Dawson's
        // asymptotic series holds over all of it) goes through ONE shared degree-15 polynomial per
        // chunk: t/(1+t^2) is the real part of the same series 1/(t - i) = sum_n q m^n u^n whose
        // imaginary part FARFIELD sums, and x^-(2j+1) of D's series expands binomially about the
        // chunk centre (all terms of one sign: no cancellation; truncation <= 1e-16 of each peak's
        // term).  Near peaks are evaluated point by point with the gathered Dawson table.
        double iacc[kPointsPerLane];
        if constexpr (FIT_IM == 2) {
#pragma unroll
            for (int q = 0; q < kPointsPerLane; ++q) iacc[q] = 0.0;
            const double2 mi2 = global_table(chunk_minmax, jb / kChunk);
            const double icen = wave_uniform(0.5 * (mi2.x + mi2.y));
            const double ihalf = wave_uniform(0.5 * (mi2.y - mi2.x));
            double isum = 0.0;     // lane l: coefficient of order l >> 2 (all 4 lanes of a quad)
            bool anyfar = false;
            const bool pair_im = kFar && P <= 32;   // (wave-uniform; a compile-time false outside the far-field kernel)
            if (pair_im) {
                // the expansions of this chunk and the next were made together by the even chunk (expand_pair_im)
                if (!ff_odd) expand_pair_im(jb);
                anyfar = (pair_far_im & (ff_odd ? 2u : 1u)) != 0u;
                for (unsigned m = ff_odd ? pend_near_im : even_near_im; m; m &= m - 1) {
                    const PeakLor rec = lor[__builtin_ctz(m)];
#pragma unroll
                    for (int q = 0; q < kPointsPerLane; ++q) iacc[q] += dispersion_tab(wv[q], rec, dtab);
                }
            } else
                for (int kb = 0; kb < P; kb += kWave) {
                    const int k = kb + lane;
                    const bool act = k < P;
                    bool farim = false;
                    double tc = 0.0, hk = 0.0, rq = 0.0, al = 0.0, agd = 0.0;
                    if (act) {
                        const PeakLor rec = lor[k];
                        tc = __builtin_fma(icen, rec.ihw, rec.c);
                        hk = ihalf * rec.ihw;
                        const double den = __builtin_fma(tc, tc, 1.0);
                        farim = (den >= 100.0 * hk * hk) && ((fabs(tc) - fabs(hk)) * kSqrtLn2 >= kDawFarX);   // false for NaN
                        rq = rcp64(den);
                        al = rec.al;
                        agd = rec.ag2 * kInvSqrtPi;
                    }
                    const unsigned long long farmask = __ballot(farim);
                    const unsigned long long nearmask = __ballot(act && !farim);
                    if (farmask) {
                        anyfar = true;
                        im_rows(farim, tc, hk, rq, al, agd);
                        wave_lds_fence();   // same-wave LDS write -> read
                        double part = 0.0;
                        const double *row = ffs + (lane >> 2) * kFarPad + (lane & 3) * 17;
#pragma unroll
                        for (int j = 0; j < 16; ++j) part += row[j];
                        part += __shfl_xor(part, 1, kWave);
                        part += __shfl_xor(part, 2, kWave);
                        isum += part;
                        wave_lds_fence();   // reads done before the next pass overwrites
                    }
                    for (unsigned long long m = nearmask; m; m &= m - 1) {
                        const PeakLor rec = lor[kb + __builtin_ctzll(m)];
#pragma unroll
                        for (int q = 0; q < kPointsPerLane; ++q) iacc[q] += dispersion_tab(wv[q], rec, dtab);
                    }
                }
            if (anyfar) {   // wave-uniform
                if (!pair_im) {
                    if ((lane & 3) == 0) ffs[lane >> 2] = isum;
                    wave_lds_fence();
                }
                const double *srci = ffs + ((pair_im && ff_odd) ? kFarTerms * kFarPad + kFarTerms : 0);
                double cfi[kFarTerms];
#pragma unroll
                for (int n = 0; n < kFarTerms; ++n) cfi[n] = srci[n];
                const double ihc = (ihalf > 0.0) ? rcp64(ihalf) : 0.0;
#pragma unroll
                for (int q = 0; q < kPointsPerLane; ++q) {
                    double uu = (wv[q] - icen) * ihc;
                    if (!full) uu = fmin(fmax(uu, -1.0), 1.0);   // padding points of the ragged chunk (weight 0)
                    double pz = cfi[kFarTerms - 1];
#pragma unroll
                    for (int n = kFarTerms - 2; n >= 0; --n) pz = __builtin_fma(pz, uu, cfi[n]);
                    iacc[q] += pz;
                }
                wave_lds_fence();
            }
        }

        if constexpr (FIT_IM == 1) {   // equations.py:197-199: the last peak's line only (before the data loads: 48 VGPRs fewer are live)
            __builtin_amdgcn_sched_barrier(0);   // (not interleaved with the far-field Horner above: its coefficients are dead first)
#pragma unroll
            for (int q = 0; q < kPointsPerLane; ++q) iacc[q] = 0.0;
            if (P > 0) dispersion_points(wv, lor[P - 1], dtab, iacc);
        }
        // keep the u/v/weights loads below the peak loop: hoisted, they would hold 48 VGPRs
        // across it
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
                const int64_t js = jb + (q >> 1) * (2 * kWave) + 2 * lane + (q & 1);   // grid_slot order
                uq[q] = ok ? u[js] : 0.0;
                vq[q] = ok ? v[js] : 0.0;
                tq[q] = ok ? wt[js] : 0.0;   // weight 0: the point contributes nothing
            }
        }
#pragma unroll
        for (int q = 0; q < kPointsPerLane; ++q) {
            const double vd = __builtin_fma(zr, uq[q], -(zi * vq[q]));   // Re((zr + i zi)(u + i v))
            const double e = tq[q] * (vd - acc[q]);                       // equations.py:202
            bs = __builtin_fma(e, e, bs);
            if (FIT_IM != 0) {                                            // equations.py:197-199,205-206
                const double id = __builtin_fma(zr, vq[q], zi * uq[q]);  // Im((zr + i zi)(u + i v))
                const double ei = tq[q] * (id - iacc[q]);
                bs_im = __builtin_fma(ei, ei, bs_im);
                // residual rows of both channels: the imaginary rows are the second plane of the same buffer
                if constexpr (WRITE_R && FIT_IM != 0) {
                    if (full || jl + q * kWave < j1) R_out[(S + particle) * N + jl + q * kWave] = ei;
                }
            }
            if (WRITE_R && (full || jl + q * kWave < j1)) R_out[particle * N + jl + q * kWave] = e;
            const double nzr = __builtin_fma(zr, rr, -(zi * ri));         // z *= rho
            zi = __builtin_fma(zr, ri, zi * rr);
            zr = nzr;
        }
        // Canonical summation order: lane sums over its points of the block, wave tree over
        // lanes, then block sums are added one after another in grid order -- by this wave if
        // it owns the whole grid, else by finalize_kernel.
        if (++cib == blk_chunks || jb + kChunk >= j1) {
            const double cs = wave_sum(bs);
            const double cs_im = (FIT_IM != 0) ? wave_sum(bs_im) : 0.0;
            bs = 0.0;
            bs_im = 0.0;
            cib = 0;
            if (nseg == 1) {
                ss += cs;
                ss_im += cs_im;
            } else if (nseg == WPB) {   // the waves of THIS workgroup (four, or eight) hold the whole particle: sums meet in LDS
                if (lane == 0) {
                    wsums[blk0 + bidx] = cs;
                    if (FIT_IM != 0) wsums[kMaxBlocks + blk0 + bidx] = cs_im;
                }
            } else if (lane == 0) {
                const int64_t slot = particle * n_blocks + blk0 + bidx;
                if (FIT_IM == 0) {
                    out[slot] = cs;
                } else {
                    out[2 * slot] = cs;
                    out[2 * slot + 1] = cs_im;
                }
            }
            ++bidx;
        }
    }
};

}  // namespace
}  // namespace nmrfit

// objective_farfield.h -- the far-field stages of the objective kernel's chunk loop (objective_kernel.h, FARFIELD and
// the all-peak imaginary model): the Taylor coefficients of the far peaks' tails about a chunk's centre, summed over
// peaks through the wave's LDS scratch.  For up to 32 peaks the expansions of a PAIR of chunks are made at once.
// (Structs of references with a call operator: see objective_prologue.h.)
#pragma once
#include "objective_math.h"

namespace nmrfit {
namespace {

// FARFIELD, P <= 32: the far-field expansions of a PAIR of chunks -- lanes 0..31 those of chunk jbE, lanes 32..63
// those of the chunk after it -- summed over peaks into slots 0..15 / 16..31 of the wave's scratch, with the
// near-peak and Gaussian-window masks of the two chunks in scalar registers.  Either half runs the same
// operations in the same order, so a chunk's coefficients do not depend on which half made them, nor on when.
struct ExpandPair {
    const double2 *__restrict__ &chunk_minmax;
    const int64_t &j1;
    const int &lane;
    const int &P;
    PeakLor *&lor;
    PeakWin *&win;
    double *&ffs;
    unsigned &even_near, &even_hits, &pend_near, &pend_hits;   // the masks of the even and of the odd chunk of the pair, kept in scalar registers
    __device__ void operator()(const int64_t jbE) const
    {
        const double2 mm = global_table(chunk_minmax, jbE / kChunk);
        const bool has_next = jbE + kChunk < j1;                  // wave-uniform
        double2 mn = mm;
        if (has_next) mn = global_table(chunk_minmax, jbE / kChunk + 1);
        const bool upper = lane >= 32;
        const int k = lane & 31;
        const double lo_w = upper ? mn.x : mm.x, hi_w = upper ? mn.y : mm.y;
        const bool act = (k < P) && (!upper || has_next);
        bool far = false, ghit = false;
        double a2 = 0.0, b2 = 0.0, y0 = 0.0, y1 = 0.0;
        if (act) {
            const PeakLor rec = lor[k];
            const PeakWin wn = win[k];
            ghit = (hi_w >= (double)wn.lo) && (lo_w <= (double)wn.hi);
            const double tc = __builtin_fma(0.5 * (lo_w + hi_w), rec.ihw, rec.c);
            const double hk = (0.5 * (hi_w - lo_w)) * rec.ihw;
            const double den = __builtin_fma(tc, tc, 1.0);
            far = den >= 100.0 * hk * hk;            // rho^2 <= 0.01 (false for NaN)
            if (far) {
                const double rq = rcp64(den);
                const double qr = tc * rq;            // q = (tc + i)/(tc^2 + 1)
                const double mr = -hk * qr, mi = -hk * rq;   // m = -hk q
                a2 = mr + mr;
                b2 = -__builtin_fma(mr, mr, mi * mi);
                y0 = rec.al * rq;
                y1 = rec.al * __builtin_fma(qr, mi, rq * mr);
            }
        }
        const unsigned long long nearmask = __ballot(act && !far);
        const unsigned long long hits = __ballot(ghit);
        // order n carries al * Im(q m^n); both roots of the real recurrence y[n+1] = 2 Re(m) y[n] - |m|^2 y[n-1]
        // have modulus |m| (stable), two operations a term; lanes without a far peak carry exact zeros (no branch
        // on "any far peak at all": a pair of chunks without one is the rare case, and the branch would cut the
        // straight-line code the scheduler interleaves with the chunk's other work)
        double *dst = ffs + lane + (lane >> 4);
#pragma unroll
        for (int n = 0; n < kFarTerms; ++n) {
            dst[n * kFarPad] = y0;
            const double y2 = __builtin_fma(a2, y1, b2 * y0);
            y0 = y1;
            y1 = y2;
        }
        even_near = (unsigned)nearmask;
        even_hits = (unsigned)hits;
        pend_near = (unsigned)(nearmask >> 32);
        pend_hits = (unsigned)(hits >> 32);
        wave_lds_fence();   // same-wave LDS write -> read (expand_sums)
    }
};

// ... second half: lane l sums order l>>2 over 16 peaks (quarter rows padded to 17 doubles), lanes l, l^1 hold
// the halves of one chunk; sums of the pair's first chunk -> slots 0..15, of its second -> slots 16..31
template <int FIT_IM>
struct ExpandSums {
    double *&ffs;
    const int &lane;
    __device__ void operator()(const int park) const   // park: where the second chunk's sums go (doubles from ffs; FIT_IM == 2 only)
    {
        const double *row = ffs + (lane >> 2) * kFarPad + (lane & 3) * 17;
        double part = 0.0;
#pragma unroll
        for (int j = 0; j < 16; ++j) part += row[j];
        part += __shfl_xor(part, 1, kWave);
        wave_lds_fence();   // reads issued before the sums overwrite row 0
        if constexpr (FIT_IM == 2) {
            if ((lane & 1) == 0) ffs[((lane & 2) ? park : 0) + (lane >> 2)] = part;
        } else {
            if ((lane & 1) == 0) ffs[((lane & 2) << 3) + (lane >> 2)] = part;
        }
        wave_lds_fence();
    }
};

// FIT_IM == 2: one lane's 16 coefficients of the far-field form of ITS peak's imaginary line about a chunk centre --
// al Re(q m^n) by the real two-term recurrence + the Gaussian's asymptotic series expanded binomially (see the
// imaginary block of the chunk below) -- written to the lane's column of the wave's scratch.  Lanes without a far
// peak write exact zeros.
struct ImRows {
    double *&ffs;
    const int &lane;
    __device__ void operator()(const bool farim, const double tc, const double hk, const double rq, const double al, const double agd) const
    {
        const double qr = tc * rq, qi = rq;
        const double mr = -hk * qr, mi = -hk * qi;
        const double a2 = farim ? mr + mr : 0.0;
        const double b2 = farim ? -__builtin_fma(mr, mr, mi * mi) : 0.0;
        double y0 = farim ? al * qr : 0.0;
        double y1 = farim ? al * __builtin_fma(qr, mr, -(qi * mi)) : 0.0;
        // Gaussian dispersion: agd * sum_j A_j x^-(2j+1), x = xc (1 - eps u), eps = -hk/tc:
        // coefficient of u^n = agd eps^n sum_j B_j binom(2j + n, n), B_j = A_j xc^-(2j+1)
        double B[kDawFarTerms];
        {
            const double xc = farim ? kSqrtLn2 * tc : 1.0;
            const double inv = rcp64(xc), inv2 = inv * inv;
            double pw = farim ? agd * inv : 0.0;
#pragma unroll
            for (int j = 0; j < kDawFarTerms; ++j) {
                B[j] = (dawson::kFar[j] * pow49_half(j)) * pw;
                pw *= inv2;
            }
        }
        const double eps = farim ? -hk * rcp64(tc) : 0.0;
        double en = 1.0;
        double *dst = ffs + lane + (lane >> 4);
#pragma unroll
        for (int n = 0; n < kFarTerms; ++n) {
            double sg = 0.0;
#pragma unroll
            for (int j = kDawFarTerms - 1; j >= 0; --j) sg = __builtin_fma(B[j], binom_d(2 * j + n, n), sg);
            dst[n * kFarPad] = __builtin_fma(sg, en, y0);
            en *= eps;
            const double y2 = __builtin_fma(a2, y1, b2 * y0);
            y0 = y1;
            y1 = y2;
        }
    }
};

// ... and, far-field kernel with P <= 32, for a PAIR of chunks at once like expand_pair: lanes 0..31 the peaks against
// chunk jbE, lanes 32..63 against the chunk after it; the sums of the first chunk land in slots 0..15 of the scratch,
// those of the second in a parking row of their own (behind the real part's), the near-peak masks in scalar registers.
template <int FIT_IM>
struct ExpandPairIm {
    const double2 *__restrict__ &chunk_minmax;
    const int64_t &j1;
    const int &lane;
    const int &P;
    PeakLor *&lor;
    unsigned &even_near_im, &pend_near_im, &pair_far_im;   // the same for the imaginary model
    const ImRows &im_rows;
    const ExpandSums<FIT_IM> &expand_sums;
    __device__ void operator()(const int64_t jbE) const
    {
        const double2 mm = global_table(chunk_minmax, jbE / kChunk);
        const bool has_next = jbE + kChunk < j1;                  // wave-uniform
        double2 mn = mm;
        if (has_next) mn = global_table(chunk_minmax, jbE / kChunk + 1);
        const bool upper = lane >= 32;
        const int k = lane & 31;
        const double lo_w = upper ? mn.x : mm.x, hi_w = upper ? mn.y : mm.y;
        const bool act = (k < P) && (!upper || has_next);
        bool farim = false;
        double tc = 0.0, hk = 0.0, rq = 0.0, al = 0.0, agd = 0.0;
        if (act) {
            const PeakLor rec = lor[k];
            tc = __builtin_fma(0.5 * (lo_w + hi_w), rec.ihw, rec.c);
            hk = (0.5 * (hi_w - lo_w)) * rec.ihw;
            const double den = __builtin_fma(tc, tc, 1.0);
            farim = (den >= 100.0 * hk * hk) && ((fabs(tc) - fabs(hk)) * kSqrtLn2 >= kDawFarX);   // false for NaN
            rq = rcp64(den);
            al = rec.al;
            agd = rec.ag2 * kInvSqrtPi;
        }
        const unsigned long long farmask = __ballot(farim);
        const unsigned long long nearmask = __ballot(act && !farim);
        even_near_im = (unsigned)nearmask;
        pend_near_im = (unsigned)(nearmask >> 32);
        pair_far_im = ((unsigned)farmask != 0u ? 1u : 0u) | ((unsigned)(farmask >> 32) != 0u ? 2u : 0u);
        if (farmask) {   // wave-uniform
            im_rows(farim, tc, hk, rq, al, agd);
            wave_lds_fence();   // same-wave LDS write -> read
            expand_sums(kFarTerms * kFarPad + kFarTerms);
        }
    }
};

}  // namespace
}  // namespace nmrfit

// result_point.h -- the reconstruction at ONE grid point, shared by the kernels that evaluate it: result.hip (the arrays
// of FitUtility.generate_result) and quality.hip (the residual statistics, which need V_fit - V_data and nothing else of
// it).  One body each for the per-peak records, the summed lines and the rotated spectrum, so that the two units give
// the same bits.  Device code only.
#pragma once
#include "objective_math.h"

namespace nmrfit {
namespace {

// the per-peak constants the lines are evaluated from (the same as the objective kernels': nmrfit_internal.h, PeakLor)
__device__ __forceinline__ PeakLor peak_record(const double *__restrict__ x, int k, double w0, double wspan)
{
    const double r = x[2];
    const double width = x[4 + 3 * k], loc = x[5 + 3 * k], a = x[6 + 3 * k];
    const double ihw = 2.0 / width;
    const double locc = loc - w0;
    const double lim = 1.0e18 / (wspan + fabs(locc));
    PeakLor rec;   // (a width below the floor: the record of the floor width, as in objective_kernel.h)
    rec.ihw = (fabs(ihw) > lim) ? copysign(lim, ihw) : ihw;
    rec.c = -locc * rec.ihw;
    const double ia = __builtin_isinf(ihw) ? ihw : rec.ihw;   // (width 0: non-finite, like the reference)
    rec.al = a * r * ia * kInvPi;
    rec.ag2 = 2.0 * a * (1.0 - r) * ia * kSqrtLn2OverPi;
    return rec;
}

// the workgroup's copy of a fit's P records in LDS (one fp64 division per peak and workgroup instead of per point);
// every thread of the workgroup calls it
template <int kThreads>
__device__ __forceinline__ void stage_peak_records(PeakLor *__restrict__ recs, const double *__restrict__ x, int P, double w0,
                                                   double wspan)
{
    for (int k = threadIdx.x; k < P; k += kThreads) recs[k] = peak_record(x, k, w0, wspan);
    __syncthreads();
}

// utils.py:262-277 at the centred grid value wj: real, imag per peak; V_fit = V_fit + real, I_fit = I_fit + imag, peak
// after peak from zero.  kImag false: the real lines alone (I is left as it is); real, imag: where point j's values of
// peak 0 go, a peak `stride` doubles after the one before, or null.
template <bool kImag>
__device__ __forceinline__ void point_lines(const PeakLor *__restrict__ recs, int P, double wj, double yoff, double *real,
                                            double *imag, int64_t stride, double *V_out, double *I_out)
{
    double V = 0.0, I = 0.0;
    for (int k = 0; k < P; ++k) {
        const PeakLor rec = recs[k];
        const double t = __builtin_fma(wj, rec.ihw, rec.c);
        const double s = __builtin_fma(t, t, 1.0);
        const double re = yoff + __builtin_fma(rec.al, rcp64(s), rec.ag2 * exp2_neg(-s));
        if (real) real[(int64_t)k * stride] = re;
        V = V + re;
        if constexpr (kImag) {
            const double im = dispersion(wj, rec);
            if (imag) imag[(int64_t)k * stride] = im;
            I = I + im;
        }
    }
    *V_out = V;
    if constexpr (kImag) *I_out = I;
}

// ps2(u, v, p0, p1) at point j of N: V = cos phi u - sin phi v, I = sin phi u + cos phi v, phi_j = p0 + (p1 j) / N
__device__ __forceinline__ void point_data(double uj, double vj, double p0, double p1, int64_t j, int64_t N, double *V_out,
                                           double *I_out)
{
    const double phi = p0 + (p1 * (double)j) / (double)N;
    double sn, cs;
    sincos_fast(phi, &sn, &cs);
    *V_out = cs * uj - sn * vj;
    *I_out = sn * uj + cs * vj;
}

}  // namespace
}  // namespace nmrfit

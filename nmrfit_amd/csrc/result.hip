// result.hip -- the reconstruction that follows a fit (FitUtility.generate_result, nmrfit/utils.py:226-295), on the GPU:
// per-peak real lines (equations.voigt, nmrfit/equations.py:115-149) and their Kramers-Kronig partners in closed form
// (the reference integrates each point numerically, equations.py:9-80), their running sums V_fit / I_fit
// (utils.py:276-277), the fit rotated back to the (u, v) frame (utils.py:284: ps2(V_fit, I_fit, inv=True)) and the
// spectrum rotated by the fitted phase (utils.py:251: data.shift_phase(method='manual'), nmrfit/containers.py:68-78).
//
// One thread per output point walks the peaks of its fit; a workgroup first stages the fit's per-peak constants in LDS
// (one fp64 division per peak and workgroup instead of per point).  The kernel is bound by what it writes -- (2 P + 6)
// doubles per point -- and is launched once for a whole device batch (blockIdx.y = the fit): K x (2 P + 6) x N x 8 B,
// 38 MB for 64 default-size fits, ~10 us of HBM time; the D2H copy that follows is what costs.
#include "result_internal.h"
#include "result_point.h"

#include <algorithm>

namespace nmrfit {
namespace {

__device__ __forceinline__ void result_body(const ResultJob &job, PeakLor *__restrict__ recs)
{
    const int P = job.P;
    const int64_t first = (int64_t)blockIdx.x * kResultThreads;
    const int64_t n_data = job.data ? job.N : 0;
    if (first >= job.Nout && first >= n_data) return;   // (a table's fits may differ in length: whole workgroups leave)
    const double *__restrict__ x = job.x;
    stage_peak_records<kResultThreads>(recs, x, P, job.w0, job.wspan);
    const int64_t j = first + threadIdx.x;
    const double p0 = x[0], p1 = x[1], yoff = x[3];
    if (j < job.Nout) {
        const int64_t Nout = job.Nout;
        const double wj = job.w_plain ? job.w_plain[j] - job.w0 : job.wc[grid_slot(j)];
        double V, I;
        point_lines<true>(recs, P, wj, yoff, job.real ? job.real + j : nullptr, job.imag ? job.imag + j : nullptr, Nout, &V, &I);
        if (job.fit) {
            // proc_autophase.ps2(V_fit, I_fit, inv=True, p0, p1) (proc_autophase.py:29-36): the ramp (p1 * j) / size over
            // the OUTPUT grid's index, rotation by 1 / exp(i phi)
            const double phi = p0 + (p1 * (double)j) / (double)Nout;
            double sn, cs;
            sincos_fast(phi, &sn, &cs);
            job.fit[j] = V;
            job.fit[Nout + j] = I;
            job.fit[2 * Nout + j] = cs * V + sn * I;
            job.fit[3 * Nout + j] = cs * I - sn * V;
        }
    }
    if (j < n_data) {
        const int64_t N = job.N;
        const int64_t slot = grid_slot(j);
        double dV, dI;
        point_data(job.u[slot], job.v[slot], p0, p1, j, N, &dV, &dI);
        job.data[j] = dV;
        job.data[N + j] = dI;
    }
}

__global__ __launch_bounds__(kResultThreads) void result_jobs_kernel(const ResultJob *__restrict__ jobs)
{
    extern __shared__ __align__(16) unsigned char lds_raw[];
    result_body(jobs[blockIdx.y], reinterpret_cast<PeakLor *>(lds_raw));
}

__global__ __launch_bounds__(kResultThreads) void result_one_kernel(const ResultJob job)
{
    extern __shared__ __align__(16) unsigned char lds_raw[];
    result_body(job, reinterpret_cast<PeakLor *>(lds_raw));
}

}  // namespace

int launch_result_jobs(hipStream_t stream, const ResultJob *d_jobs, int32_t njobs, int64_t max_points, int32_t Pmax)
{
    if (njobs <= 0 || max_points <= 0) return NMRFIT_OK;
    const int64_t tiles = (max_points + kResultThreads - 1) / kResultThreads;
    if (njobs > 65535 || tiles > 0x7fffffffLL) {
        set_error("reconstruction launch: at most 65535 fits and 2^31 tiles");
        return NMRFIT_E_INVALID;
    }
    const size_t lds = (size_t)std::max(Pmax, 1) * sizeof(PeakLor);
    hipLaunchKernelGGL(result_jobs_kernel, dim3((unsigned)tiles, (unsigned)njobs), dim3(kResultThreads), lds, stream, d_jobs);
    NMRFIT_HIP(hipGetLastError());
    return NMRFIT_OK;
}

int launch_result_one(hipStream_t stream, const ResultJob &job)
{
    const int64_t points = std::max<int64_t>(job.Nout, job.data ? job.N : 0);
    if (points <= 0) return NMRFIT_OK;
    const int64_t tiles = (points + kResultThreads - 1) / kResultThreads;
    if (tiles > 0x7fffffffLL) {
        set_error("reconstruction launch: grid too long");
        return NMRFIT_E_INVALID;
    }
    const size_t lds = (size_t)std::max(job.P, 1) * sizeof(PeakLor);
    hipLaunchKernelGGL(result_one_kernel, dim3((unsigned)tiles), dim3(kResultThreads), lds, stream, job);
    NMRFIT_HIP(hipGetLastError());
    return NMRFIT_OK;
}

}  // namespace nmrfit

// noise.hip -- noise replicas of spectra on the GPU (opt-in; include/nmrfit_amd_noise.h): data + sigma * standard normal
// deviates, what the reference's utils.rnd_data makes on the host from numpy's global generator, for a ragged batch of
// spectra -- K spectra x M replicas x N points x 2 channels of deviates is the preparation of a replica study, and at
// the batched fit rates it is not small next to the fits.  The deviates are a pure function of (seed, grid point): one
// Philox4x32-10 block per point (the swarm's generator, pso_update.h, under a counter tag of its own) and one Box-Muller
// pair for the two channels, so a replica is the same bits alone, in any batch, out of place (nmrfit_noise_replicas) or
// in place on a batch's resident planes (nmrfit_batch_add_noise, batch_data.hip).  fp64 libdevice log / sin / cos, no fast
// forms; a thread per point, no atomics, no scratch, no LDS.
#include "host_call.h"
#include "nmrfit_amd_noise.h"
#include "noise_internal.h"
#include "pso_update.h"
#include "weights_internal.h"   // the per-call limits, shared with nmrfit_weights_build

#include <algorithm>
#include <cmath>
#include <vector>

namespace nmrfit {
namespace {

#pragma clang fp contract(off)

constexpr int kNoiseThreads = 256;

// (z_u, z_v) of grid point j under the noise seed: the definition in include/nmrfit_amd_noise.h, line by line
__device__ __forceinline__ void noise_normals(uint64_t seed, uint64_t j, double *zu, double *zv)
{
    const U4 c{(uint32_t)j, (uint32_t)(j >> 32), NMRFIT_NOISE_TAG, 0u};
    const U4 o = philox4x32_10(c, (uint32_t)seed, (uint32_t)(seed >> 32));
    const uint64_t ua = ((uint64_t)o.y << 32) | o.x;
    const uint64_t ub = ((uint64_t)o.w << 32) | o.z;
    const double a = (double)((ua >> 11) + 1) * 0x1.0p-53;   // (0, 1]
    const double b = (double)(ub >> 11) * 0x1.0p-53;         // [0, 1)
    const double r = sqrt(-2.0 * log(a));
    const double t = 6.283185307179586 * b;
    double s, co;
    sincos(t, &s, &co);
    *zu = r * co;
    *zv = r * s;
}

template <bool kSlotted>
__global__ __launch_bounds__(kNoiseThreads) void noise_kernel(const NoiseJob *jobs)
{
    const NoiseJob &q = jobs[blockIdx.y];
    const int64_t j = (int64_t)blockIdx.x * kNoiseThreads + threadIdx.x;
    if (j >= q.N) return;
    const int64_t at = kSlotted ? grid_slot(j) : j;
    if (q.sigma_u == 0.0 && q.sigma_v == 0.0) {   // not touched: the bits stay
        if (q.u_out != q.u_in) {
            q.u_out[at] = q.u_in[at];
            q.v_out[at] = q.v_in[at];
        }
        return;
    }
    double zu, zv;
    noise_normals(q.seed, (uint64_t)j, &zu, &zv);
    const double du = q.sigma_u * zu, dv = q.sigma_v * zv;
    q.u_out[at] = q.u_in[at] + du;
    q.v_out[at] = q.v_in[at] + dv;
}

__global__ __launch_bounds__(kNoiseThreads) void noise_gather_kernel(const double *u, const double *v, int64_t N, double *u_out,
                                                                    double *v_out)
{
    const int64_t j = (int64_t)blockIdx.x * kNoiseThreads + threadIdx.x;
    if (j >= N) return;
    const int64_t at = grid_slot(j);
    u_out[j] = u[at];
    v_out[j] = v[at];
}

}  // namespace

int check_noise_args(const char *who, int32_t K, const double *sigma_u, const double *sigma_v, const uint64_t *seed)
{
    if (K <= 0 || !sigma_u || !sigma_v || !seed) {
        set_error(std::string(who) + ": the number of spectra must be > 0 and sigma_u, sigma_v, seed non-null");
        return NMRFIT_E_INVALID;
    }
    for (int32_t k = 0; k < K; ++k)
        if (!(sigma_u[k] >= 0.0) || !(sigma_v[k] >= 0.0) || std::isinf(sigma_u[k]) || std::isinf(sigma_v[k])) {
            set_error(std::string(who) + ": every sigma must be finite and >= 0 (spectrum " + std::to_string(k) + ")");
            return NMRFIT_E_INVALID;
        }
    return NMRFIT_OK;
}

int launch_noise(hipStream_t st, const NoiseJob *jobs, int32_t K, int64_t Nmax, bool slotted)
{
    const dim3 grid((unsigned)((Nmax + kNoiseThreads - 1) / kNoiseThreads), (unsigned)K);
    if (slotted)
        hipLaunchKernelGGL(noise_kernel<true>, grid, dim3(kNoiseThreads), 0, st, jobs);
    else
        hipLaunchKernelGGL(noise_kernel<false>, grid, dim3(kNoiseThreads), 0, st, jobs);
    NMRFIT_HIP(hipGetLastError());
    return NMRFIT_OK;
}

int launch_noise_gather(hipStream_t st, const double *u, const double *v, int64_t N, double *u_out, double *v_out)
{
    const dim3 grid((unsigned)((N + kNoiseThreads - 1) / kNoiseThreads));
    hipLaunchKernelGGL(noise_gather_kernel, grid, dim3(kNoiseThreads), 0, st, u, v, N, u_out, v_out);
    NMRFIT_HIP(hipGetLastError());
    return NMRFIT_OK;
}

}  // namespace nmrfit

using namespace nmrfit;

#pragma GCC visibility push(default)   // the C-ABI: the only symbols the library exports (build.sh: -fvisibility=hidden)

int nmrfit_noise_replicas(int device, int32_t K, const int64_t *N, const double *u, const double *v, const double *sigma_u,
                          const double *sigma_v, const uint64_t *seed, double *u_out, double *v_out)
{
    const char *who = "nmrfit_noise_replicas";
    if (!N || !u || !v || !u_out || !v_out) {
        set_error(std::string(who) + ": null pointer");
        return NMRFIT_E_INVALID;
    }
    int rc = check_noise_args(who, K, sigma_u, sigma_v, seed);
    if (rc != NMRFIT_OK) return rc;
    int64_t points = 0, Nmax = 0;
    bool too_long = false;
    for (int32_t k = 0; k < K; ++k) {
        if (N[k] <= 0) {
            set_error(std::string(who) + ": every spectrum needs N > 0 (spectrum " + std::to_string(k) + ")");
            return NMRFIT_E_INVALID;
        }
        if (N[k] > kWeightsMaxPoints || points > kWeightsMaxPoints) too_long = true;   // (and the sum cannot overflow)
        else points += N[k];
        Nmax = std::max(Nmax, N[k]);
    }
    if (K > kWeightsMaxSpectra || too_long || points > kWeightsMaxPoints) {
        set_error(std::string(who) + ": a call takes at most " + std::to_string(kWeightsMaxSpectra) + " spectra and " +
                  std::to_string(kWeightsMaxPoints) + " grid points (summed over the spectra)");
        return NMRFIT_E_UNSUPPORTED;
    }
    if ((rc = use_device(device)) != NMRFIT_OK) return rc;
    StreamLease lease(device);
    NMRFIT_HIP(lease.take());
    hipStream_t st = lease.s;
    Scratch mem;
    NoiseJob *d_jobs = nullptr;
    double *d_in = nullptr, *d_out = nullptr;   // [2][points] each: the u plane, then the v plane
    const size_t np = (size_t)points, plane = np * sizeof(double);
    NMRFIT_HIP(mem.alloc(&d_jobs, (size_t)K));
    NMRFIT_HIP(mem.alloc(&d_in, 2 * np));
    NMRFIT_HIP(mem.alloc(&d_out, 2 * np));
    std::vector<NoiseJob> jobs((size_t)K);
    int64_t off = 0;
    for (int32_t k = 0; k < K; ++k) {
        jobs[(size_t)k] = NoiseJob{d_in + off, d_in + np + off, d_out + off, d_out + np + off, N[k], sigma_u[k], sigma_v[k], seed[k]};
        off += N[k];
    }
    // (pageable host memory: the copies have left the host arrays when hipMemcpyAsync returns)
    NMRFIT_HIP(hipMemcpyAsync(d_jobs, jobs.data(), jobs.size() * sizeof(NoiseJob), hipMemcpyHostToDevice, st));
    NMRFIT_HIP(hipMemcpyAsync(d_in, u, plane, hipMemcpyHostToDevice, st));
    NMRFIT_HIP(hipMemcpyAsync(d_in + np, v, plane, hipMemcpyHostToDevice, st));
    if ((rc = launch_noise(st, d_jobs, K, Nmax, false)) != NMRFIT_OK) return rc;
    if ((rc = staged_d2h(device, st, u_out, d_out, plane)) != NMRFIT_OK) return rc;
    return staged_d2h(device, st, v_out, d_out + np, plane);
}

#pragma GCC visibility pop

// noise_internal.h -- shared by noise.hip (the kernels, nmrfit_noise_replicas) and batch_data.hip (nmrfit_batch_add_noise,
// nmrfit_batch_spectrum): one spectrum of a noise launch, the argument check and the launches.
#pragma once
#include "nmrfit_internal.h"

namespace nmrfit {

// One spectrum of a launch: N points of (u_in, v_in) become (u_out, v_out) = (u_in + sigma_u z_u, v_in + sigma_v z_v)
// with the deviates of (seed, j), include/nmrfit_amd_noise.h.  In place (u_out == u_in) or not.
struct NoiseJob {
    const double *u_in, *v_in;
    double *u_out, *v_out;
    int64_t N;
    double sigma_u, sigma_v;
    uint64_t seed;
};

// what both entry points check before any device work: K sigmas of each channel, finite and >= 0, and the seeds non-null
int check_noise_args(const char *who, int32_t K, const double *sigma_u, const double *sigma_v, const uint64_t *seed);

// One launch on `st` over K jobs in device memory (grid.y = the job, a thread per point; Nmax: the longest spectrum).
// slotted: point j of a job lies at grid_slot(j) of its arrays (a batch's resident planes), else at j.
int launch_noise(hipStream_t st, const NoiseJob *jobs, int32_t K, int64_t Nmax, bool slotted);

// u_out[j] = u[grid_slot(j)], v_out[j] = v[grid_slot(j)] for j < N (device pointers): the inverse of a batch's scatter
int launch_noise_gather(hipStream_t st, const double *u, const double *v, int64_t N, double *u_out, double *v_out);

}  // namespace nmrfit

// weights_internal.h -- shared by weights.hip (the kernels, nmrfit_weights_build) and batch_create.hip
// (nmrfit_batch_create_regions): the layout of a ragged batch of weight regions and the two launches that turn it into
// the spectra's error weights.
#pragma once
#include "nmrfit_internal.h"

namespace nmrfit {

constexpr int32_t kWeightsMaxSpectra = 65535;            // spectra per call (a launch's grid.y)
constexpr int64_t kWeightsMaxPoints = (int64_t)1 << 26;  // grid points per call, summed over the spectra (w and the weights: 512 MiB each)

// one spectrum of the batch: its N points from x_off in the concatenated grids / weights, its R regions from r_off in the
// concatenated region tables
struct WeightSpec {
    int64_t x_off, N;
    int64_t r_off;
    int32_t R, pad;
};

// What both entry points check before any device work: S > 0, N and R non-null, N[k] > 0, R[k] >= 0, edges and level
// non-null where there is a region (NMRFIT_E_INVALID); the per-call limits above (NMRFIT_E_UNSUPPORTED).  *n_points,
// *n_regions: the sums.
int check_weight_regions(const char *who, int32_t S, const int64_t *N, const int32_t *R, const double *edges,
                         const double *level, int64_t *n_points, int64_t *n_regions);

// the layout of S spectra (N[k] > 0, R[k] >= 0, already checked): specs[k], and for every region its spectrum
void weights_layout(int32_t S, const int64_t *N, const int32_t *R, std::vector<WeightSpec> *specs,
                    std::vector<int32_t> *region_spec);

// The first of the two launches below on its own (quality.hip takes its region edges from it: the rule is written once):
// the nearest grid point to both edges of every region into first_last (2 int64 per region, sorted).  No region: nothing.
int launch_weights_nearest(hipStream_t st, const WeightSpec *specs, const int32_t *region_spec, int64_t n_regions,
                           const double *w, const double *edges, int64_t *first_last);

// The two launches on `st` (device pointers): the nearest grid point to both edges of every region into first_last
// (2 int64 per region, sorted), then fill + ten smoothing sweeps of every spectrum into out (sum N doubles, laid out
// like w).  n_regions = sum R (0: one launch), Nmax = the longest spectrum.
int launch_weights(hipStream_t st, int32_t S, const WeightSpec *specs, const int32_t *region_spec, int64_t n_regions,
                   int64_t Nmax, const double *w, const double *edges, const double *level, int64_t *first_last,
                   double *out);

}  // namespace nmrfit

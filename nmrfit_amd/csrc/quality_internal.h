// quality_internal.h -- shared by quality.hip (the kernels, nmrfit_quality_stats) and batch_data.hip
// (nmrfit_batch_quality_stats): one fit of a residual-statistics launch, the argument check and the launches.
#pragma once
#include "nmrfit_amd_quality.h"
#include "weights_internal.h"

namespace nmrfit {

constexpr int kQualityTile = 256;                           // points per tile: a workgroup, one point per thread
constexpr int kQualityRow = NMRFIT_QUALITY_ROW;             // doubles per row
constexpr int32_t kQualityMaxRegions = NMRFIT_QUALITY_MAX_REGIONS;

// One fit of a launch.  Every pointer is device memory.
struct QualityJob {
    const double *w, *u, *v;       // slotted: the centred grid and the spectrum in grid_slot order (a batch's resident planes,
                                   // a context's); else in plain order, w NOT centred (w[j] - w0 is formed in the kernel,
                                   // the same subtraction that made the resident planes)
    const double *x;               // the parameter vector, 4 + 3 P doubles
    const int64_t *first_last;     // R pairs: the regions' first and last index (launch_weights_nearest)
    double *partial;               // [R + 2][tiles][8]: the tiles' sums, written by stage 1
    double *out;                   // [R + 2][8]: the rows
    double w0, wspan;              // centring offset of the fit's grid and its span (analyse_grid)
    int64_t N;
    int32_t P, R;
    int32_t tiles, slotted;        // tiles = ceil(N / kQualityTile)
};

inline int64_t quality_tiles(int64_t N) { return (N + kQualityTile - 1) / kQualityTile; }

// What both entry points check before any device work (include/nmrfit_amd_quality.h): K > 0, N[k] > 0, R[k] >= 0, edges
// non-null where there is a region and no NaN among them (NMRFIT_E_INVALID); the per-call limits of nmrfit_weights_build
// and R[k] <= kQualityMaxRegions (NMRFIT_E_UNSUPPORTED).  *n_points, *n_regions: the sums.
int check_quality_args(const char *who, int32_t K, const int64_t *N, const int32_t *R, const double *edges,
                       int64_t *n_points, int64_t *n_regions);

// The three launches on `st` over K jobs in device memory, whose first_last the first launch fills: the regions' nearest
// points (specs, region_spec, n_regions, w_plain, edges: as for launch_weights_nearest; w_plain the K grids in plain
// order, NOT centred), the tiles' sums (grid.y = the fit; max_tiles, Pmax, Rmax: the largest of the jobs) and the fold
// into the rows.
int launch_quality(hipStream_t st, const QualityJob *jobs, int32_t K, int64_t max_tiles, int32_t Pmax, int32_t Rmax,
                   const WeightSpec *specs, const int32_t *region_spec, int64_t n_regions, const double *w_plain,
                   const double *edges, int64_t *first_last);

}  // namespace nmrfit

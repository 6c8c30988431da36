// weights.hip -- the error weights of a fit on the GPU (opt-in): FitUtility._compute_weights of the reference
// (nmrfit/utils.py:191-224) for a ragged batch of spectra.  Spectrum k has N[k] grid points and R[k] regions, a region
// being a peak's bounds (b0, b1) and its level (tallest |height| / |height|) ** expon -- the levels are formed on the
// host by the scalar power the reference calls; the device never calls pow.  Two launches:
//   1. weights_nearest_kernel      a workgroup per region: argmin_j |w[j] - b0| and argmin_j |w[j] - b1| in one scan of
//                                  the spectrum's grid, with numpy's argmin order (a NaN wins, else the smallest value;
//                                  the lowest index on ties), sorted into (first, last).  w in any order: a full scan.
//   2. weights_fill_smooth_kernel  a workgroup per kTile points: a point's value is the level of the LAST region that
//                                  holds it (the reference assigns the slices in list order), 1 where none does; then
//                                  the ten sweeps of equations.laplace1d (utils.py:223; nmrfit/equations.py:215-238) in
//                                  LDS on the tile and a halo of ten points either side, whose fill values the workgroup
//                                  computes itself; the end points of a spectrum never change.
// Every value is an exact restatement of numpy's arithmetic (contraction off), so a spectrum's weights are bit-identical
// to the host routine's, alone or in any batch.  No atomics, no scratch; every loop is bounded.
#include "host_call.h"
#include "nmrfit_amd_prep.h"
#include "weights_internal.h"

#include <algorithm>
#include <cmath>
#include <vector>

namespace nmrfit {
namespace {

#pragma clang fp contract(off)

constexpr int kNearThreads = 256;
constexpr int kSweeps = 10;                   // laplace1d(x, n=10, ...)
constexpr int kTile = NMRFIT_WEIGHTS_TILE;    // points a workgroup owns
constexpr int kSmoothThreads = 256;
constexpr int kStage = kTile + 2 * kSweeps;   // ... and stages: a sweep spoils one more point at each end of the stage
constexpr double kOmega = 0.33333333;         // laplace1d(..., omega=0.33333333)
constexpr double kKeep = 1. - kOmega;         // (1. - omega) * x[1:-1]
constexpr double kShare = kOmega * 0.5;       // + omega * 0.5 * (x[2:] + x[:-2])

// (|w[j] - b|, j) in np.argmin's order: a NaN comes before every number, and of two NaNs or two equal values the one
// with the lower index
struct Near {
    double d;
    int64_t j;
};
__device__ __forceinline__ bool before(const Near &a, const Near &b)
{
    const bool an = __builtin_isnan(a.d), bn = __builtin_isnan(b.d);
    if (an || bn) return an && (!bn || a.j < b.j);
    return a.d < b.d || (a.d == b.d && a.j < b.j);
}
__device__ __forceinline__ Near wave_first(Near a)
{
    for (int o = kWave / 2; o > 0; o >>= 1) {
        const Near b{__shfl_xor(a.d, o), (int64_t)__shfl_xor((long long)a.j, o)};
        if (before(b, a)) a = b;
    }
    return a;
}

// launch 1: one workgroup per region, one scan of its spectrum's grid for both edges
__global__ __launch_bounds__(kNearThreads) void weights_nearest_kernel(const WeightSpec *specs, const int32_t *region_spec,
                                                                      const double *w_all, const double *edges,
                                                                      int64_t *first_last)
{
    __shared__ double s_d[2][kNearThreads / kWave];
    __shared__ long long s_j[2][kNearThreads / kWave];
    const int64_t r = blockIdx.x;
    const WeightSpec sp = specs[region_spec[r]];
    const double *w = w_all + sp.x_off;
    const double b0 = edges[2 * r], b1 = edges[2 * r + 1];
    Near n0{INFINITY, INT64_MAX}, n1{INFINITY, INT64_MAX};
    for (int64_t j = threadIdx.x; j < sp.N; j += kNearThreads) {
        const double x = w[j];
        const Near c0{fabs(x - b0), j}, c1{fabs(x - b1), j};
        if (before(c0, n0)) n0 = c0;
        if (before(c1, n1)) n1 = c1;
    }
    n0 = wave_first(n0);
    n1 = wave_first(n1);
    const int lane = threadIdx.x % kWave, wave = threadIdx.x / kWave;
    if (lane == 0) {
        s_d[0][wave] = n0.d;
        s_j[0][wave] = n0.j;
        s_d[1][wave] = n1.d;
        s_j[1][wave] = n1.j;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int k = 1; k < kNearThreads / kWave; ++k) {
            const Near c0{s_d[0][k], (int64_t)s_j[0][k]}, c1{s_d[1][k], (int64_t)s_j[1][k]};
            if (before(c0, n0)) n0 = c0;
            if (before(c1, n1)) n1 = c1;
        }
        first_last[2 * r] = std::min(n0.j, n1.j);
        first_last[2 * r + 1] = std::max(n0.j, n1.j);
    }
}

// launch 2: workgroup blockIdx.x of spectrum blockIdx.y owns points [k0, k0 + kTile) and stages [k0 - 10, k0 + kTile + 10).
// After sweep s the staged values are the spectrum's except the outer s at each end of the stage (their neighbours were
// not staged) -- unless the stage ends beyond the spectrum, whose end points are fixed: the owned points are exact.
__global__ __launch_bounds__(kSmoothThreads) void weights_fill_smooth_kernel(const WeightSpec *specs, const double *level,
                                                                            const int64_t *first_last, double *out)
{
    __shared__ double buf[2][kStage];
    const WeightSpec sp = specs[blockIdx.y];
    const int64_t k0 = (int64_t)blockIdx.x * kTile;
    if (k0 >= sp.N) return;
    const int64_t *fl = first_last + 2 * sp.r_off;
    const double *lv = level + sp.r_off;
    const int t = threadIdx.x;
    for (int q = t; q < kStage; q += kSmoothThreads) {
        const int64_t p = k0 - kSweeps + q;
        double x = 1.0;
        if (p >= 0 && p < sp.N)
            for (int32_t r = sp.R - 1; r >= 0; --r)   // the last region that holds p
                if (fl[2 * r] <= p && p <= fl[2 * r + 1]) {
                    x = lv[r];
                    break;
                }
        buf[0][q] = x;
    }
    __syncthreads();
    int cur = 0;
    for (int s = 0; s < kSweeps; ++s) {
        const double *from = buf[cur];
        double *to = buf[cur ^ 1];
        for (int q = t; q < kStage; q += kSmoothThreads) {
            const int64_t p = k0 - kSweeps + q;
            double x = from[q];
            if (q > 0 && q < kStage - 1 && p > 0 && p < sp.N - 1) x = kKeep * x + kShare * (from[q + 1] + from[q - 1]);
            to[q] = x;
        }
        __syncthreads();
        cur ^= 1;
    }
    for (int q = t; q < kTile; q += kSmoothThreads)
        if (k0 + q < sp.N) out[sp.x_off + k0 + q] = buf[cur][q + kSweeps];
}

}  // namespace

void weights_layout(int32_t S, const int64_t *N, const int32_t *R, std::vector<WeightSpec> *specs,
                    std::vector<int32_t> *region_spec)
{
    specs->assign((size_t)S, WeightSpec{});
    region_spec->clear();
    int64_t x_off = 0, r_off = 0;
    for (int32_t k = 0; k < S; ++k) {
        WeightSpec &sp = (*specs)[(size_t)k];
        sp.x_off = x_off;
        sp.N = N[k];
        sp.r_off = r_off;
        sp.R = R[k];
        region_spec->insert(region_spec->end(), (size_t)R[k], k);
        x_off += N[k];
        r_off += R[k];
    }
}

int launch_weights_nearest(hipStream_t st, const WeightSpec *specs, const int32_t *region_spec, int64_t n_regions,
                           const double *w, const double *edges, int64_t *first_last)
{
    if (n_regions <= 0) return NMRFIT_OK;
    hipLaunchKernelGGL(weights_nearest_kernel, dim3((unsigned)n_regions), dim3(kNearThreads), 0, st, specs, region_spec, w,
                       edges, first_last);
    NMRFIT_HIP(hipGetLastError());
    return NMRFIT_OK;
}

int launch_weights(hipStream_t st, int32_t S, const WeightSpec *specs, const int32_t *region_spec, int64_t n_regions,
                   int64_t Nmax, const double *w, const double *edges, const double *level, int64_t *first_last,
                   double *out)
{
    const int rc = launch_weights_nearest(st, specs, region_spec, n_regions, w, edges, first_last);
    if (rc != NMRFIT_OK) return rc;
    const dim3 grid((unsigned)((Nmax + kTile - 1) / kTile), (unsigned)S);
    hipLaunchKernelGGL(weights_fill_smooth_kernel, grid, dim3(kSmoothThreads), 0, st, specs, level, first_last, out);
    NMRFIT_HIP(hipGetLastError());
    return NMRFIT_OK;
}

// what both entry points check before any device work; *n_points, *n_regions: the sums
int check_weight_regions(const char *who, int32_t S, const int64_t *N, const int32_t *R, const double *edges,
                         const double *level, int64_t *n_points, int64_t *n_regions)
{
    if (S <= 0 || !N || !R) {
        set_error(std::string(who) + ": the number of spectra must be > 0 and N, R non-null");
        return NMRFIT_E_INVALID;
    }
    int64_t points = 0, regions = 0;
    bool too_long = false;
    for (int32_t k = 0; k < S; ++k) {
        if (N[k] <= 0 || R[k] < 0) {
            set_error(std::string(who) + ": every spectrum needs N > 0 and R >= 0 (spectrum " + std::to_string(k) + ")");
            return NMRFIT_E_INVALID;
        }
        if (N[k] > kWeightsMaxPoints || points > kWeightsMaxPoints) too_long = true;   // (and the sum cannot overflow)
        else points += N[k];
        regions += R[k];
    }
    if (regions > 0 && (!edges || !level)) {
        set_error(std::string(who) + ": null pointer (edges, level)");
        return NMRFIT_E_INVALID;
    }
    if (S > kWeightsMaxSpectra || too_long || points > kWeightsMaxPoints || regions > 0x7fffffffLL) {
        set_error(std::string(who) + ": a call takes at most " + std::to_string(kWeightsMaxSpectra) + " spectra and " +
                  std::to_string(kWeightsMaxPoints) + " grid points (summed over the spectra)");
        return NMRFIT_E_UNSUPPORTED;
    }
    *n_points = points;
    *n_regions = regions;
    return NMRFIT_OK;
}

}  // namespace nmrfit

using namespace nmrfit;

#pragma GCC visibility push(default)   // the C-ABI: the only symbols the library exports (build.sh: -fvisibility=hidden)

int nmrfit_weights_build(int device, int32_t S, const int64_t *N, const double *w, const int32_t *R, const double *edges,
                         const double *level, double *weights_out, int64_t *first_last_out)
{
    const char *who = "nmrfit_weights_build";
    if (!w || !weights_out) {
        set_error(std::string(who) + ": null pointer");
        return NMRFIT_E_INVALID;
    }
    int64_t n_points = 0, n_regions = 0;
    int rc = check_weight_regions(who, S, N, R, edges, level, &n_points, &n_regions);
    if (rc != NMRFIT_OK) return rc;
    std::vector<WeightSpec> specs;
    std::vector<int32_t> region_spec;
    weights_layout(S, N, R, &specs, &region_spec);
    if ((rc = use_device(device)) != NMRFIT_OK) return rc;
    StreamLease lease(device);
    NMRFIT_HIP(lease.take());
    hipStream_t st = lease.s;
    Scratch mem;
    WeightSpec *d_specs = nullptr;
    int32_t *d_rs = nullptr;
    double *d_w = nullptr, *d_edges = nullptr, *d_level = nullptr, *d_out = nullptr;
    int64_t *d_fl = nullptr;
    const size_t nr = (size_t)n_regions, np = (size_t)n_points;
    NMRFIT_HIP(mem.alloc(&d_specs, specs.size()));
    NMRFIT_HIP(mem.alloc(&d_rs, nr));
    NMRFIT_HIP(mem.alloc(&d_w, np));
    NMRFIT_HIP(mem.alloc(&d_edges, 2 * nr));
    NMRFIT_HIP(mem.alloc(&d_level, nr));
    NMRFIT_HIP(mem.alloc(&d_fl, 2 * nr));
    NMRFIT_HIP(mem.alloc(&d_out, np));
    NMRFIT_HIP(hipMemcpyAsync(d_specs, specs.data(), specs.size() * sizeof(WeightSpec), hipMemcpyHostToDevice, st));
    NMRFIT_HIP(hipMemcpyAsync(d_w, w, np * sizeof(double), hipMemcpyHostToDevice, st));
    if (nr) {
        NMRFIT_HIP(hipMemcpyAsync(d_rs, region_spec.data(), nr * sizeof(int32_t), hipMemcpyHostToDevice, st));
        NMRFIT_HIP(hipMemcpyAsync(d_edges, edges, 2 * nr * sizeof(double), hipMemcpyHostToDevice, st));
        NMRFIT_HIP(hipMemcpyAsync(d_level, level, nr * sizeof(double), hipMemcpyHostToDevice, st));
    }
    int64_t Nmax = 0;
    for (int32_t k = 0; k < S; ++k) Nmax = std::max(Nmax, N[k]);
    if ((rc = launch_weights(st, S, d_specs, d_rs, n_regions, Nmax, d_w, d_edges, d_level, d_fl, d_out)) != NMRFIT_OK) return rc;
    if ((rc = staged_d2h(device, st, weights_out, d_out, np * sizeof(double))) != NMRFIT_OK) return rc;
    if (first_last_out && nr) return staged_d2h(device, st, first_last_out, d_fl, 2 * nr * sizeof(int64_t));
    return NMRFIT_OK;
}

#pragma GCC visibility pop

// quality.hip -- residual statistics of finished fits on the GPU (opt-in; include/nmrfit_amd_quality.h): e = V_fit - V_data
// reduced per region of the grid, over the whole grid and over what no region holds, in a fixed order -- (R + 2) rows of
// 8 doubles per fit instead of the (2 P + 6) N doubles of the reconstruction.  Three launches:
//   1. weights.hip's nearest-point launch   the regions' (first, last) indices, by the rule of utils.compute_weights
//   2. quality_tiles_kernel                 a workgroup per tile of 256 points, a thread per point: V_j and d_j by the
//                                           functions result.hip evaluates them with (result_point.h), e_{j-1} from the
//                                           neighbouring lane, then per row the wave's tree and the four waves in order
//   3. quality_fold_kernel                  a thread per (fit, row, quantity): the tiles' sums in ascending tile order
// No atomics, no scratch memory; every value is a pure function of (spectrum, x, regions).
#include "host_call.h"
#include "quality_internal.h"
#include "result_point.h"

#include <algorithm>
#include <cmath>
#include <vector>

namespace nmrfit {
namespace {

#pragma clang fp contract(off)   // (the sums' terms are rounded products; the shared per-point functions keep their own setting)

constexpr int kTile = kQualityTile;
constexpr int kTileWaves = kTile / kWave;
constexpr int kRowBatch = 16;   // rows whose wave sums wait in LDS for the four waves to be added (two barriers per batch)
constexpr int kQ = kQualityRow;

// V_j and d_j of point j < N, as the reconstruction kernel forms them
__device__ __forceinline__ void point_values(const QualityJob &q, const PeakLor *__restrict__ recs, int j, double p0, double p1,
                                             double yoff, double *V, double *d)
{
    const int64_t at = q.slotted ? grid_slot(j) : j;
    const double wj = q.slotted ? q.w[at] : q.w[at] - q.w0;
    point_lines<false>(recs, q.P, wj, yoff, nullptr, nullptr, 0, V, nullptr);
    double dI;
    point_data(q.u[at], q.v[at], p0, p1, j, q.N, d, &dI);
}

// point j lies in no region (fl: the fit's R staged pairs)
__device__ __forceinline__ bool in_no_region(const int *__restrict__ fl, int R, int j)
{
    bool held = false;
    for (int r = 0; r < R; ++r) held = held || (fl[2 * r] <= j && j <= fl[2 * r + 1]);
    return !held;
}

// (|e_j|, j) of a row's points whose e is a number, largest value first and the lowest index among equals; no point: (-1, .)
struct Peak {
    double a;
    int j;
};
__device__ __forceinline__ bool above(const Peak &x, const Peak &y) { return x.a > y.a || (x.a == y.a && x.j < y.j); }
__device__ __forceinline__ Peak wave_peak(Peak p)
{
    for (int o = kWave / 2; o > 0; o >>= 1) {
        const Peak other{__shfl_xor(p.a, o), __shfl_xor(p.j, o)};
        if (above(other, p)) p = other;
    }
    return p;
}

// Stage 1.  Workgroup blockIdx.x of fit blockIdx.y owns points [256 blockIdx.x, +256); thread t the point 256 blockIdx.x + t.
__global__ __launch_bounds__(kTile) void quality_tiles_kernel(const QualityJob *__restrict__ jobs)
{
    extern __shared__ __align__(16) unsigned char lds_raw[];
    __shared__ double s_sum[kRowBatch][kTileWaves][kQ];
    __shared__ double s_last_e[kTileWaves];
    __shared__ int s_last_free[kTileWaves];
    const QualityJob &q = jobs[blockIdx.y];
    if ((int)blockIdx.x >= q.tiles) return;   // (the fits of a launch may differ in length: whole workgroups leave)
    const int P = q.P, R = q.R, N = (int)q.N;   // (N <= 2^26: kWeightsMaxPoints)
    PeakLor *recs = reinterpret_cast<PeakLor *>(lds_raw);
    int *fl = reinterpret_cast<int *>(recs + P);
    const double *__restrict__ x = q.x;
    for (int r = threadIdx.x; r < 2 * R; r += kTile) fl[r] = (int)q.first_last[r];
    stage_peak_records<kTile>(recs, x, P, q.w0, q.wspan);   // (ends with the workgroup's barrier: fl is staged too)
    const double p0 = x[0], p1 = x[1], yoff = x[3];
    const int tile0 = (int)blockIdx.x * kTile;
    const int j = tile0 + (int)threadIdx.x;
    const int lane = threadIdx.x % kWave, wave = threadIdx.x / kWave;
    const bool inside = j < N;

    // the point's residual and its neighbour's: e_{j-1} from the lane below; lane 0 of a wave takes it from the wave below
    // through LDS, the tile's first thread evaluates the point before the tile
    double e = 0.0, d = 0.0;
    bool free_j = false;   // j is in no region
    if (inside) {
        double V;
        point_values(q, recs, j, p0, p1, yoff, &V, &d);
        e = V - d;
        free_j = in_no_region(fl, R, j);
    }
    double e_prev = __shfl_up(e, 1);
    bool free_prev = __shfl_up((int)free_j, 1) != 0;
    if (lane == kWave - 1) {
        s_last_e[wave] = e;
        s_last_free[wave] = (int)free_j;
    }
    if (threadIdx.x == 0 && j > 0) {   // (j - 1 < N: the tile exists)
        double V, dp;
        point_values(q, recs, j - 1, p0, p1, yoff, &V, &dp);
        e_prev = V - dp;
        free_prev = in_no_region(fl, R, j - 1);
    }
    __syncthreads();
    if (lane == 0 && wave > 0) {
        e_prev = s_last_e[wave - 1];
        free_prev = s_last_free[wave - 1] != 0;
    }
    const bool has_prev = inside && j > 0;
    const double step = e - e_prev;
    const double ee = e * e, dd = d * d, ss = step * step, ae = fabs(e);

    // Per row: does this wave's range of 64 indices meet the row's first .. last?  Wave-uniform by construction (the
    // wave's base index and the row's pair go through readfirstlane), so a wave skips the whole reduction of a row it
    // does not touch -- regions are narrow: nearly every (wave, region) pair -- and leaves the sums' +0.0.
    const int wbase = __builtin_amdgcn_readfirstlane(tile0 + wave * kWave);
    const int rows = R + 2;
    double *__restrict__ partial = q.partial;
    for (int row0 = 0; row0 < rows; row0 += kRowBatch) {
        const int nb = min(kRowBatch, rows - row0);
        for (int i = 0; i < nb; ++i) {
            const int row = row0 + i;
            int first = 0, last = N - 1;
            if (row < R) {
                first = __builtin_amdgcn_readfirstlane(fl[2 * row]);
                last = __builtin_amdgcn_readfirstlane(fl[2 * row + 1]);
            }
            const bool rest = row == R + 1;   // the complement row
            double out[kQ] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, -1.0, -1.0};
            if (wbase < N && wbase <= last && wbase + (kWave - 1) >= first) {
                const bool m = inside && first <= j && j <= last && (!rest || free_j);
                const bool mp = m && has_prev && first <= j - 1 && (!rest || free_prev);
                out[0] = (double)__popcll(__ballot(m));
                out[1] = wave_sum(m ? e : 0.0);
                out[2] = wave_sum(m ? ee : 0.0);
                out[3] = wave_sum(mp ? ss : 0.0);
                out[4] = wave_sum(m ? d : 0.0);
                out[5] = wave_sum(m ? dd : 0.0);
                const bool counts = m && !__builtin_isnan(e);
                const Peak top = wave_peak(Peak{counts ? ae : -1.0, counts ? j : 0x7fffffff});
                out[6] = top.a;
                out[7] = top.a < 0.0 ? -1.0 : (double)top.j;
            }
            if (lane == 0)
                for (int k = 0; k < kQ; ++k) s_sum[i][wave][k] = out[k];
        }
        __syncthreads();
        if ((int)threadIdx.x < nb * kQ) {
            const int i = threadIdx.x / kQ, k = threadIdx.x % kQ;
            double t;
            if (k < 6) {
                t = s_sum[i][0][k];
                for (int wv = 1; wv < kTileWaves; ++wv) t += s_sum[i][wv][k];
            } else {
                double a = s_sum[i][0][6], at = s_sum[i][0][7];
                for (int wv = 1; wv < kTileWaves; ++wv)
                    if (s_sum[i][wv][6] > a) {   // (the waves' indices ascend: equal values keep the lower one)
                        a = s_sum[i][wv][6];
                        at = s_sum[i][wv][7];
                    }
                t = k == 6 ? a : at;
            }
            partial[((int64_t)(row0 + i) * q.tiles + blockIdx.x) * kQ + k] = t;
        }
        __syncthreads();
    }
}

// Stage 2.  Thread (row, quantity) of fit blockIdx.y adds the tiles' sums in ascending tile order.
__global__ __launch_bounds__(kTile) void quality_fold_kernel(const QualityJob *__restrict__ jobs)
{
    const QualityJob &q = jobs[blockIdx.y];
    const int t = blockIdx.x * kTile + threadIdx.x;
    const int row = t / kQ, k = t % kQ;
    if (row >= q.R + 2) return;
    const double *__restrict__ p = q.partial + (int64_t)row * q.tiles * kQ;
    double r;
    if (k < 6) {
        r = p[k];
        for (int tile = 1; tile < q.tiles; ++tile) r += p[(int64_t)tile * kQ + k];
    } else {
        double a = p[6], at = p[7];
        for (int tile = 1; tile < q.tiles; ++tile) {
            const double b = p[(int64_t)tile * kQ + 6], bt = p[(int64_t)tile * kQ + 7];
            if (b > a || (b == a && bt < at)) {   // the larger value; on a tie the lower index
                a = b;
                at = bt;
            }
        }
        r = k == 6 ? (a < 0.0 ? 0.0 : a) : (a < 0.0 ? -1.0 : at);
    }
    q.out[(int64_t)row * kQ + k] = r;
}

}  // namespace

int check_quality_args(const char *who, int32_t K, const int64_t *N, const int32_t *R, const double *edges,
                       int64_t *n_points, int64_t *n_regions)
{
    if (K <= 0 || !N || !R) return refuse(NMRFIT_E_INVALID, std::string(who) + ": the number of fits must be > 0 and N, R non-null");
    int64_t points = 0, regions = 0;
    int32_t Rmax = 0;
    bool too_long = false;
    for (int32_t k = 0; k < K; ++k) {
        if (N[k] <= 0 || R[k] < 0)
            return refuse(NMRFIT_E_INVALID, std::string(who) + ": every fit needs N > 0 and R >= 0 (fit " + std::to_string(k) + ")");
        if (N[k] > kWeightsMaxPoints || points > kWeightsMaxPoints) too_long = true;   // (and the sum cannot overflow)
        else points += N[k];
        regions += R[k];
        Rmax = std::max(Rmax, R[k]);
    }
    if (regions > 0 && !edges) return refuse(NMRFIT_E_INVALID, std::string(who) + ": null pointer (edges)");
    for (int64_t i = 0; i < 2 * regions; ++i)
        if (std::isnan(edges[i]))
            return refuse(NMRFIT_E_INVALID, std::string(who) + ": a region's edge is NaN (region " + std::to_string(i / 2) + ")");
    if (K > kWeightsMaxSpectra || too_long || points > kWeightsMaxPoints)
        return refuse(NMRFIT_E_UNSUPPORTED, std::string(who) + ": a call takes at most " + std::to_string(kWeightsMaxSpectra) +
                                                " fits and " + std::to_string(kWeightsMaxPoints) + " grid points (summed over the fits)");
    if (Rmax > kQualityMaxRegions)
        return refuse(NMRFIT_E_UNSUPPORTED, std::string(who) + ": at most " + std::to_string(kQualityMaxRegions) + " regions per fit");
    *n_points = points;
    *n_regions = regions;
    return NMRFIT_OK;
}

int launch_quality(hipStream_t st, const QualityJob *jobs, int32_t K, int64_t max_tiles, int32_t Pmax, int32_t Rmax,
                   const WeightSpec *specs, const int32_t *region_spec, int64_t n_regions, const double *w_plain,
                   const double *edges, int64_t *first_last)
{
    int rc = launch_weights_nearest(st, specs, region_spec, n_regions, w_plain, edges, first_last);
    if (rc != NMRFIT_OK) return rc;
    const size_t lds = (size_t)std::max(Pmax, 1) * sizeof(PeakLor) + (size_t)std::max(Rmax, 1) * 2 * sizeof(int);
    hipLaunchKernelGGL(quality_tiles_kernel, dim3((unsigned)max_tiles, (unsigned)K), dim3(kTile), lds, st, jobs);
    NMRFIT_HIP(hipGetLastError());
    const unsigned fold_blocks = (unsigned)(((int64_t)(Rmax + 2) * kQ + kTile - 1) / kTile);
    hipLaunchKernelGGL(quality_fold_kernel, dim3(fold_blocks, (unsigned)K), dim3(kTile), 0, st, jobs);
    NMRFIT_HIP(hipGetLastError());
    return NMRFIT_OK;
}

}  // namespace nmrfit

using namespace nmrfit;

#pragma GCC visibility push(default)   // the C-ABI: the only symbols the library exports (build.sh: -fvisibility=hidden)

int nmrfit_quality_stats(int device, int32_t K, const int64_t *N, const double *w, const double *u, const double *v,
                         const int32_t *P, const double *x, const int32_t *R, const double *edges, double *out)
{
    const char *who = "nmrfit_quality_stats";
    if (!w || !u || !v || !P || !x || !out) return refuse(NMRFIT_E_INVALID, std::string(who) + ": null pointer");
    int64_t n_points = 0, n_regions = 0;
    int rc = check_quality_args(who, K, N, R, edges, &n_points, &n_regions);
    if (rc != NMRFIT_OK) return rc;
    int64_t n_x = 0, n_rows = 0, n_partial = 0, max_tiles = 0;
    int32_t Pmax = 0, Rmax = 0;
    for (int32_t k = 0; k < K; ++k) {
        if (P[k] < 0 || P[k] > kMaxPeaks)
            return refuse(NMRFIT_E_INVALID, std::string(who) + ": every fit needs 0 <= P <= " + std::to_string(kMaxPeaks) + " (fit " +
                                                std::to_string(k) + ")");
        n_x += 4 + 3 * (int64_t)P[k];
        n_rows += R[k] + 2;
        n_partial += (int64_t)(R[k] + 2) * quality_tiles(N[k]);
        max_tiles = std::max(max_tiles, quality_tiles(N[k]));
        Pmax = std::max(Pmax, P[k]);
        Rmax = std::max(Rmax, R[k]);
    }
    std::vector<WeightSpec> specs;
    std::vector<int32_t> region_spec;
    weights_layout(K, N, R, &specs, &region_spec);
    if ((rc = use_device(device)) != NMRFIT_OK) return rc;
    StreamLease lease(device);
    NMRFIT_HIP(lease.take());
    hipStream_t st = lease.s;
    const size_t np = (size_t)n_points, nr = (size_t)n_regions, plane = np * sizeof(double);
    Scratch mem;   // one allocation for the call's buffers
    Carver c;
    const size_t o_jobs = c.take((size_t)K * sizeof(QualityJob)), o_specs = c.take(specs.size() * sizeof(WeightSpec));
    const size_t o_rs = c.take(nr * sizeof(int32_t)), o_fl = c.take(2 * nr * sizeof(int64_t)), o_edges = c.take(2 * nr * sizeof(double));
    const size_t o_in = c.take((3 * np + (size_t)n_x) * sizeof(double));   // [3][points] w, u, v, then the K parameter vectors
    const size_t o_partial = c.take((size_t)n_partial * kQualityRow * sizeof(double));
    const size_t o_out = c.take((size_t)n_rows * kQualityRow * sizeof(double));
    unsigned char *base = nullptr;
    NMRFIT_HIP(mem.alloc(&base, c.total));
    QualityJob *d_jobs = reinterpret_cast<QualityJob *>(base + o_jobs);
    WeightSpec *d_specs = reinterpret_cast<WeightSpec *>(base + o_specs);
    int32_t *d_rs = reinterpret_cast<int32_t *>(base + o_rs);
    int64_t *d_fl = reinterpret_cast<int64_t *>(base + o_fl);
    double *d_edges = reinterpret_cast<double *>(base + o_edges), *d_in = reinterpret_cast<double *>(base + o_in);
    double *d_partial = reinterpret_cast<double *>(base + o_partial), *d_out = reinterpret_cast<double *>(base + o_out);
    double *d_x = d_in + 3 * np;
    std::vector<QualityJob> jobs((size_t)K);
    int64_t at_x = 0, at_row = 0, at_partial = 0;
    for (int32_t k = 0; k < K; ++k) {
        const WeightSpec &sp = specs[(size_t)k];
        QualityJob &j = jobs[(size_t)k];
        j = QualityJob{};
        j.w = d_in + sp.x_off;
        j.u = d_in + np + sp.x_off;
        j.v = d_in + 2 * np + sp.x_off;
        j.x = d_x + at_x;
        j.first_last = d_fl + 2 * sp.r_off;
        j.partial = d_partial + at_partial * kQualityRow;
        j.out = d_out + at_row * kQualityRow;
        double lane_step, grid_dev;
        analyse_grid(w + sp.x_off, N[k], &j.w0, &j.wspan, &lane_step, &grid_dev);
        j.N = N[k];
        j.P = P[k];
        j.R = R[k];
        j.tiles = (int32_t)quality_tiles(N[k]);
        j.slotted = 0;
        at_x += 4 + 3 * (int64_t)P[k];
        at_row += R[k] + 2;
        at_partial += (int64_t)(R[k] + 2) * j.tiles;
    }
    // (pageable host memory: the copies have left the host arrays when hipMemcpyAsync returns)
    NMRFIT_HIP(hipMemcpyAsync(d_jobs, jobs.data(), jobs.size() * sizeof(QualityJob), hipMemcpyHostToDevice, st));
    NMRFIT_HIP(hipMemcpyAsync(d_specs, specs.data(), specs.size() * sizeof(WeightSpec), hipMemcpyHostToDevice, st));
    NMRFIT_HIP(hipMemcpyAsync(d_in, w, plane, hipMemcpyHostToDevice, st));
    NMRFIT_HIP(hipMemcpyAsync(d_in + np, u, plane, hipMemcpyHostToDevice, st));
    NMRFIT_HIP(hipMemcpyAsync(d_in + 2 * np, v, plane, hipMemcpyHostToDevice, st));
    NMRFIT_HIP(hipMemcpyAsync(d_x, x, (size_t)n_x * sizeof(double), hipMemcpyHostToDevice, st));
    if (nr) {
        NMRFIT_HIP(hipMemcpyAsync(d_rs, region_spec.data(), nr * sizeof(int32_t), hipMemcpyHostToDevice, st));
        NMRFIT_HIP(hipMemcpyAsync(d_edges, edges, 2 * nr * sizeof(double), hipMemcpyHostToDevice, st));
    }
    if ((rc = launch_quality(st, d_jobs, K, max_tiles, Pmax, Rmax, d_specs, d_rs, n_regions, d_in, d_edges, d_fl)) != NMRFIT_OK)
        return rc;
    return staged_d2h(device, st, out, d_out, (size_t)n_rows * kQualityRow * sizeof(double));
}

#pragma GCC visibility pop

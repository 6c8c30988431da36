// baseline.hip -- least-squares polynomial baselines and noise levels of many spectra on the GPU (opt-in;
// include/nmrfit_amd_baseline.h holds the definition): over a masked part of a grid, a polynomial of degree <= 8 in the
// Chebyshev basis of the masked points' own domain, the normal equations summed in a fixed order and solved by
// L D L^T, the baseline at every grid point and the spread of the residual over the mask.
//   baseline_jobs_kernel<DC>       a workgroup of 256 threads per job (spectrum, channel), every pass inside the one
//                                  launch: mask / n / min / max, the 3 d + 2 sums, the solve (one lane, in LDS), the
//                                  baseline with S1, then S2.  DC: the launch's degree class (2, 4 or 8 >= every job's
//                                  degree): a lane carries 3 DC + 2 running sums in registers; a sum does not depend on DC
//   baseline_residual_kernel       y_j = d_j - V_j of the fits of a batch part into a plane in plain index order, V_j
//                                  and d_j by the functions result.hip evaluates them with (result_point.h)
// No atomics, no scratch memory; every value is a pure function of (w, y, mask, d).
#include "batch_part.h"
#include "nmrfit_amd_baseline.h"
#include "result_point.h"
#include "weights_internal.h"

#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

namespace nmrfit {
namespace {

#pragma clang fp contract(off)   // (every product of the definition is rounded; the shared per-point functions keep their own setting)

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / kWave;
constexpr int kMaxDeg = NMRFIT_BASELINE_MAX_DEG;
constexpr int kRow = NMRFIT_BASELINE_ROW;
constexpr int32_t kMaxIntervals = NMRFIT_BASELINE_MAX_INTERVALS;
constexpr int kMaxSums = 3 * kMaxDeg + 2;
static_assert(kRow == 8 + kMaxDeg + 1, "a row is 8 numbers and the coefficients");

// One job of a launch.  Every pointer is device memory.
struct BaselineJob {
    const double *w;       // the spectrum's grid, plain order, N points
    const double *y;       // the job's values, plain order
    const double *edges;   // the spectrum's R pairs
    double *row;           // [kRow]
    double *baseline;      // [N], or null
    int32_t N, R, deg, complement;
};

// One fit of a residual gather: the resident planes (grid_slot order), the parameter vector, where y goes.
struct ResidualJob {
    const double *wc, *u, *v, *x;
    double *y;
    double w0, wspan;
    int32_t N, P;
};

__device__ __forceinline__ bool masked(const double *__restrict__ ed, int R, bool complement, double wj)
{
    bool in = false;
    for (int r = 0; r < R; ++r) in = in || (ed[2 * r] <= wj && wj <= ed[2 * r + 1]);
    return (wj == wj) && (complement ? !in : in);
}

__device__ __forceinline__ double domain_t(double wj, double a, double b, double span)
{
    return span == 0.0 ? 0.0 : ((wj - a) - (b - wj)) / span;
}

// the waves' lane-0 values of `n_sums` sums meet in LDS: ((wave 0 + wave 1) + wave 2) + wave 3 into total[]
__device__ __forceinline__ void fold_waves(double (*part)[kMaxSums], double *total, int n_sums)
{
    __syncthreads();
    if ((int)threadIdx.x < n_sums) {
        double t = part[0][threadIdx.x];
        for (int wv = 1; wv < kWaves; ++wv) t += part[wv][threadIdx.x];
        total[threadIdx.x] = t;
    }
    __syncthreads();
}

// b_j from the coefficients in LDS: c_0, then + c_i T_i(t) for i = 1 .. d
__device__ __forceinline__ double baseline_at(const double *__restrict__ c, int d, double t)
{
    double b = c[0];
    double tk1 = 1.0, tk = t;   // T_{i-1}, T_i
    const double t2 = 2.0 * t;
    for (int i = 1; i <= d; ++i) {
        b = b + c[i] * tk;
        const double next = t2 * tk - tk1;
        tk1 = tk;
        tk = next;
    }
    return b;
}

template <int DC>
__global__ __launch_bounds__(kThreads) void baseline_jobs_kernel(const BaselineJob *__restrict__ jobs, int K)
{
    constexpr int kMu = 2 * DC + 1, kG = DC + 1;
    __shared__ double s_edges[2 * kMaxIntervals];
    __shared__ double s_part[kWaves][kMaxSums];
    __shared__ double s_tot[kMaxSums];
    __shared__ double s_G[(kMaxDeg + 1) * (kMaxDeg + 1)];   // G, overwritten column by column with L
    __shared__ double s_D[kMaxDeg + 1], s_v[kMaxDeg + 1], s_c[kMaxDeg + 1];
    __shared__ double s_lo[kWaves], s_hi[kWaves];
    __shared__ int s_n[kWaves];
    __shared__ int s_status;

    const BaselineJob &q = jobs[(int)blockIdx.y * K + (int)blockIdx.x];
    const int N = q.N, d = q.deg;
    const int R = min(q.R, kMaxIntervals);   // (the host refuses more)
    const bool complement = q.complement != 0;
    const double *__restrict__ w = q.w;
    const double *__restrict__ y = q.y;
    const int lane = threadIdx.x % kWave, wave = threadIdx.x / kWave;

    for (int r = threadIdx.x; r < R; r += kThreads) {
        const double e0 = q.edges[2 * r], e1 = q.edges[2 * r + 1];
        s_edges[2 * r] = e0 <= e1 ? e0 : e1;
        s_edges[2 * r + 1] = e0 <= e1 ? e1 : e0;
    }
    __syncthreads();

    // pass 1: n, a, b (exact whatever the order)
    int n_l = 0;
    double lo = INFINITY, hi = -INFINITY;
    for (int j = threadIdx.x; j < N; j += kThreads) {
        const double wj = w[j];
        if (masked(s_edges, R, complement, wj)) {
            ++n_l;
            lo = fmin(lo, wj);
            hi = fmax(hi, wj);
        }
    }
    for (int o = kWave / 2; o > 0; o >>= 1) {
        n_l += __shfl_xor(n_l, o);
        lo = fmin(lo, __shfl_xor(lo, o));
        hi = fmax(hi, __shfl_xor(hi, o));
    }
    if (lane == 0) {
        s_n[wave] = n_l;
        s_lo[wave] = lo;
        s_hi[wave] = hi;
    }
    __syncthreads();
    int n = 0;
    double a = INFINITY, b = -INFINITY;
    for (int wv = 0; wv < kWaves; ++wv) {
        n += s_n[wv];
        a = fmin(a, s_lo[wv]);
        b = fmax(b, s_hi[wv]);
    }
    const double nan = __builtin_nan("");
    int status = n == 0 ? 1 : (n < d + 1 ? 2 : 0);
    const double span = b - a;

    if (status == 0) {
        // pass 2: the sums mu_0 .. mu_2d and g_0 .. g_d, one running sum each per lane (the class's sums beyond the
        // job's degree are formed and not read)
        double mu[kMu], g[kG];
#pragma unroll
        for (int k = 0; k < kMu; ++k) mu[k] = 0.0;
#pragma unroll
        for (int k = 0; k < kG; ++k) g[k] = 0.0;
        for (int j = threadIdx.x; j < N; j += kThreads) {
            const double wj = w[j], yj = y[j];
            const bool m = masked(s_edges, R, complement, wj);
            const double t = domain_t(wj, a, b, span), t2 = 2.0 * t;
            double tk1 = 1.0, tk = t;
            mu[0] += m ? 1.0 : 0.0;
            g[0] += m ? 1.0 * yj : 0.0;
#pragma unroll
            for (int k = 1; k < kMu; ++k) {
                mu[k] += m ? tk : 0.0;
                if (k < kG) g[k] += m ? tk * yj : 0.0;
                const double next = t2 * tk - tk1;
                tk1 = tk;
                tk = next;
            }
        }
#pragma unroll
        for (int k = 0; k < kMu; ++k) {
            const double s = wave_sum(mu[k]);
            if (lane == 0) s_part[wave][k] = s;
        }
#pragma unroll
        for (int k = 0; k < kG; ++k) {
            const double s = wave_sum(g[k]);
            if (lane == 0) s_part[wave][kMu + k] = s;
        }
        fold_waves(s_part, s_tot, kMu + kG);

        // the solve, by one lane, in LDS (indices are run-time values: no register arrays, no scratch memory)
        if (threadIdx.x == 0) {
            const int ld = kMaxDeg + 1;
            for (int i = 0; i <= d; ++i)
                for (int k = 0; k <= i; ++k) s_G[i * ld + k] = 0.5 * (s_tot[i + k] + s_tot[i - k]);
            int st = 0;
            for (int j = 0; j <= d && st == 0; ++j) {
                for (int k = 0; k < j; ++k) s_v[k] = s_G[j * ld + k] * s_D[k];
                double s = s_G[j * ld + j];
                for (int k = 0; k < j; ++k) s = s - s_G[j * ld + k] * s_v[k];
                s_D[j] = s;
                if (!(s > 0.0)) {
                    st = 2;
                    break;
                }
                for (int i = j + 1; i <= d; ++i) {
                    double r = s_G[i * ld + j];
                    for (int k = 0; k < j; ++k) r = r - s_G[i * ld + k] * s_v[k];
                    s_G[i * ld + j] = r / s;
                }
            }
            if (st == 0) {
                double *z = s_v;
                for (int i = 0; i <= d; ++i) {
                    double r = s_tot[kMu + i];
                    for (int k = 0; k < i; ++k) r = r - s_G[i * ld + k] * z[k];
                    z[i] = r;
                }
                for (int i = 0; i <= d; ++i) z[i] = z[i] / s_D[i];
                for (int i = d; i >= 0; --i) {
                    double r = z[i];
                    for (int k = i + 1; k <= d; ++k) r = r - s_G[k * ld + i] * s_c[k];
                    s_c[i] = r;
                }
                double dmin = s_D[0], dmax = s_D[0];
                for (int i = 1; i <= d; ++i) {
                    dmin = fmin(dmin, s_D[i]);
                    dmax = fmax(dmax, s_D[i]);
                }
                s_tot[0] = dmin / dmax;
            }
            s_status = st;
        }
        __syncthreads();
        status = s_status;
    }

    double *__restrict__ out = q.baseline;
    if (status != 0) {   // (uniform over the workgroup)
        if (out)
            for (int j = threadIdx.x; j < N; j += kThreads) out[j] = nan;
        if (threadIdx.x == 0) {
            double *row = q.row;
            row[0] = (double)status;
            row[1] = (double)n;
            row[2] = n ? a : nan;
            row[3] = n ? b : nan;
            row[4] = row[5] = row[6] = nan;
            row[7] = (double)d;
            for (int i = 0; i <= kMaxDeg; ++i) row[8 + i] = i <= d ? nan : 0.0;
        }
        return;
    }
    const double ratio = s_tot[0];

    // pass 3: the baseline at every point, S1 over the mask
    double s1 = 0.0;
    for (int j = threadIdx.x; j < N; j += kThreads) {
        const double wj = w[j];
        const double bj = baseline_at(s_c, d, domain_t(wj, a, b, span));
        if (out) out[j] = bj;
        s1 += masked(s_edges, R, complement, wj) ? y[j] - bj : 0.0;
    }
    s1 = wave_sum(s1);
    if (lane == 0) s_part[wave][0] = s1;
    fold_waves(s_part, s_tot, 1);
    const double S1 = s_tot[0];
    const double rbar = S1 / (double)n;

    // pass 4: S2 about the mean (the baseline again, from the same operands: the same bits)
    double s2 = 0.0;
    for (int j = threadIdx.x; j < N; j += kThreads) {
        const double wj = w[j];
        const double bj = baseline_at(s_c, d, domain_t(wj, a, b, span));
        const double dev = (y[j] - bj) - rbar;
        s2 += masked(s_edges, R, complement, wj) ? dev * dev : 0.0;
    }
    s2 = wave_sum(s2);
    if (lane == 0) s_part[wave][0] = s2;
    fold_waves(s_part, s_tot, 1);
    if (threadIdx.x == 0) {
        double *row = q.row;
        row[0] = 0.0;
        row[1] = (double)n;
        row[2] = a;
        row[3] = b;
        row[4] = S1;
        row[5] = s_tot[0];
        row[6] = ratio;
        row[7] = (double)d;
        for (int i = 0; i <= kMaxDeg; ++i) row[8 + i] = i <= d ? s_c[i] : 0.0;
    }
}

// y_j = d_j - V_j of fit blockIdx.y, a thread per point, into the fit's stretch of a plane in plain index order
__global__ __launch_bounds__(kThreads) void baseline_residual_kernel(const ResidualJob *__restrict__ jobs)
{
    extern __shared__ __align__(16) unsigned char lds_raw[];
    const ResidualJob &q = jobs[blockIdx.y];
    if ((int64_t)blockIdx.x * kThreads >= q.N) return;   // (the fits of a launch may differ in length: whole workgroups leave)
    PeakLor *recs = reinterpret_cast<PeakLor *>(lds_raw);
    const double *__restrict__ x = q.x;
    stage_peak_records<kThreads>(recs, x, q.P, q.w0, q.wspan);
    const int j = (int)blockIdx.x * kThreads + (int)threadIdx.x;
    if (j >= q.N) return;
    const int64_t at = grid_slot(j);
    double V, dV, dI;
    point_lines<false>(recs, q.P, q.wc[at], x[3], nullptr, nullptr, 0, &V, nullptr);
    point_data(q.u[at], q.v[at], x[0], x[1], j, q.N, &dV, &dI);
    q.y[j] = dV - V;
}

int launch_baseline_jobs(hipStream_t st, const BaselineJob *jobs, int32_t K, int32_t C, int32_t max_deg)
{
    const dim3 grid((unsigned)K, (unsigned)C), block(kThreads);
    if (max_deg <= 2) hipLaunchKernelGGL(baseline_jobs_kernel<2>, grid, block, 0, st, jobs, (int)K);
    else if (max_deg <= 4) hipLaunchKernelGGL(baseline_jobs_kernel<4>, grid, block, 0, st, jobs, (int)K);
    else hipLaunchKernelGGL(baseline_jobs_kernel<8>, grid, block, 0, st, jobs, (int)K);
    NMRFIT_HIP(hipGetLastError());
    return NMRFIT_OK;
}

// What both entry points check before any device work (include/nmrfit_amd_baseline.h).  *n_points, *n_intervals: the
// sums; *max_deg: the largest degree.
int check_baseline_args(const char *who, int32_t K, const int64_t *N, const int32_t *deg, const int32_t *R, const double *edges,
                        const int32_t *complement, int64_t *n_points, int64_t *n_intervals, int32_t *max_deg)
{
    if (K <= 0 || !N || !deg || !R || !complement)
        return refuse(NMRFIT_E_INVALID, std::string(who) + ": the number of spectra must be > 0 and N, deg, R, complement non-null");
    int64_t points = 0, intervals = 0;
    int32_t Rmax = 0, dmax = 0;
    bool too_long = false;
    for (int32_t k = 0; k < K; ++k) {
        if (N[k] <= 0 || R[k] < 0)
            return refuse(NMRFIT_E_INVALID, std::string(who) + ": every spectrum needs N > 0 and R >= 0 (spectrum " + std::to_string(k) + ")");
        if (deg[k] < 0 || deg[k] > kMaxDeg)
            return refuse(NMRFIT_E_INVALID, std::string(who) + ": a degree is 0 .. " + std::to_string(kMaxDeg) + " (spectrum " +
                                                std::to_string(k) + ")");
        if (N[k] > kWeightsMaxPoints || points > kWeightsMaxPoints) too_long = true;   // (and the sum cannot overflow)
        else points += N[k];
        intervals += R[k];
        Rmax = std::max(Rmax, R[k]);
        dmax = std::max(dmax, deg[k]);
    }
    if (intervals > 0 && !edges) return refuse(NMRFIT_E_INVALID, std::string(who) + ": null pointer (edges)");
    for (int64_t i = 0; i < 2 * intervals; ++i)
        if (std::isnan(edges[i]))
            return refuse(NMRFIT_E_INVALID, std::string(who) + ": an interval's edge is NaN (interval " + std::to_string(i / 2) + ")");
    if (K > kWeightsMaxSpectra || too_long || points > kWeightsMaxPoints)
        return refuse(NMRFIT_E_UNSUPPORTED, std::string(who) + ": a call takes at most " + std::to_string(kWeightsMaxSpectra) +
                                                " spectra and " + std::to_string(kWeightsMaxPoints) + " grid points (summed over the spectra)");
    if (Rmax > kMaxIntervals)
        return refuse(NMRFIT_E_UNSUPPORTED, std::string(who) + ": at most " + std::to_string(kMaxIntervals) + " intervals per spectrum");
    *n_points = points;
    *n_intervals = intervals;
    *max_deg = dmax;
    return NMRFIT_OK;
}

// The residual baselines of the fits of a part, enqueued on the part's stream: the parameter vectors (x: this part's
// share on the host, or null: the best rows), the gather launch, the job launch.  deg, R, complement, edges: this part's
// shares, already checked.  Every buffer is a piece of ONE block of `mem`, the caller's (it synchronises the stream
// before `mem` goes).  *d_rows, *d_base: the part's rows and baseline values in device memory (d_base null unless asked).
int part_residual_baseline_enqueue(BatchPart *b, const double *x, const int32_t *deg, const int32_t *R, const double *edges,
                                   const int32_t *complement, bool want_baseline, Scratch &mem, double **d_rows, double **d_base)
{
    int rc = x ? bind_batch(b) : bind_started(b, "nmrfit_batch_residual_baseline");
    if (rc != NMRFIT_OK) return rc;
    if (!x && (rc = flush_fold(b)) != NMRFIT_OK) return rc;   // (the tail launch leaves every fit's best row in d_bestx)
    const int32_t K = b->K;
    const size_t np = (size_t)b->noff[(size_t)K];
    size_t nr = 0;
    int32_t max_deg = 0;
    for (int32_t k = 0; k < K; ++k) {
        nr += (size_t)R[k];
        max_deg = std::max(max_deg, deg[k]);
    }
    Carver c;
    const size_t o_gather = c.take((size_t)K * sizeof(ResidualJob)), o_jobs = c.take((size_t)K * sizeof(BaselineJob));
    const size_t o_edges = c.take(2 * nr * sizeof(double)), o_x = c.take(x ? (size_t)b->Dsum * sizeof(double) : 0);
    const size_t o_y = c.take(np * sizeof(double)), o_rows = c.take((size_t)K * kRow * sizeof(double));
    const size_t o_base = c.take(want_baseline ? np * sizeof(double) : 0);
    unsigned char *base = nullptr;
    NMRFIT_HIP(mem.alloc(&base, c.total));
    ResidualJob *d_gather = reinterpret_cast<ResidualJob *>(base + o_gather);
    BaselineJob *d_jobs = reinterpret_cast<BaselineJob *>(base + o_jobs);
    double *d_edges = reinterpret_cast<double *>(base + o_edges), *d_x = reinterpret_cast<double *>(base + o_x);
    double *d_y = reinterpret_cast<double *>(base + o_y);
    *d_rows = reinterpret_cast<double *>(base + o_rows);
    *d_base = want_baseline ? reinterpret_cast<double *>(base + o_base) : nullptr;
    std::vector<ResidualJob> gather((size_t)K);
    std::vector<BaselineJob> jobs((size_t)K);
    size_t at_r = 0;
    for (int32_t k = 0; k < K; ++k) {
        const BatchFit &f = b->h_fits[(size_t)k];
        const int64_t off = b->noff[(size_t)k];
        gather[(size_t)k] = ResidualJob{f.wc, f.u, f.v, (x ? d_x : b->d_bestx) + b->boff[(size_t)k], d_y + off, f.w0, f.wspan,
                                        (int32_t)f.N, f.P};
        jobs[(size_t)k] = BaselineJob{b->d_w_plain + off, d_y + off, d_edges + 2 * at_r, *d_rows + (size_t)k * kRow,
                                      want_baseline ? *d_base + off : nullptr, (int32_t)f.N, R[k], deg[k], complement[k]};
        at_r += (size_t)R[k];
    }
    hipStream_t st = b->stream;
    // (pageable host memory: the copies have left the host arrays when hipMemcpyAsync returns)
    NMRFIT_HIP(hipMemcpyAsync(d_gather, gather.data(), gather.size() * sizeof(ResidualJob), hipMemcpyHostToDevice, st));
    NMRFIT_HIP(hipMemcpyAsync(d_jobs, jobs.data(), jobs.size() * sizeof(BaselineJob), hipMemcpyHostToDevice, st));
    if (x) NMRFIT_HIP(hipMemcpyAsync(d_x, x, (size_t)b->Dsum * sizeof(double), hipMemcpyHostToDevice, st));
    if (nr) NMRFIT_HIP(hipMemcpyAsync(d_edges, edges, 2 * nr * sizeof(double), hipMemcpyHostToDevice, st));
    const size_t lds = (size_t)std::max(b->Pmax, 1) * sizeof(PeakLor);
    const unsigned tiles = (unsigned)((b->Nmax + kThreads - 1) / kThreads);
    hipLaunchKernelGGL(baseline_residual_kernel, dim3(tiles, (unsigned)K), dim3(kThreads), lds, st, d_gather);
    NMRFIT_HIP(hipGetLastError());
    return launch_baseline_jobs(st, d_jobs, K, 1, max_deg);
}

}  // namespace
}  // namespace nmrfit

using namespace nmrfit;

#pragma GCC visibility push(default)   // the C-ABI: the only symbols the library exports (build.sh: -fvisibility=hidden)

int nmrfit_baseline_fit(int device, int32_t K, const int64_t *N, const double *w, int32_t C, const double *y, const int32_t *deg,
                        const int32_t *R, const double *edges, const int32_t *complement, double *rows_out, double *baseline_out)
{
    const char *who = "nmrfit_baseline_fit";
    if (!w || !y || !rows_out) return refuse(NMRFIT_E_INVALID, std::string(who) + ": null pointer");
    if (C != 1 && C != 2) return refuse(NMRFIT_E_INVALID, std::string(who) + ": the number of channels is 1 or 2");
    int64_t n_points = 0, n_intervals = 0;
    int32_t max_deg = 0;
    int rc = check_baseline_args(who, K, N, deg, R, edges, complement, &n_points, &n_intervals, &max_deg);
    if (rc != NMRFIT_OK) return rc;
    if ((rc = use_device(device)) != NMRFIT_OK) return rc;
    StreamLease lease(device);
    NMRFIT_HIP(lease.take());
    hipStream_t st = lease.s;
    const size_t np = (size_t)n_points, nr = (size_t)n_intervals, nc = (size_t)C, plane = np * sizeof(double);
    Scratch mem;   // one allocation for the call's buffers
    Carver c;
    const size_t o_jobs = c.take(nc * (size_t)K * sizeof(BaselineJob)), o_edges = c.take(2 * nr * sizeof(double));
    const size_t o_w = c.take(plane), o_y = c.take(nc * plane), o_rows = c.take(nc * (size_t)K * kRow * sizeof(double));
    const size_t o_base = c.take(baseline_out ? nc * plane : 0);
    unsigned char *base = nullptr;
    NMRFIT_HIP(mem.alloc(&base, c.total));
    BaselineJob *d_jobs = reinterpret_cast<BaselineJob *>(base + o_jobs);
    double *d_edges = reinterpret_cast<double *>(base + o_edges), *d_w = reinterpret_cast<double *>(base + o_w);
    double *d_y = reinterpret_cast<double *>(base + o_y), *d_rows = reinterpret_cast<double *>(base + o_rows);
    double *d_base = baseline_out ? reinterpret_cast<double *>(base + o_base) : nullptr;
    std::vector<BaselineJob> jobs(nc * (size_t)K);
    for (size_t ch = 0; ch < nc; ++ch) {
        size_t off = 0, at_r = 0;
        for (int32_t k = 0; k < K; ++k) {
            const size_t i = ch * (size_t)K + (size_t)k;
            jobs[i] = BaselineJob{d_w + off, d_y + ch * np + off, d_edges + 2 * at_r, d_rows + i * kRow,
                                  d_base ? d_base + ch * np + off : nullptr, (int32_t)N[k], R[k], deg[k], complement[k]};
            off += (size_t)N[k];
            at_r += (size_t)R[k];
        }
    }
    // (pageable host memory: the copies have left the host arrays when hipMemcpyAsync returns)
    NMRFIT_HIP(hipMemcpyAsync(d_jobs, jobs.data(), jobs.size() * sizeof(BaselineJob), hipMemcpyHostToDevice, st));
    NMRFIT_HIP(hipMemcpyAsync(d_w, w, plane, hipMemcpyHostToDevice, st));
    NMRFIT_HIP(hipMemcpyAsync(d_y, y, nc * plane, hipMemcpyHostToDevice, st));
    if (nr) NMRFIT_HIP(hipMemcpyAsync(d_edges, edges, 2 * nr * sizeof(double), hipMemcpyHostToDevice, st));
    if ((rc = launch_baseline_jobs(st, d_jobs, K, C, max_deg)) != NMRFIT_OK) return rc;
    if ((rc = staged_d2h(device, st, rows_out, d_rows, nc * (size_t)K * kRow * sizeof(double))) != NMRFIT_OK) return rc;
    if (baseline_out) return staged_d2h(device, st, baseline_out, d_base, nc * plane);
    return NMRFIT_OK;
}

int nmrfit_batch_residual_baseline(nmrfit_batch *b, const double *x, const int32_t *deg, const int32_t *R, const double *edges,
                                   const int32_t *complement, double *rows_out, double *baseline_out)
{
    const char *who = "nmrfit_batch_residual_baseline";
    int rc = check_batch_handle(b);
    if (rc != NMRFIT_OK) return rc;
    if (!rows_out) return refuse(NMRFIT_E_INVALID, std::string(who) + ": null pointer");
    std::vector<int64_t> N((size_t)b->K);
    for (int32_t k = 0; k < b->K; ++k) N[(size_t)k] = b->noff[(size_t)k + 1] - b->noff[(size_t)k];
    int64_t n_points = 0, n_intervals = 0;
    int32_t max_deg = 0;
    if ((rc = check_baseline_args(who, b->K, N.data(), deg, R, edges, complement, &n_points, &n_intervals, &max_deg)) != NMRFIT_OK)
        return rc;
    if (!x && (rc = check_idle(b, who)) != NMRFIT_OK) return rc;
    // every part enqueues its launches on its own stream; then the rows (and the baselines) come back part after part
    // and all streams are waited for, before `mem` frees what the launches write.  A part's share of x, deg, R,
    // complement, edges and the outputs starts where the fits before it end.
    Scratch mem;
    std::vector<double *> d_rows(b->parts.size(), nullptr), d_base(b->parts.size(), nullptr);
    int64_t r0 = 0;
    for (size_t p = 0; p < b->parts.size() && rc == NMRFIT_OK; ++p) {
        const int32_t f0 = b->first[p], f1 = b->first[p + 1];
        rc = part_residual_baseline_enqueue(b->parts[p], x ? x + b->boff[(size_t)f0] : nullptr, deg + f0, R + f0,
                                            edges ? edges + 2 * r0 : nullptr, complement + f0, baseline_out != nullptr, mem, &d_rows[p],
                                            &d_base[p]);
        for (int32_t k = f0; k < f1; ++k) r0 += R[k];
    }
    for (size_t p = 0; p < b->parts.size(); ++p) {
        BatchPart *q = b->parts[p];
        const int32_t f0 = b->first[p], f1 = b->first[p + 1];
        if (rc == NMRFIT_OK && d_rows[p])
            rc = staged_d2h(q->device, q->stream, rows_out + (size_t)f0 * kRow, d_rows[p], (size_t)(f1 - f0) * kRow * sizeof(double));
        if (rc == NMRFIT_OK && d_base[p])
            rc = staged_d2h(q->device, q->stream, baseline_out + b->noff[(size_t)f0], d_base[p],
                            (size_t)(b->noff[(size_t)f1] - b->noff[(size_t)f0]) * sizeof(double));
        const hipError_t e = hipStreamSynchronize(q->stream);
        if (rc == NMRFIT_OK && e != hipSuccess) rc = hip_fail(e, "hipStreamSynchronize(residual baseline)", __FILE__, __LINE__);
    }
    return rc;
}

#pragma GCC visibility pop

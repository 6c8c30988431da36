// peaks.hip -- automatic peak picking on the GPU (opt-in): AutoPeakSelector(w, V, thresh, window).find_peaks() of the
// reference (nmrfit/utils.py:670-783, called by Data.select_peaks, nmrfit/containers.py:132-173) for a batch of
// spectra of any lengths.  Three launches:
//   1. peaks_smooth_kernel     the 100x upsampled grid W, U = interp1d(w, u)(W) (numpy.interp's arithmetic, which is
//                              what scipy's linear interp1d calls) and S = savgol_filter(U, 11, 4) inside; the five
//                              edge values at each end come from the caller (scipy fits them with a polynomial)
//   2. peaks_baseline_kernel   the global baseline peakutils.baseline(S, 0)[0], one workgroup per spectrum
//   3. peaks_pick_kernel       one wave per slot of (order + 1) points: the slot's strict maximum, the threshold, the
//                              argrelmax window, the half-height crossings, the local baseline and Simpson's area
// W, U, S, the crossings, width, bounds and the index range are exact restatements (contraction off).  The means of the
// baselines and the area's sum are compensated sums in a fixed order that depends on the spectrum alone (the host's
// pinv @ y and np.sum orders cannot be restated): a spectrum's values are bit-identical alone or in any batch.  No
// atomics, no scratch; every loop is bounded (the baselines stop after 100 passes, NaN spectra included).
#include "host_call.h"
#include "nmrfit_amd_diag.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

namespace nmrfit {
namespace {

#pragma clang fp contract(off)

constexpr int kSmoothThreads = 256;
constexpr int kHalo = 5;                      // savgol_filter(., 11, 4): 5 points each side
constexpr int kBaseThreads = 1024;            // stage 2: one workgroup per spectrum
constexpr int kPickWaves = 4;                 // stage 3: one wave per slot, four slots per workgroup
constexpr int kBaselineMaxIt = 100;           // peakutils.baseline: max_it
constexpr double kBaselineTol = 1e-3;         // ... tol
constexpr int64_t kUpsample = 100;            // utils.py: np.linspace(w.min(), w.max(), len(w) * 100)
constexpr int64_t kPointBudget = (int64_t)1 << 26;   // upsampled points per call (U and S: 1 GiB of device memory)

// scipy.signal.savgol_coeffs(11, 4)[5:] bit for bit (the filter is not exactly symmetric: the interior is
// U[i] c[5] + sum_{k=5..1} (U[i+k] + U[i-k]) c[5+k], which reproduces savgol_filter's interior exactly)
__constant__ double kSavgol[6] = {0x1.55555555556b4p-2, 0x1.1e6efe35b4e24p-2, 0x1.1e6efe35b4e26p-3,
                                  -0x1.7de952f2467e3p-6, -0x1.ada67d508f524p-4, 0x1.57b8644072a7ep-5};

struct PeakSpec {
    int64_t x_off;     // the spectrum's N sorted abscissae / ordinates in xs, ys
    int64_t N;
    int64_t m_off;     // its M = 100 N upsampled points in U, S
    int64_t M;
    int64_t slot_off;  // its slots: (M - 1) / (order + 1) + 1 from slot_off
    int64_t nslot;
    int64_t order;
    double wmin, wmax, thresh;
};

// np.linspace(wmin, wmax, M)[k]: k step + wmin, the last point wmax; a step that rounds to 0 takes (k / div) delta
__device__ __forceinline__ double grid_at(const PeakSpec &sp, int64_t k)
{
    if (k == sp.M - 1) return sp.wmax;
    const double delta = sp.wmax - sp.wmin, div = (double)(sp.M - 1);
    const double step = delta / div;
    if (step == 0.0) return ((double)k / div) * delta + sp.wmin;
    return (double)k * step + sp.wmin;
}

// numpy.interp(x, xs, ys) for xs[0] <= x <= xs[N-1]; j0 <= j <= j1 bracket the answer j = #(xs <= x) - 1
__device__ double interp_at(const double *xs, const double *ys, int64_t N, double x, int64_t j0, int64_t j1)
{
    int64_t lo = j0, hi = j1;              // invariant: xs[lo] <= x (or lo == j0), answer in [lo, hi]
    while (lo < hi) {
        const int64_t mid = lo + (hi - lo + 1) / 2;
        if (xs[mid] <= x) lo = mid;
        else hi = mid - 1;
    }
    const int64_t j = lo;
    if (j >= N - 1) return ys[N - 1];
    if (xs[j] == x) return ys[j];
    const double slope = (ys[j + 1] - ys[j]) / (xs[j + 1] - xs[j]);
    double r = slope * (x - xs[j]) + ys[j];
    if (__builtin_isnan(r)) {
        r = slope * (x - xs[j + 1]) + ys[j + 1];
        if (__builtin_isnan(r) && ys[j] == ys[j + 1]) r = ys[j];
    }
    return r;
}

// j = #(xs <= x) - 1 over the whole spectrum, clamped to [0, N-1]
__device__ int64_t bracket(const double *xs, int64_t N, double x)
{
    int64_t lo = 0, hi = N - 1;
    while (lo < hi) {
        const int64_t mid = lo + (hi - lo + 1) / 2;
        if (xs[mid] <= x) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// stage 1: a workgroup per 256 points of one spectrum (blockIdx.y): U of its points and 5 either side into LDS, then S
__global__ __launch_bounds__(kSmoothThreads) void peaks_smooth_kernel(const PeakSpec *specs, const double *xs_all,
                                                                      const double *ys_all, const double *edges,
                                                                      double *U_all, double *S_all)
{
    __shared__ double u[kSmoothThreads + 2 * kHalo];
    __shared__ int64_t jb[2];
    const PeakSpec sp = specs[blockIdx.y];
    const int64_t k0 = (int64_t)blockIdx.x * kSmoothThreads;
    if (k0 >= sp.M) return;
    const double *xs = xs_all + sp.x_off, *ys = ys_all + sp.x_off;
    const int t = threadIdx.x;
    const int64_t p_first = std::max<int64_t>(k0 - kHalo, 0);
    const int64_t p_last = std::min<int64_t>(k0 + kSmoothThreads + kHalo, sp.M) - 1;
    if (t == 0) jb[0] = bracket(xs, sp.N, grid_at(sp, p_first));
    if (t == 1) jb[1] = bracket(xs, sp.N, grid_at(sp, p_last));
    __syncthreads();
    for (int q = t; q < kSmoothThreads + 2 * kHalo; q += kSmoothThreads) {
        const int64_t p = k0 - kHalo + q;
        u[q] = (p >= p_first && p <= p_last) ? interp_at(xs, ys, sp.N, grid_at(sp, p), jb[0], jb[1]) : 0.0;
    }
    __syncthreads();
    const int64_t k = k0 + t;
    if (k >= sp.M) return;
    const double *e = edges + 10 * (int64_t)blockIdx.y;
    double s;
    if (k < kHalo) {
        s = e[k];
    } else if (k >= sp.M - kHalo) {
        s = e[kHalo + (k - (sp.M - kHalo))];
    } else {
        const int c = t + kHalo;
        s = u[c] * kSavgol[0];
#pragma unroll
        for (int d = kHalo; d >= 1; --d) s = s + (u[c + d] + u[c - d]) * kSavgol[d];
    }
    U_all[sp.m_off + k] = u[t + kHalo];
    S_all[sp.m_off + k] = s;
}

// a compensated (Neumaier) running sum; `s` alone is the plain sum in the same order, kept where the total is not finite
struct CSum {
    double s = 0.0, c = 0.0;
    __device__ __forceinline__ void add(double v)
    {
        const double t = s + v;
        c = c + ((fabs(s) >= fabs(v)) ? ((s - t) + v) : ((v - t) + s));
        s = t;
    }
    __device__ __forceinline__ void merge(double os, double oc)
    {
        const double t = s + os;
        const double bb = t - s;
        const double err = (s - (t - bb)) + (os - bb);   // exact: symmetric in the two operands
        c = (c + oc) + err;
        s = t;
    }
    __device__ __forceinline__ double total() const { return __builtin_isfinite(s) ? s + c : s; }
};

__device__ __forceinline__ void wave_csum(CSum &a)
{
    for (int o = kWave / 2; o > 0; o >>= 1) {
        const double os = __shfl_xor(a.s, o), oc = __shfl_xor(a.c, o);
        a.merge(os, oc);
    }
}

struct WaveReduce {
    __device__ __forceinline__ void operator()(CSum &a) const { wave_csum(a); }
};

struct BlockReduce {
    double *lds;   // 2 x (blockDim / 64)
    __device__ __forceinline__ void operator()(CSum &a) const
    {
        wave_csum(a);
        const int lane = threadIdx.x % kWave, wave = threadIdx.x / kWave, nw = blockDim.x / kWave;
        __syncthreads();
        if (lane == 0) {
            lds[2 * wave] = a.s;
            lds[2 * wave + 1] = a.c;
        }
        __syncthreads();
        CSum r;
        r.s = lds[0];
        r.c = lds[1];
        for (int w = 1; w < nw; ++w) r.merge(lds[2 * w], lds[2 * w + 1]);
        a = r;
    }
};

// np.minimum: NaN if either is NaN
__device__ __forceinline__ double min_nan(double a, double b)
{
    if (__builtin_isnan(a) || __builtin_isnan(b)) return NAN;
    return b < a ? b : a;
}

// peakutils.baseline(y, 0)[0] (nmrfit_amd/peaks.py: baseline): c <- mean(min(y, c)) from c = 1.0 until
// |new - c| / |c| < tol (numpy's norm: sqrt(x * x)) or 100 passes; the result is the last ACCEPTED c, y[0] when the
// first test already passes.  The clip is the running minimum of the accepted c's (np.minimum(y, base) every pass).
// tid / nt: this thread's place among the threads that share the spectrum; red sums a CSum over them.
template <class Red>
__device__ double const_baseline(const double *y, int64_t n, int tid, int nt, const Red &red)
{
    double coef = 1.0, clip = INFINITY, out = y[0];
    for (int it = 0; it < kBaselineMaxIt; ++it) {
        CSum acc;
        for (int64_t k = tid; k < n; k += nt) acc.add(min_nan(y[k], clip));
        red(acc);
        const double mean = acc.total() / (double)n;
        const double d = mean - coef;
        if (sqrt(d * d) / sqrt(coef * coef) < kBaselineTol) break;
        coef = mean;
        out = mean;
        clip = min_nan(clip, mean);
    }
    return out;
}

// stage 2: the global baseline of every spectrum
__global__ __launch_bounds__(kBaseThreads) void peaks_baseline_kernel(const PeakSpec *specs, const double *S_all,
                                                                      double *base)
{
    __shared__ double lds[2 * (kBaseThreads / kWave)];
    const PeakSpec sp = specs[blockIdx.x];
    const double b = const_baseline(S_all + sp.m_off, sp.M, threadIdx.x, kBaseThreads, BlockReduce{lds});
    if (threadIdx.x == 0) base[blockIdx.x] = b;
}

// numpy's sign: 1, -1, 0, NaN
__device__ __forceinline__ double np_sign(double x)
{
    if (x > 0.0) return 1.0;
    if (x < 0.0) return -1.0;
    if (x == 0.0) return 0.0;
    return x;
}

// (d, j) pairs: the smaller distance, on a tie the lower index (np.argmin over np.abs(w[cross] - loc))
struct Near {
    double d;
    int64_t j;
};
__device__ __forceinline__ bool nearer(const Near &a, const Near &b) { return a.d < b.d || (a.d == b.d && a.j < b.j); }
__device__ __forceinline__ Near wave_nearest(Near a)
{
    for (int o = kWave / 2; o > 0; o >>= 1) {
        Near b{__shfl_xor(a.d, o), (int64_t)__shfl_xor((long long)a.j, o)};
        if (nearer(b, a)) a = b;
    }
    return a;
}

// scipy.integrate.simpson(y, x=x) of scipy 1.15.3 for y = U[lo..hi] - pb, x = W[lo..hi] (n points): the irregular
// composite rule over pairs of intervals, for even n the Cartwright correction of the last interval, n = 2 the trapezoid
__device__ double simpson_area(const PeakSpec &sp, const double *U, int64_t lo, int64_t n, double pb, int lane)
{
    if (n < 2) return 0.0;
    auto X = [&](int64_t q) { return grid_at(sp, lo + q); };
    auto Y = [&](int64_t q) { return U[lo + q] - pb; };
    if (n == 2) return 0.5 * (X(1) - X(0)) * (Y(1) + Y(0));
    const int64_t nterms = (n % 2 == 1) ? (n - 1) / 2 : (n - 2) / 2;   // pairs starting at 0, 2, ... (< n-2 or < n-3)
    CSum acc;
    for (int64_t m = lane; m < nterms; m += kWave) {
        const int64_t i = 2 * m;
        const double x0 = X(i), x1 = X(i + 1), x2 = X(i + 2);
        const double h0 = x1 - x0, h1 = x2 - x1;
        const double hsum = h0 + h1, hprod = h0 * h1;
        const double r = (h1 != 0.0) ? h0 / h1 : 0.0;
        const double inv = (r != 0.0) ? 1.0 / r : 0.0;
        const double q = (hprod != 0.0) ? hsum / hprod : 0.0;
        const double t = hsum / 6.0 * ((Y(i) * (2.0 - inv) + Y(i + 1) * (hsum * q)) + Y(i + 2) * (2.0 - r));
        acc.add(t);
    }
    wave_csum(acc);
    double result = acc.total();
    if (n % 2 == 0) {
        const double h0 = X(n - 2) - X(n - 3), h1 = X(n - 1) - X(n - 2);
        double den = 6.0 * (h1 + h0);
        const double alpha = (den != 0.0) ? (2.0 * (h1 * h1) + (3.0 * h0) * h1) / den : 0.0;
        den = 6.0 * h0;
        const double beta = (den != 0.0) ? (h1 * h1 + (3.0 * h0) * h1) / den : 0.0;
        den = (6.0 * h0) * (h0 + h1);
        const double eta = (den != 0.0) ? pow(h1, 3.0) / den : 0.0;
        result = result + ((alpha * Y(n - 1) + beta * Y(n - 2)) - eta * Y(n - 3));
    }
    return result;
}

// first k in [0, M) with W[k] >= v (M if none); W is non-decreasing
__device__ int64_t grid_lower_bound(const PeakSpec &sp, double v)
{
    int64_t lo = 0, hi = sp.M;
    while (lo < hi) {
        const int64_t mid = lo + (hi - lo) / 2;
        if (grid_at(sp, mid) >= v) hi = mid;
        else lo = mid + 1;
    }
    return lo;
}
// first k in [0, M) with W[k] > v (M if none)
__device__ int64_t grid_upper_bound(const PeakSpec &sp, double v)
{
    int64_t lo = 0, hi = sp.M;
    while (lo < hi) {
        const int64_t mid = lo + (hi - lo) / 2;
        if (grid_at(sp, mid) > v) hi = mid;
        else lo = mid + 1;
    }
    return lo;
}

// stage 3: one wave per slot [s (order + 1), (s + 1)(order + 1)) of a spectrum.  A strict maximum over +-order is the
// strict maximum of its slot (the slot lies inside its window), so a slot holds at most one: the wave finds the slot's
// strict maximum, tests it against the threshold and the rest of its window, then measures the peak (AutoPeakSelector.
// find_width).  out_idx: 3 per slot (i, first and last index of the bounds; i = -1: no peak); out_val: 5 per slot
// (loc, width, baseline, height, area).
__global__ __launch_bounds__(kPickWaves * kWave) void peaks_pick_kernel(const PeakSpec *specs, int32_t S,
                                                                        int64_t total_slots, const double *U_all,
                                                                        const double *S_all, const double *base,
                                                                        int64_t *out_idx, double *out_val)
{
    const int lane = threadIdx.x % kWave;
    const int64_t slot = (int64_t)blockIdx.x * kPickWaves + threadIdx.x / kWave;
    if (slot >= total_slots) return;
    int32_t lo_s = 0, hi_s = S - 1;          // the spectrum: last with slot_off <= slot
    while (lo_s < hi_s) {
        const int32_t mid = lo_s + (hi_s - lo_s + 1) / 2;
        if (specs[mid].slot_off <= slot) lo_s = mid;
        else hi_s = mid - 1;
    }
    const PeakSpec sp = specs[lo_s];
    const double *U = U_all + sp.m_off, *Sm = S_all + sp.m_off;
    const double B = base[lo_s];
    const int64_t M = sp.M, order = sp.order;
    int64_t *oi = out_idx + 3 * slot;
    double *ov = out_val + 5 * slot;
    if (lane == 0) oi[0] = -1;
    const int64_t b0 = (slot - sp.slot_off) * (order + 1), b1 = std::min<int64_t>(b0 + order + 1, M);
    // the slot's strict maximum (a tie for the largest value: none)
    double v = -INFINITY;
    int64_t vi = -1;
    bool tie = false;
    for (int64_t j = b0 + lane; j < b1; j += kWave) {
        const double x = Sm[j];
        if (vi < 0 || x > v) {
            v = x;
            vi = j;
            tie = false;
        } else if (x == v) {
            tie = true;
        }
    }
    for (int o = kWave / 2; o > 0; o >>= 1) {
        const double ov2 = __shfl_xor(v, o);
        const int64_t oi2 = (int64_t)__shfl_xor((long long)vi, o);
        const bool ot = __shfl_xor((int)tie, o) != 0;
        if (oi2 < 0) continue;
        if (vi < 0 || ov2 > v) {
            v = ov2;
            vi = oi2;
            tie = ot;
        } else if (ov2 == v) {
            tie = true;
        }
    }
    const int64_t i = (int64_t)__shfl((long long)vi, 0);   // (wave-uniform from here on)
    if (__shfl((int)tie, 0) || i < 1 || i > M - 2) return;
    const double h = U[i] - B;                      // AutoPeakSelector.find_maxima: u[i] - baseline > thresh
    if (!(h > sp.thresh)) return;
    // the rest of the window [i - order, i + order] (clipped at the ends)
    const double si = Sm[i];
    bool ok = true;
    const int64_t w0 = std::max<int64_t>(i - order, 0), w1 = std::min<int64_t>(i + order, M - 1);
    for (int64_t j = w0 + lane; j < b0; j += kWave) ok = ok && (si > Sm[j]);
    for (int64_t j = b1 + lane; j <= w1; j += kWave) ok = ok && (si > Sm[j]);
    if (!__all(ok)) return;
    // half-height crossings nearest to loc: side = sign(h/2 - (u - baseline)), cross[j] = side[j] - side[j+1]
    const double loc = grid_at(sp, i);
    const double h2 = h / 2.0;
    Near fall{INFINITY, INT64_MAX}, rise{INFINITY, INT64_MAX};
    // left of the peak (j = i, i-1, ..., 0): the distance grows (weakly) with every step, and on a tie the farther point
    // has the lower index, so go on until the farthest point of a chunk is strictly farther than both found
    for (int64_t base_j = i; base_j >= 0; base_j -= kWave) {
        const int64_t j = base_j - lane;
        Near f{INFINITY, INT64_MAX}, r{INFINITY, INT64_MAX};
        if (j >= 0) {
            const double cr = np_sign(h2 - (U[j] - B)) - np_sign(h2 - (U[j + 1] - B));
            const double d = fabs(grid_at(sp, j) - loc);
            if (cr < 0.0) f = Near{d, j};
            if (cr > 0.0) r = Near{d, j};
        }
        f = wave_nearest(f);
        r = wave_nearest(r);
        if (nearer(f, fall)) fall = f;
        if (nearer(r, rise)) rise = r;
        const int64_t jfar = base_j - (kWave - 1);
        if (jfar <= 0) break;
        const double dfar = fabs(grid_at(sp, jfar) - loc);
        if (dfar > fall.d && dfar > rise.d) break;
    }
    // right of the peak (j = i+1 .. M-2): a tie there loses to the lower index already found
    for (int64_t base_j = i + 1; base_j <= M - 2; base_j += kWave) {
        const int64_t jfirst_d = base_j;
        if (fabs(grid_at(sp, jfirst_d) - loc) >= fall.d && fabs(grid_at(sp, jfirst_d) - loc) >= rise.d) break;
        const int64_t j = base_j + lane;
        Near f{INFINITY, INT64_MAX}, r{INFINITY, INT64_MAX};
        if (j <= M - 2) {
            const double cr = np_sign(h2 - (U[j] - B)) - np_sign(h2 - (U[j + 1] - B));
            const double d = fabs(grid_at(sp, j) - loc);
            if (cr < 0.0) f = Near{d, j};
            if (cr > 0.0) r = Near{d, j};
        }
        f = wave_nearest(f);
        r = wave_nearest(r);
        if (nearer(f, fall)) fall = f;
        if (nearer(r, rise)) rise = r;
    }
    if (fall.j == INT64_MAX || rise.j == INT64_MAX) return;
    const double x_right = grid_at(sp, fall.j), x_left = grid_at(sp, rise.j);
    if (!(x_left < x_right)) return;
    const double width = x_right - x_left;
    const double bl = loc - 2.0 * width, bh = loc + 2.0 * width;
    const int64_t lo = grid_lower_bound(sp, bl), hi = grid_upper_bound(sp, bh) - 1;   // np.where((w >= bl) & (w <= bh))
    const int64_t n = hi - lo + 1;
    const double pb = const_baseline(U + lo, n, lane, kWave, WaveReduce{});
    const double area = simpson_area(sp, U, lo, n, pb, lane);
    if (lane == 0) {
        oi[0] = i;
        oi[1] = lo;
        oi[2] = hi;
        ov[0] = loc;
        ov[1] = width;
        ov[2] = pb;
        ov[3] = U[i] - pb;
        ov[4] = area;
    }
}

// ---- host side -------------------------------------------------------------------------------------------------------

// the batch's layout; order may be NULL (the diagnostic: no slots)
int plan(const char *who, int32_t S, const int64_t *N, const double *w, const double *u, const double *edges,
         const int64_t *order, const double *thresh, std::vector<PeakSpec> *specs)
{
    int rc = check_spectra_count(who, S);
    if (rc != NMRFIT_OK) return rc;
    if (!N || !w || !u || !edges) {
        set_error(std::string(who) + ": null pointer");
        return NMRFIT_E_INVALID;
    }
    specs->assign((size_t)S, PeakSpec{});
    int64_t x_off = 0, m_off = 0, slot_off = 0;
    for (int32_t k = 0; k < S; ++k) {
        const std::string at = " (spectrum " + std::to_string(k) + ")";
        if (N[k] < 2 || N[k] > kPointBudget / kUpsample) {
            set_error(std::string(who) + ": every spectrum needs 2 <= N <= " + std::to_string(kPointBudget / kUpsample) + at);
            return N[k] < 2 ? NMRFIT_E_INVALID : NMRFIT_E_UNSUPPORTED;
        }
        for (int64_t j = 1; j < N[k]; ++j)
            if (!(w[x_off + j - 1] <= w[x_off + j])) {
                set_error(std::string(who) + ": w must be sorted ascending (and not NaN)" + at);
                return NMRFIT_E_INVALID;
            }
        PeakSpec &sp = (*specs)[(size_t)k];
        sp.x_off = x_off;
        sp.N = N[k];
        sp.m_off = m_off;
        sp.M = kUpsample * N[k];
        sp.wmin = w[x_off];
        sp.wmax = w[x_off + N[k] - 1];
        if (order) {
            if (order[k] < 1) {
                set_error(std::string(who) + ": order must be >= 1" + at);
                return NMRFIT_E_INVALID;
            }
            sp.order = order[k];
            sp.nslot = (sp.M - 1) / (order[k] + 1) + 1;
            sp.slot_off = slot_off;
            sp.thresh = thresh[k];
            slot_off += sp.nslot;
        }
        x_off += N[k];
        m_off += sp.M;
        if (m_off > kPointBudget) {
            set_error(std::string(who) + ": a call takes at most " + std::to_string(kPointBudget) +
                      " upsampled points (100 N summed over the spectra)");
            return NMRFIT_E_UNSUPPORTED;
        }
    }
    return NMRFIT_OK;
}

// stages 1 (and 2, 3 with outputs): U, S stay on the device unless U_out / S_out are given
int run(int device, int32_t S, const std::vector<PeakSpec> &specs, const double *w, const double *u, const double *edges,
        double *U_out, double *S_out, double *baseline, int64_t *count, int64_t *peak_idx, double *peak_val)
{
    int rc = use_device(device);
    if (rc != NMRFIT_OK) return rc;
    StreamLease lease(device);
    NMRFIT_HIP(lease.take());
    hipStream_t st = lease.s;
    Scratch mem;
    const PeakSpec &last = specs.back();
    const size_t nx = (size_t)(last.x_off + last.N), nm = (size_t)(last.m_off + last.M);
    const int64_t nslots = last.slot_off + last.nslot;
    int64_t maxM = 0;
    for (const PeakSpec &sp : specs) maxM = std::max(maxM, sp.M);
    PeakSpec *d_specs = nullptr;
    double *d_x = nullptr, *d_y = nullptr, *d_e = nullptr, *d_U = nullptr, *d_S = nullptr, *d_b = nullptr, *d_val = nullptr;
    int64_t *d_idx = nullptr;
    NMRFIT_HIP(mem.alloc(&d_specs, specs.size()));
    NMRFIT_HIP(mem.alloc(&d_x, nx));
    NMRFIT_HIP(mem.alloc(&d_y, nx));
    NMRFIT_HIP(mem.alloc(&d_e, 10 * (size_t)S));
    NMRFIT_HIP(mem.alloc(&d_U, nm));
    NMRFIT_HIP(mem.alloc(&d_S, nm));
    NMRFIT_HIP(hipMemcpyAsync(d_specs, specs.data(), specs.size() * sizeof(PeakSpec), hipMemcpyHostToDevice, st));
    NMRFIT_HIP(hipMemcpyAsync(d_x, w, nx * sizeof(double), hipMemcpyHostToDevice, st));
    NMRFIT_HIP(hipMemcpyAsync(d_y, u, nx * sizeof(double), hipMemcpyHostToDevice, st));
    NMRFIT_HIP(hipMemcpyAsync(d_e, edges, 10 * (size_t)S * sizeof(double), hipMemcpyHostToDevice, st));
    const dim3 grid1((unsigned)((maxM + kSmoothThreads - 1) / kSmoothThreads), (unsigned)S);
    hipLaunchKernelGGL(peaks_smooth_kernel, grid1, dim3(kSmoothThreads), 0, st, d_specs, d_x, d_y, d_e, d_U, d_S);
    NMRFIT_HIP(hipGetLastError());
    if (U_out) {
        if ((rc = staged_d2h(device, st, U_out, d_U, nm * sizeof(double))) != NMRFIT_OK) return rc;
        return staged_d2h(device, st, S_out, d_S, nm * sizeof(double));
    }
    NMRFIT_HIP(mem.alloc(&d_b, (size_t)S));
    NMRFIT_HIP(mem.alloc(&d_idx, 3 * (size_t)nslots));
    NMRFIT_HIP(mem.alloc(&d_val, 5 * (size_t)nslots));
    hipLaunchKernelGGL(peaks_baseline_kernel, dim3((unsigned)S), dim3(kBaseThreads), 0, st, d_specs, d_S, d_b);
    NMRFIT_HIP(hipGetLastError());
    const int64_t blocks = (nslots + kPickWaves - 1) / kPickWaves;
    hipLaunchKernelGGL(peaks_pick_kernel, dim3((unsigned)blocks), dim3(kPickWaves * kWave), 0, st, d_specs, S, nslots,
                       d_U, d_S, d_b, d_idx, d_val);
    NMRFIT_HIP(hipGetLastError());
    std::vector<int64_t> idx(3 * (size_t)nslots);
    std::vector<double> val(5 * (size_t)nslots);
    NMRFIT_HIP(hipMemcpyAsync(baseline, d_b, (size_t)S * sizeof(double), hipMemcpyDeviceToHost, st));
    NMRFIT_HIP(hipMemcpyAsync(idx.data(), d_idx, idx.size() * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    NMRFIT_HIP(hipMemcpyAsync(val.data(), d_val, val.size() * sizeof(double), hipMemcpyDeviceToHost, st));
    NMRFIT_HIP(hipStreamSynchronize(st));
    // compaction: spectrum k's peaks, in index order, from the start of its slot range
    for (int32_t k = 0; k < S; ++k) {
        const PeakSpec &sp = specs[(size_t)k];
        int64_t c = 0;
        for (int64_t q = sp.slot_off; q < sp.slot_off + sp.nslot; ++q) {
            if (idx[3 * (size_t)q] < 0) continue;
            const size_t dst = (size_t)(sp.slot_off + c++);
            std::memcpy(peak_idx + 3 * dst, &idx[3 * (size_t)q], 3 * sizeof(int64_t));
            std::memcpy(peak_val + 5 * dst, &val[5 * (size_t)q], 5 * sizeof(double));
        }
        count[k] = c;
    }
    return NMRFIT_OK;
}

}  // namespace
}  // namespace nmrfit

using namespace nmrfit;

#pragma GCC visibility push(default)   // the C-ABI: the only symbols the library exports (build.sh: -fvisibility=hidden)

int nmrfit_peaks_pick(int device, int32_t S, const int64_t *N, const double *w, const double *u, const double *edges,
                      const int64_t *order, const double *thresh, double *baseline, int64_t *count, int64_t *peak_idx,
                      double *peak_val)
{
    const char *who = "nmrfit_peaks_pick";
    if (!order || !thresh || !baseline || !count || !peak_idx || !peak_val) {
        set_error(std::string(who) + ": null pointer");
        return NMRFIT_E_INVALID;
    }
    std::vector<PeakSpec> specs;
    int rc = plan(who, S, N, w, u, edges, order, thresh, &specs);
    if (rc != NMRFIT_OK) return rc;
    return run(device, S, specs, w, u, edges, nullptr, nullptr, baseline, count, peak_idx, peak_val);
}

int nmrfit_diag_peaks_smooth(int device, int32_t S, const int64_t *N, const double *w, const double *u,
                             const double *edges, double *U, double *Sm)
{
    const char *who = "nmrfit_diag_peaks_smooth";
    if (!U || !Sm) {
        set_error(std::string(who) + ": null pointer");
        return NMRFIT_E_INVALID;
    }
    std::vector<PeakSpec> specs;
    int rc = plan(who, S, N, w, u, edges, nullptr, nullptr, &specs);
    if (rc != NMRFIT_OK) return rc;
    return run(device, S, specs, w, u, edges, U, Sm, nullptr, nullptr, nullptr, nullptr);
}

#pragma GCC visibility pop

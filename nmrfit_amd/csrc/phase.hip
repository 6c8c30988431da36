// phase.hip -- automatic phase correction on the GPU (opt-in): the scores the reference's phase estimate minimises
// (nmrfit/proc_autophase.py:142-187 ACME, :190-219 peak minima), the per-angle test of Data._brute_phase
// (nmrfit/containers.py:98-110), and the whole of scipy.optimize.fmin over (p0, p1) in one workgroup per spectrum
// (proc_autophase.py:107-139: approximate_phase).
//
// A batch holds S spectra of any lengths one after the other (as nmrfit_batch_create_ragged lays them out).  Every
// score is a workgroup reduction in a fixed order that depends on N alone (phase_threads(N) threads take part; a launch
// sized for a longer spectrum leaves the others idle), so a spectrum's values are bit-identical run to run, alone or
// in any batch, in the score kernel or inside the optimiser.  No atomics.
//
// Every arithmetic step that restates numpy or scipy is written in their operation order with contraction off.
#include "host_call.h"
#include "nmrfit_amd_diag.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

namespace nmrfit {
namespace {

#pragma clang fp contract(off)

constexpr int kPhaseMaxThreads = 512;     // (1024-thread workgroups cap a thread at 128 VGPRs: the optimiser spilled)
constexpr int kPhaseMaxWaves = kPhaseMaxThreads / kWave;
constexpr int kMinimaWindow = 100;       // proc_autophase.py:217-218: real[i - 100:i], real[i:i + 100]
constexpr int kBruteMaxMeanTerms = 128;  // numpy's pairwise block (PW_BLOCKSIZE): one 8-accumulator block per mean
constexpr int kMaxFun = 400;             // fmin: maxiter = maxfun = 200 x len(x0)
enum { kScoreAcme = NMRFIT_PHASE_ACME, kScorePeakMinima = NMRFIT_PHASE_PEAK_MINIMA, kScoreBrute = NMRFIT_PHASE_BRUTE_LEVEL,
       kScoreRosenbrock = 3 };
enum { kStatusOk = 0, kStatusEmptyWindow = 1 };

// threads that evaluate a spectrum of N points (the reduction order follows from it)
__host__ __device__ inline int phase_threads(int64_t N) { return N >= 16384 ? 512 : 256; }

struct Spectrum {
    const double *u, *v;
    int64_t N;
};

struct Lds {
    double red[kPhaseMaxWaves * 3];
    int64_t idx[kPhaseMaxWaves];
    double win[2 * kMinimaWindow];
};

__device__ __forceinline__ double wave_sum(double x)
{
    for (int o = kWave / 2; o > 0; o >>= 1) x = x + __shfl_xor(x, o);   // (fp add commutes: every lane ends equal)
    return x;
}

// sum of K per-thread values over the first nt threads, in a fixed order; every thread gets the same result
template <int K>
__device__ __forceinline__ void block_sum(double (&val)[K], Lds &lds, int nt)
{
    const int lane = threadIdx.x % kWave, wave = threadIdx.x / kWave;
#pragma unroll
    for (int k = 0; k < K; ++k) val[k] = wave_sum(val[k]);
    __syncthreads();
    if (lane == 0)
#pragma unroll
        for (int k = 0; k < K; ++k) lds.red[wave * K + k] = val[k];
    __syncthreads();
    const int nw = nt / kWave;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        double s = lds.red[k];
        for (int w = 1; w < nw; ++w) s = s + lds.red[w * K + k];
        val[k] = s;
    }
}

// numpy's argmax order: the first NaN, else the first of the largest values
__device__ __forceinline__ void argmax_combine(double &va, int64_t &ia, double vb, int64_t ib)
{
    const bool na = __builtin_isnan(va), nb = __builtin_isnan(vb);
    bool take_b;
    if (na || nb) take_b = na ? (nb && ib < ia) : true;
    else take_b = vb > va || (vb == va && ib < ia);
    if (take_b) {
        va = vb;
        ia = ib;
    }
}

// np.min, np.max: NaN propagates
__device__ __forceinline__ double min_nan(double a, double b)
{
    if (__builtin_isnan(a)) return a;
    if (__builtin_isnan(b)) return b;
    return b < a ? b : a;
}
__device__ __forceinline__ double max_nan(double a, double b)
{
    if (__builtin_isnan(a)) return a;
    if (__builtin_isnan(b)) return b;
    return b > a ? b : a;
}

// real(apod * data) for apod = c + i s: numpy's complex multiply (its FMA loop on x86-64 with AVX2 / AVX-512 -- what
// the reference's goldens hold) rounds the real part as fma(c, u, -(s v)), not as c u - s v
__device__ __forceinline__ double rotate_real(double c, double s, double u, double v) { return __builtin_fma(c, u, -(s * v)); }

// the real part of ps(data, p0, p1) at point j: apod = exp(i (p0r + (p1r j) / N)) (proc_autophase.py:39-68)
__device__ __forceinline__ double phased_real(const Spectrum &sp, int64_t j, double p0r, double p1r, double Nd)
{
    const double theta = p0r + (p1r * (double)j) / Nd;
    double s, c;
    sincos(theta, &s, &c);
    return rotate_real(c, s, sp.u[j], sp.v[j]);
}

// ACME (proc_autophase.py:142-187) in two sweeps: T = sum ds and the penalty sums, then sum -p log p with p = ds / T.
// Work is cut into 64-point tiles that overlap by one point (63 slopes each): a lane's right neighbour comes from the
// next lane, and each point's rotation is computed once per sweep.
__device__ double score_acme(const Spectrum &sp, double p0, double p1, Lds &lds, int nt)
{
    const double pi = 3.141592653589793;
    const double p0r = p0 * pi / 180.0, p1r = p1 * pi / 180.0;
    const int64_t N = sp.N;
    const double Nd = (double)N;
    const int lane = threadIdx.x % kWave, wave = threadIdx.x / kWave, nw = nt / kWave;
    const int64_t ntiles = (N - 1 + (kWave - 2)) / (kWave - 1);
    double acc[3] = {0.0, 0.0, 0.0};   // sum ds, sum (r - |r|), sum ((r - |r|) / 2)^2
    for (int64_t t = wave; wave < nw && t < ntiles; t += nw) {
        const int64_t j = (kWave - 1) * t + lane;
        const double r = (j < N) ? phased_real(sp, j, p0r, p1r, Nd) : 0.0;
        const double rn = __shfl_down(r, 1);
        if (lane < kWave - 1 && j < N - 1) acc[0] = acc[0] + fabs((rn - r) / 2.0);
        if ((lane < kWave - 1 && j < N - 1) || j == N - 1) {
            const double neg = r - fabs(r);
            const double h = neg / 2.0;
            acc[1] = acc[1] + neg;
            acc[2] = acc[2] + h * h;
        }
    }
    if (wave >= nw) acc[0] = acc[1] = acc[2] = 0.0;
    block_sum<3>(acc, lds, nt);
    const double T = acc[0];
    double ent[1] = {0.0};
    for (int64_t t = wave; wave < nw && t < ntiles; t += nw) {
        const int64_t j = (kWave - 1) * t + lane;
        const double r = (j < N) ? phased_real(sp, j, p0r, p1r, Nd) : 0.0;
        const double rn = __shfl_down(r, 1);
        if (lane < kWave - 1 && j < N - 1) {
            const double p = fabs((rn - r) / 2.0) / T;
            if (!(p == 0.0)) ent[0] = ent[0] + (-p) * log(p);   // prob[prob == 0] = 1: the term is 0
        }
    }
    if (wave >= nw) ent[0] = 0.0;
    block_sum<1>(ent, lds, nt);
    const double penalty = (acc[1] < 0.0) ? acc[2] : 0.0;
    return ent[0] + 1000.0 * penalty;
}

// peak minima (proc_autophase.py:190-219): |min real[i-100:i] - min real[i:i+100]|, i = argmax(real).  *empty: the
// left slice is empty (numpy's np.min raises there).
__device__ double score_peak_minima(const Spectrum &sp, double p0, double p1, Lds &lds, int nt, bool *empty)
{
    const double pi = 3.141592653589793;
    const double p0r = p0 * pi / 180.0, p1r = p1 * pi / 180.0;
    const int64_t N = sp.N;
    const double Nd = (double)N;
    const int tid = threadIdx.x, lane = tid % kWave, wave = tid / kWave, nw = nt / kWave;
    double best = -INFINITY;
    int64_t bi = INT64_MAX;
    if (tid < nt)
        for (int64_t j = tid; j < N; j += nt) argmax_combine(best, bi, phased_real(sp, j, p0r, p1r, Nd), j);
    for (int o = kWave / 2; o > 0; o >>= 1) {
        const double vb = __shfl_xor(best, o);
        const int64_t ib = __shfl_xor(bi, o);
        argmax_combine(best, bi, vb, ib);
    }
    __syncthreads();
    if (lane == 0) {
        lds.red[wave] = best;
        lds.idx[wave] = bi;
    }
    __syncthreads();
    double v = lds.red[0];
    int64_t i = lds.idx[0];
    for (int w = 1; w < nw; ++w) argmax_combine(v, i, lds.red[w], lds.idx[w]);
    // python slicing of real[i - 100:i]: a negative start counts from the end, then clips at 0
    int64_t ls = i - kMinimaWindow;
    if (ls < 0) ls += N;
    if (ls < 0) ls = 0;
    const int64_t re = std::min<int64_t>(i + kMinimaWindow, N);
    *empty = !(ls < i);
    if (*empty) return NAN;
    if (tid < kMinimaWindow) {
        const int64_t j = ls + tid;
        lds.win[tid] = (j < i) ? phased_real(sp, j, p0r, p1r, Nd) : INFINITY;
    } else if (tid < 2 * kMinimaWindow) {
        const int64_t j = i + (tid - kMinimaWindow);
        lds.win[tid] = (j < re) ? phased_real(sp, j, p0r, p1r, Nd) : INFINITY;
    }
    __syncthreads();
    double ml = INFINITY, mr = INFINITY;
    for (int k = 0; k < kMinimaWindow; ++k) {
        ml = min_nan(ml, lds.win[k]);
        mr = min_nan(mr, lds.win[kMinimaWindow + k]);
    }
    return fabs(ml - mr);
}

// numpy's pairwise_sum for n <= 128 terms: plain left to right below 8, else eight accumulators + the tail
__device__ double numpy_block_sum(const Spectrum &sp, int64_t first, int64_t n, double c, double s)
{
    auto V = [&](int64_t k) { return rotate_real(c, s, sp.u[first + k], sp.v[first + k]); };
    if (n < 8) {
        double res = 0.0;
        for (int64_t k = 0; k < n; ++k) res = res + V(k);
        return res;
    }
    double r0 = V(0), r1 = V(1), r2 = V(2), r3 = V(3), r4 = V(4), r5 = V(5), r6 = V(6), r7 = V(7);
    int64_t k = 8;
    for (; k < n - (n % 8); k += 8) {
        r0 = r0 + V(k + 0);
        r1 = r1 + V(k + 1);
        r2 = r2 + V(k + 2);
        r3 = r3 + V(k + 3);
        r4 = r4 + V(k + 4);
        r5 = r5 + V(k + 5);
        r6 = r6 + V(k + 6);
        r7 = r7 + V(k + 7);
    }
    double res = ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7));
    for (; k < n; ++k) res = res + V(k);
    return res;
}

// the per-angle test of Data._brute_phase (containers.py:98-110) for the rotation factor (c, s) = exp(i angle):
// V = real(exp(i angle) (u + i v)); err = sqrt((mean(V[:n]) - mean(V[-n:]))^2); err where max(V) > |min(V)|, else NaN.
// n is the mean length the host takes from len(self.V) before its scan (not from N: select_bounds crops u, v and leaves
// V alone); python clips both slices at N, so the means are over min(n, N) points.
__device__ double score_brute(const Spectrum &sp, double c, double s, int64_t n_mean, Lds &lds, int nt)
{
    const int64_t N = sp.N;
    const int tid = threadIdx.x, lane = tid % kWave, wave = tid / kWave, nw = nt / kWave;
    double mx = -INFINITY, mn = INFINITY;
    if (tid < nt)
        for (int64_t j = tid; j < N; j += nt) {
            const double V = rotate_real(c, s, sp.u[j], sp.v[j]);
            mx = max_nan(mx, V);
            mn = min_nan(mn, V);
        }
    for (int o = kWave / 2; o > 0; o >>= 1) {
        mx = max_nan(mx, __shfl_xor(mx, o));
        mn = min_nan(mn, __shfl_xor(mn, o));
    }
    __syncthreads();
    if (lane == 0) {
        lds.red[2 * wave] = mx;
        lds.red[2 * wave + 1] = mn;
    }
    __syncthreads();
    mx = lds.red[0];
    mn = lds.red[1];
    for (int w = 1; w < nw; ++w) {
        mx = max_nan(mx, lds.red[2 * w]);
        mn = min_nan(mn, lds.red[2 * w + 1]);
    }
    const int64_t n = std::min<int64_t>(n_mean, N);
    const double nd = (double)n;
    const double d = numpy_block_sum(sp, 0, n, c, s) / nd - numpy_block_sum(sp, N - n, n, c, s) / nd;
    const double err = sqrt(d * d);
    return (mx > fabs(mn)) ? err : NAN;
}

__device__ __forceinline__ Spectrum spectrum_of(const double *u, const double *v, const int64_t *off, int k)
{
    Spectrum sp;
    sp.u = u + off[k];
    sp.v = v + off[k];
    sp.N = off[k + 1] - off[k];
    return sp;
}

// the brute level's mean length when the caller gives none: the host's n for a V as long as u
__host__ __device__ inline int64_t brute_default_mean(int64_t N) { return N / 5000 > 1 ? N / 5000 : 1; }

template <int KIND>
__device__ __forceinline__ double evaluate(const Spectrum &sp, double a, double b, Lds &lds, int nt, bool *empty,
                                           int64_t n_mean = 0)
{
    *empty = false;
    if (KIND == kScoreAcme) return score_acme(sp, a, b, lds, nt);
    if (KIND == kScorePeakMinima) return score_peak_minima(sp, a, b, lds, nt, empty);
    if (KIND == kScoreBrute) return score_brute(sp, a, b, n_mean, lds, nt);
    // the optimiser's test score: Rosenbrock, as python evaluates (1 - x)**2 + 100*(y - x**2)**2
    const double p = 1.0 - a, q = b - a * a;
    return p * p + 100.0 * (q * q);
}

// one score per (candidate, spectrum) workgroup: blockIdx.x = candidate, blockIdx.y = spectrum.  n_mean: the brute
// level's mean length per spectrum (null: brute_default_mean(N)); unused by the other scores.
template <int KIND>
__global__ __launch_bounds__(kPhaseMaxThreads) void phase_scores_kernel(const double *__restrict__ u, const double *__restrict__ v,
                                                                        const int64_t *__restrict__ off, int32_t M,
                                                                        const double *__restrict__ cand, double *__restrict__ score,
                                                                        int32_t *__restrict__ empty_out,
                                                                        const int64_t *__restrict__ n_mean)
{
    __shared__ Lds lds;
    const int k = blockIdx.y;
    const int64_t slot = (int64_t)k * M + blockIdx.x;
    const Spectrum sp = spectrum_of(u, v, off, k);
    const int nt = phase_threads(sp.N);
    bool empty = false;
    const int64_t n = KIND == kScoreBrute ? (n_mean ? n_mean[k] : brute_default_mean(sp.N)) : 0;
    const double f = evaluate<KIND>(sp, cand[2 * slot], cand[2 * slot + 1], lds, nt, &empty, n);
    if (threadIdx.x == 0) {
        score[slot] = f;
        empty_out[slot] = empty ? 1 : 0;
    }
}

// stable insertion sort of the three vertices by value, NaN last (np.argsort + np.take)
__device__ __forceinline__ bool nm_less(double a, double b) { return a < b || (!__builtin_isnan(a) && __builtin_isnan(b)); }

struct Vertex {
    double x, y, f;
};

__device__ __forceinline__ void vswap(Vertex &a, Vertex &b)
{
    const Vertex t = a;
    a = b;
    b = t;
}

__device__ __forceinline__ void nm_sort(Vertex &v0, Vertex &v1, Vertex &v2)
{
    if (nm_less(v1.f, v0.f)) vswap(v0, v1);
    if (nm_less(v2.f, v1.f)) {
        vswap(v1, v2);
        if (nm_less(v1.f, v0.f)) vswap(v0, v1);
    }
}

// scipy.optimize._optimize._minimize_neldermead (scipy 1.15.3) as fmin(score, x0, disp=False) calls it, for two
// parameters: xatol = fatol = 1e-4, maxiter = maxfun = 400, rho 1, chi 2, psi 0.5, sigma 0.5, not adaptive, no
// bounds.  Every thread runs the same scalar control flow; the scores come out of LDS identical in every thread.  A
// call past maxfun is refused as the wrapper refuses it (_MaxFuncCallError): the iteration is abandoned, the simplex
// sorted, the loop left.
template <int KIND>
__global__ __launch_bounds__(kPhaseMaxThreads) void phase_nm_kernel(const double *__restrict__ u, const double *__restrict__ v,
                                                                    const int64_t *__restrict__ off, const double *__restrict__ x0,
                                                                    double *__restrict__ x_out, double *__restrict__ f_out,
                                                                    int32_t *__restrict__ nfev_out, int32_t *__restrict__ nit_out,
                                                                    int32_t *__restrict__ status_out)
{
    __shared__ Lds lds;
    const int k = blockIdx.x;
    Spectrum sp;
    if (KIND == kScoreRosenbrock) {
        sp.u = sp.v = nullptr;
        sp.N = 0;
    } else {
        sp = spectrum_of(u, v, off, k);
    }
    const int nt = phase_threads(sp.N);
    int nfev = 0;
    bool empty = false;
    // the function wrapper: false when the call is refused (nfev already at maxfun) or the score raised (empty window)
    auto call = [&](double a, double b, double *f) -> bool {
        if (nfev >= kMaxFun || empty) return false;
        ++nfev;
        *f = evaluate<KIND>(sp, a, b, lds, nt, &empty);
        return !empty;
    };
    const double nonzdelt = 0.05, zdelt = 0.00025, xatol = 1e-4, fatol = 1e-4;
    const double ax = x0[2 * k], ay = x0[2 * k + 1];
    Vertex v0{ax, ay, INFINITY}, v1{ax, ay, INFINITY}, v2{ax, ay, INFINITY};
    v1.x = (ax != 0.0) ? (1.0 + nonzdelt) * ax : zdelt;
    v2.y = (ay != 0.0) ? (1.0 + nonzdelt) * ay : zdelt;
    int iterations = 1;
    call(v0.x, v0.y, &v0.f);   // (refused after an empty peak-minima window: the reference raises there)
    call(v1.x, v1.y, &v1.f);
    call(v2.x, v2.y, &v2.f);
    nm_sort(v0, v1, v2);
    while (!empty && nfev < kMaxFun && iterations < kMaxFun) {
        if (fabs(v1.x - v0.x) <= xatol && fabs(v1.y - v0.y) <= xatol && fabs(v2.x - v0.x) <= xatol &&
            fabs(v2.y - v0.y) <= xatol && fabs(v0.f - v1.f) <= fatol && fabs(v0.f - v2.f) <= fatol)
            break;   // (np.max(...) <= tol: false as soon as one term is NaN, as here)
        bool done = false;
        const double xbx = (v0.x + v1.x) / 2.0, xby = (v0.y + v1.y) / 2.0;
        const double xrx = 2.0 * xbx - v2.x, xry = 2.0 * xby - v2.y;
        double fxr;
        if (!call(xrx, xry, &fxr)) {
            done = true;
        } else if (fxr < v0.f) {
            const double xex = 3.0 * xbx - 2.0 * v2.x, xey = 3.0 * xby - 2.0 * v2.y;
            double fxe;
            if (!call(xex, xey, &fxe)) done = true;
            else if (fxe < fxr) v2 = Vertex{xex, xey, fxe};
            else v2 = Vertex{xrx, xry, fxr};
        } else if (fxr < v1.f) {
            v2 = Vertex{xrx, xry, fxr};
        } else {
            bool doshrink = false;
            if (fxr < v2.f) {
                const double xcx = 1.5 * xbx - 0.5 * v2.x, xcy = 1.5 * xby - 0.5 * v2.y;
                double fxc;
                if (!call(xcx, xcy, &fxc)) done = true;
                else if (fxc <= fxr) v2 = Vertex{xcx, xcy, fxc};
                else doshrink = true;
            } else {
                const double xcx = 0.5 * xbx + 0.5 * v2.x, xcy = 0.5 * xby + 0.5 * v2.y;
                double fxcc;
                if (!call(xcx, xcy, &fxcc)) done = true;
                else if (fxcc < v2.f) v2 = Vertex{xcx, xcy, fxcc};
                else doshrink = true;
            }
            if (doshrink) {
                v1.x = v0.x + 0.5 * (v1.x - v0.x);
                v1.y = v0.y + 0.5 * (v1.y - v0.y);
                if (!call(v1.x, v1.y, &v1.f)) {
                    done = true;
                } else {
                    v2.x = v0.x + 0.5 * (v2.x - v0.x);
                    v2.y = v0.y + 0.5 * (v2.y - v0.y);
                    if (!call(v2.x, v2.y, &v2.f)) done = true;
                }
            }
        }
        if (!done) ++iterations;
        nm_sort(v0, v1, v2);
        if (done) break;
    }
    if (threadIdx.x == 0) {
        const bool any_nan = __builtin_isnan(v0.f) || __builtin_isnan(v1.f) || __builtin_isnan(v2.f);
        x_out[2 * k] = v0.x;
        x_out[2 * k + 1] = v0.y;
        f_out[k] = any_nan ? NAN : v0.f;   // np.min(fsim)
        nfev_out[k] = nfev;
        nit_out[k] = iterations;
        status_out[k] = empty ? kStatusEmptyWindow : kStatusOk;
    }
}

// ---- host side -------------------------------------------------------------------------------------------------------

int check_spectra(const char *who, int32_t S, const int64_t *N, const double *u, const double *v, std::vector<int64_t> *off)
{
    int rc = check_spectra_count(who, S);
    if (rc != NMRFIT_OK) return rc;
    if (!N || !u || !v) {
        set_error(std::string(who) + ": null pointer");
        return NMRFIT_E_INVALID;
    }
    off->assign((size_t)S + 1, 0);
    for (int32_t k = 0; k < S; ++k) {
        if (N[k] < 2 || N[k] > ((int64_t)1 << 40)) {
            set_error(std::string(who) + ": every spectrum needs N >= 2 points (spectrum " + std::to_string(k) + ")");
            return NMRFIT_E_INVALID;
        }
        (*off)[(size_t)k + 1] = (*off)[(size_t)k] + N[k];
    }
    return NMRFIT_OK;
}

int upload_spectra(hipStream_t st, Scratch &mem, const std::vector<int64_t> &off, const double *u, const double *v,
                   double **d_u, double **d_v, int64_t **d_off)
{
    const size_t total = (size_t)off.back();
    NMRFIT_HIP(mem.alloc(d_u, total));
    NMRFIT_HIP(mem.alloc(d_v, total));
    NMRFIT_HIP(mem.alloc(d_off, off.size()));
    NMRFIT_HIP(hipMemcpyAsync(*d_u, u, total * sizeof(double), hipMemcpyHostToDevice, st));
    NMRFIT_HIP(hipMemcpyAsync(*d_v, v, total * sizeof(double), hipMemcpyHostToDevice, st));
    NMRFIT_HIP(hipMemcpyAsync(*d_off, off.data(), off.size() * sizeof(int64_t), hipMemcpyHostToDevice, st));
    return NMRFIT_OK;
}

int max_threads(const std::vector<int64_t> &off)
{
    int nt = 0;
    for (size_t k = 0; k + 1 < off.size(); ++k) nt = std::max(nt, phase_threads(off[k + 1] - off[k]));
    return std::max(nt, phase_threads(0));
}

int run_nm(int device, int kind, int32_t S, const std::vector<int64_t> &off, const double *u, const double *v,
           const double *x0, double *x, double *f, int32_t *nfev, int32_t *nit, int32_t *status)
{
    int rc = use_device(device);
    if (rc != NMRFIT_OK) return rc;
    StreamLease lease(device);
    NMRFIT_HIP(lease.take());
    hipStream_t st = lease.s;
    Scratch mem;
    double *d_u = nullptr, *d_v = nullptr, *d_x0 = nullptr, *d_x = nullptr, *d_f = nullptr;
    int64_t *d_off = nullptr;
    int32_t *d_i = nullptr;
    if (kind != kScoreRosenbrock && (rc = upload_spectra(st, mem, off, u, v, &d_u, &d_v, &d_off)) != NMRFIT_OK) return rc;
    NMRFIT_HIP(mem.alloc(&d_x0, 2 * (size_t)S));
    NMRFIT_HIP(mem.alloc(&d_x, 2 * (size_t)S));
    NMRFIT_HIP(mem.alloc(&d_f, (size_t)S));
    NMRFIT_HIP(mem.alloc(&d_i, 3 * (size_t)S));
    NMRFIT_HIP(hipMemcpyAsync(d_x0, x0, 2 * (size_t)S * sizeof(double), hipMemcpyHostToDevice, st));
    const int nt = kind == kScoreRosenbrock ? kWave : max_threads(off);
    if (kind == kScoreAcme)
        hipLaunchKernelGGL(phase_nm_kernel<kScoreAcme>, dim3(S), dim3(nt), 0, st, d_u, d_v, d_off, d_x0, d_x, d_f, d_i, d_i + S, d_i + 2 * S);
    else if (kind == kScorePeakMinima)
        hipLaunchKernelGGL(phase_nm_kernel<kScorePeakMinima>, dim3(S), dim3(nt), 0, st, d_u, d_v, d_off, d_x0, d_x, d_f, d_i, d_i + S, d_i + 2 * S);
    else
        hipLaunchKernelGGL(phase_nm_kernel<kScoreRosenbrock>, dim3(S), dim3(nt), 0, st, d_u, d_v, d_off, d_x0, d_x, d_f, d_i, d_i + S, d_i + 2 * S);
    NMRFIT_HIP(hipGetLastError());
    std::vector<int32_t> ints(3 * (size_t)S);
    NMRFIT_HIP(hipMemcpyAsync(x, d_x, 2 * (size_t)S * sizeof(double), hipMemcpyDeviceToHost, st));
    NMRFIT_HIP(hipMemcpyAsync(f, d_f, (size_t)S * sizeof(double), hipMemcpyDeviceToHost, st));
    NMRFIT_HIP(hipMemcpyAsync(ints.data(), d_i, ints.size() * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    NMRFIT_HIP(hipStreamSynchronize(st));
    std::memcpy(nfev, ints.data(), (size_t)S * sizeof(int32_t));
    std::memcpy(nit, ints.data() + S, (size_t)S * sizeof(int32_t));
    if (status) std::memcpy(status, ints.data() + 2 * S, (size_t)S * sizeof(int32_t));
    return NMRFIT_OK;
}

// one phase_scores_kernel launch over (M candidates) x (S spectra); empty: S x M flags (peak minima's empty window)
int run_scores(int device, int kind, int32_t S, const std::vector<int64_t> &off, const double *u, const double *v,
               int32_t M, const double *cand, const int64_t *n_mean, double *score, int32_t *empty)
{
    int rc = use_device(device);
    if (rc != NMRFIT_OK) return rc;
    StreamLease lease(device);
    NMRFIT_HIP(lease.take());
    hipStream_t st = lease.s;
    Scratch mem;
    double *d_u = nullptr, *d_v = nullptr, *d_c = nullptr, *d_s = nullptr;
    int64_t *d_off = nullptr, *d_n = nullptr;
    int32_t *d_e = nullptr;
    const size_t SM = (size_t)S * (size_t)M;
    if ((rc = upload_spectra(st, mem, off, u, v, &d_u, &d_v, &d_off)) != NMRFIT_OK) return rc;
    NMRFIT_HIP(mem.alloc(&d_c, 2 * SM));
    NMRFIT_HIP(mem.alloc(&d_s, SM));
    NMRFIT_HIP(mem.alloc(&d_e, SM));
    NMRFIT_HIP(hipMemcpyAsync(d_c, cand, 2 * SM * sizeof(double), hipMemcpyHostToDevice, st));
    if (n_mean) {
        NMRFIT_HIP(mem.alloc(&d_n, (size_t)S));
        NMRFIT_HIP(hipMemcpyAsync(d_n, n_mean, (size_t)S * sizeof(int64_t), hipMemcpyHostToDevice, st));
    }
    const dim3 grid((unsigned)M, (unsigned)S), block((unsigned)max_threads(off));
    if (kind == NMRFIT_PHASE_ACME)
        hipLaunchKernelGGL(phase_scores_kernel<kScoreAcme>, grid, block, 0, st, d_u, d_v, d_off, M, d_c, d_s, d_e, d_n);
    else if (kind == NMRFIT_PHASE_PEAK_MINIMA)
        hipLaunchKernelGGL(phase_scores_kernel<kScorePeakMinima>, grid, block, 0, st, d_u, d_v, d_off, M, d_c, d_s, d_e, d_n);
    else
        hipLaunchKernelGGL(phase_scores_kernel<kScoreBrute>, grid, block, 0, st, d_u, d_v, d_off, M, d_c, d_s, d_e, d_n);
    NMRFIT_HIP(hipGetLastError());
    NMRFIT_HIP(hipMemcpyAsync(score, d_s, SM * sizeof(double), hipMemcpyDeviceToHost, st));
    NMRFIT_HIP(hipMemcpyAsync(empty, d_e, SM * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    NMRFIT_HIP(hipStreamSynchronize(st));
    return NMRFIT_OK;
}

}  // namespace
}  // namespace nmrfit

using namespace nmrfit;

#pragma GCC visibility push(default)   // the C-ABI: the only symbols the library exports (build.sh: -fvisibility=hidden)

int nmrfit_phase_scores(int device, int kind, int32_t S, const int64_t *N, const double *u, const double *v, int32_t M,
                        const double *cand, double *score, int32_t *status)
{
    const char *who = "nmrfit_phase_scores";
    if (kind != NMRFIT_PHASE_ACME && kind != NMRFIT_PHASE_PEAK_MINIMA && kind != NMRFIT_PHASE_BRUTE_LEVEL) {
        set_error(std::string(who) + ": unknown score kind " + std::to_string(kind));
        return NMRFIT_E_INVALID;
    }
    if (M < 1) {
        set_error(std::string(who) + ": M must be >= 1");
        return NMRFIT_E_INVALID;
    }
    if (!cand || !score || !status) {
        set_error(std::string(who) + ": null pointer");
        return NMRFIT_E_INVALID;
    }
    std::vector<int64_t> off;
    int rc = check_spectra(who, S, N, u, v, &off);
    if (rc != NMRFIT_OK) return rc;
    if (kind == NMRFIT_PHASE_BRUTE_LEVEL)
        for (int32_t k = 0; k < S; ++k)
            if (brute_default_mean(N[k]) > kBruteMaxMeanTerms) {
                set_error(std::string(who) + ": the brute level test takes means of at most 128 points (N < 645000)");
                return NMRFIT_E_UNSUPPORTED;
            }
    std::vector<int32_t> empty((size_t)S * (size_t)M);
    if ((rc = run_scores(device, kind, S, off, u, v, M, cand, nullptr, score, empty.data())) != NMRFIT_OK) return rc;
    for (int32_t k = 0; k < S; ++k) {
        status[k] = kStatusOk;
        for (int32_t m = 0; m < M; ++m)
            if (empty[(size_t)k * M + m]) status[k] = kStatusEmptyWindow;
    }
    return NMRFIT_OK;
}

int nmrfit_phase_brute_levels(int device, int32_t S, const int64_t *N, const int64_t *n_mean, const double *u,
                              const double *v, int32_t M, const double *cand, double *score)
{
    const char *who = "nmrfit_phase_brute_levels";
    if (M < 1) {
        set_error(std::string(who) + ": M must be >= 1");
        return NMRFIT_E_INVALID;
    }
    if (!n_mean || !cand || !score) {
        set_error(std::string(who) + ": null pointer");
        return NMRFIT_E_INVALID;
    }
    std::vector<int64_t> off;
    int rc = check_spectra(who, S, N, u, v, &off);
    if (rc != NMRFIT_OK) return rc;
    for (int32_t k = 0; k < S; ++k) {
        if (n_mean[k] < 1) {
            set_error(std::string(who) + ": the mean length must be >= 1 (spectrum " + std::to_string(k) + ")");
            return NMRFIT_E_INVALID;
        }
        if (n_mean[k] > kBruteMaxMeanTerms) {
            set_error(std::string(who) + ": the brute level test takes means of at most 128 points, spectrum " +
                      std::to_string(k) + " asks for a mean length of " + std::to_string(n_mean[k]));
            return NMRFIT_E_UNSUPPORTED;
        }
    }
    std::vector<int32_t> empty((size_t)S * (size_t)M);
    return run_scores(device, NMRFIT_PHASE_BRUTE_LEVEL, S, off, u, v, M, cand, n_mean, score, empty.data());
}

int nmrfit_phase_estimate(int device, int kind, int32_t S, const int64_t *N, const double *u, const double *v,
                          const double *x0, double *x, double *f, int32_t *nfev, int32_t *nit, int32_t *status)
{
    const char *who = "nmrfit_phase_estimate";
    if (kind != NMRFIT_PHASE_ACME && kind != NMRFIT_PHASE_PEAK_MINIMA) {
        set_error(std::string(who) + ": kind must be NMRFIT_PHASE_ACME or NMRFIT_PHASE_PEAK_MINIMA (the brute level test "
                  "is a scan, not a score to minimise), got " + std::to_string(kind));
        return NMRFIT_E_INVALID;
    }
    if (!x0 || !x || !f || !nfev || !nit || !status) {
        set_error(std::string(who) + ": null pointer");
        return NMRFIT_E_INVALID;
    }
    std::vector<int64_t> off;
    int rc = check_spectra(who, S, N, u, v, &off);
    if (rc != NMRFIT_OK) return rc;
    return run_nm(device, kind, S, off, u, v, x0, x, f, nfev, nit, status);
}

int nmrfit_diag_phase_nm_rosenbrock(int device, int32_t S, const double *x0, double *x, double *f, int32_t *nfev, int32_t *nit)
{
    if (S < 1 || S > 65535 || !x0 || !x || !f || !nfev || !nit) {
        set_error("nmrfit_diag_phase_nm_rosenbrock: bad arguments");
        return NMRFIT_E_INVALID;
    }
    std::vector<int64_t> off((size_t)S + 1, 0);
    return run_nm(device, kScoreRosenbrock, S, off, nullptr, nullptr, x0, x, f, nfev, nit, nullptr);
}

#pragma GCC visibility pop

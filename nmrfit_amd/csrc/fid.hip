// fid.hip -- raw FIDs to spectra on the GPU (opt-in; include/nmrfit_amd_fid.h holds the definition): a batched fp64
// complex Fourier transform with zero filling, the centring and reversal of the reference's loader in the last pass's
// store, then the normaliser (a lexicographic maximum), the quotient by Smith's rule and the sum over traces.
//   fid_short_kernel      a workgroup of 256 threads per trace of n <= 4096 points: load with zero fill, every stage in
//                         LDS, the centred and reversed store
//   fid_pass1_kernel      n = n1 n2 > 4096: a workgroup takes 4096 / n1 adjacent columns (stride n2) of one trace,
//                         transforms them in LDS and stores them times the twiddle omega_n^(j2 q1)
//   fid_pass2_kernel      ... and 4096 / n2 adjacent rows (n2 contiguous points each), whose store centres and reverses
//   fid_max_part_kernel   the lexicographic maximum and a not-finite flag of 8192 values of a spectrum, of any length
//   fid_max_kernel        ... of the partial maxima of a spectrum: the row
//   fid_finish_kernel     1024 output points of a spectrum: the quotient of every trace's value, summed over the traces
// Every launch is a flat list of work items over all spectra of the call; a workgroup finds its spectrum by a binary
// search in the launch's prefix table (K + 1 numbers): at most six launches whatever K and T.  No atomics, no scratch
// memory; every value is a pure function of the spectrum's own input (the definition's PURITY).  The entry points and
// the body of a call are fid_call.hip's; this file exports nothing.
//
// THE LDS BLOCK.  Up to 4096 complex points as two planes of doubles (re, im).  C = 2^lgC transforms of length L are
// interleaved, point p of transform c at index p C + c, so a stage of C > 1 transforms is a stage of one transform of
// C L points that stops early.  A stage of radix R reads its R inputs at b + r M / R (b: the butterfly, M = C L):
// consecutive lanes read consecutive doubles.  It writes runs of Ns C consecutive doubles R Ns C apart (Ns: the length
// already transformed), and the row loads of pass 2 write R doubles apart: power-of-two strides, which unswizzled land
// 2 to 16 lanes of a 16-lane store group (16 eight-byte slots of the 32 banks a ds_write sees) on one slot.  swz()
// XORs the low four bits of an index with a GF(2)-linear function of bits 4 .. 8 that makes every one of these
// patterns -- runs of 1, 2, 4, 8 at radix 2 or 4, strides 2 .. 32, and unit stride -- a bijection of the 16 lanes onto
// the 16 slots, and leaves 32 consecutive aligned doubles on 32 distinct slots of the 64 banks a ds_read_b64 sees
// (tests/test_fid_cpu.py enumerates the patterns).  The XOR stays inside an aligned block of 16: no padding, 64 KiB for
// 4096 points, two workgroups per CU.
//
// A stage is in place: every thread reads the inputs of its butterflies into registers, the workgroup meets, every
// thread writes.  Radix 4 keeps 4 butterflies x 4 points (64 VGPRs of data) per thread at 4096 points and halves the
// stages, and with them the barriers and the LDS traffic, against radix 2; an odd log2 L takes ONE radix-2 stage first
// (its twiddles are all 1).
#include "fid_device.h"
#include "fid_internal.h"
#include "nmrfit_amd_fid.h"

#include <climits>
#include <cmath>
#include <vector>

namespace nmrfit {
namespace {

#pragma clang fp contract(off)   // (every product and sum of the definition is rounded once)

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / kWave;
constexpr int kRow = NMRFIT_FID_ROW;
constexpr int kLgLds = NMRFIT_FID_LDS_LOG2, kLdsPoints = 1 << kLgLds;
constexpr int kLgMax = NMRFIT_FID_MAX_LOG2;
constexpr int kMaxChunk = 8192;      // values per partial maximum
constexpr int kFinishChunk = 1024;   // output points per finishing workgroup
constexpr unsigned kGridX = 32768;   // work items per grid row (an item is blockIdx.y * gridDim.x + blockIdx.x)
static_assert(kLgLds == kFidLgStage && kLgMax == kFidLgMax, "the twiddle tables are sized for these lengths");
static_assert(kLgMax <= 2 * (kLgLds - 1), "both factors of a long transform leave at least two transforms per block");

// where index a of the block lies in a plane (the header comment: THE LDS BLOCK)
__device__ __forceinline__ int swz(int a)
{
    const int h = a >> 4;
    return a ^ ((-(h & 1) & 15) ^ (-((h >> 1) & 1) & 10) ^ ((h >> 2) & 7));
}

// One in-place stage of radix R on M = C L points: Ns = 2^lgNs points of every transform are transformed already.
template <int R>
__device__ __forceinline__ void lds_stage(double *__restrict__ re, double *__restrict__ im, int M, int lgC, int lgNs,
                                          const FidTw *__restrict__ tw)
{
    constexpr int kPer = kLdsPoints / R / kThreads;   // butterflies per thread at a full block
    constexpr int lgR = R == 4 ? 2 : 1;
    const int nb = M >> lgR;
    Cx x[kPer][R];
#pragma unroll
    for (int i = 0; i < kPer; ++i) {
        const int b = (int)threadIdx.x + i * kThreads;
        if (b < nb) {
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const int at = swz(b + r * nb);
                x[i][r] = Cx{re[at], im[at]};
            }
        }
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < kPer; ++i) {
        const int b = (int)threadIdx.x + i * kThreads;
        if (b < nb) {
            const int j = b >> lgC, c = b & ((1 << lgC) - 1);
            const int k = j & ((1 << lgNs) - 1);
            const int out = ((((j - k) << lgR) + k) << lgC) + c, step = 1 << (lgNs + lgC);
            Cx y[R];
            if constexpr (R == 2) {   // (the first stage of an odd log2 L: Ns = 1, every twiddle is 1)
                y[0] = cadd(x[i][0], x[i][1]);
                y[1] = csub(x[i][0], x[i][1]);
            } else {
                const int ts = kFidLgStage - 2 - lgNs;   // omega_{4 Ns}^(k r) = omega_4096^(k r 4096 / (4 Ns))
                const FidTw w1 = tw[k << ts], w2 = tw[(2 * k) << ts], w3 = tw[(3 * k) << ts];
                const Cx z1 = cmul(x[i][1], Cx{w1.re, w1.im}), z2 = cmul(x[i][2], Cx{w2.re, w2.im});
                const Cx z3 = cmul(x[i][3], Cx{w3.re, w3.im});
                const Cx s02 = cadd(x[i][0], z2), d02 = csub(x[i][0], z2), s13 = cadd(z1, z3), d13 = csub(z1, z3);
                const Cx mi = Cx{d13.im, -d13.re};   // -i d13
                y[0] = cadd(s02, s13);
                y[1] = cadd(d02, mi);
                y[2] = csub(s02, s13);
                y[3] = csub(d02, mi);
            }
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const int at = swz(out + r * step);
                re[at] = y[r].re;
                im[at] = y[r].im;
            }
        }
    }
    __syncthreads();
}

// C = 2^lgC interleaved transforms of length 2^lgL in the block, M = C L points.  The caller's loads are followed by a
// barrier; the last stage ends with one.  Every thread of the workgroup makes the same number of stages.
__device__ __forceinline__ void lds_fft(double *__restrict__ re, double *__restrict__ im, int M, int lgC, int lgL,
                                        const FidTw *__restrict__ tw)
{
    int lgNs = 0;
    if (lgL & 1) {
        lds_stage<2>(re, im, M, lgC, 0, tw);
        lgNs = 1;
    }
    for (; lgNs < lgL; lgNs += 2) lds_stage<4>(re, im, M, lgC, lgNs, tw);
}

__global__ __launch_bounds__(kThreads) void fid_short_kernel(const FidJob *__restrict__ jobs, const long long *__restrict__ pref,
                                                             int K, int plane, const FidTw *__restrict__ tw)
{
    extern __shared__ __align__(16) double lds[];
    double *re = lds, *im = lds + plane;
    ItemAt at;
    if (!item_at(pref, K, &at)) return;
    const FidJob &q = jobs[at.k];
    const long long t = at.local();
    const int n = q.n, n_in = q.n_in;
    const double2 *__restrict__ x = q.x + t * n_in;
    for (int e = threadIdx.x; e < n; e += kThreads) {
        const double2 val = e < n_in ? x[e] : make_double2(0.0, 0.0);
        const int at = swz(e);
        re[at] = val.x;
        im[at] = val.y;
    }
    __syncthreads();
    lds_fft(re, im, n, 0, q.lg, tw);
    double2 *__restrict__ z = q.z + t * n;
    for (int j = threadIdx.x; j < n; j += kThreads) {
        const int at = swz((n - 1 - j) ^ (n >> 1));   // Z[j] = Y[n - 1 - j] = X[(n - 1 - j + n / 2) mod n]
        z[j] = make_double2(re[at], im[at]);
    }
}

__global__ __launch_bounds__(kThreads) void fid_pass1_kernel(const FidJob *__restrict__ jobs, const long long *__restrict__ pref,
                                                             int K, const FidTw *__restrict__ tw, const FidTwDD *__restrict__ hi,
                                                             const FidTwDD *__restrict__ lo)
{
    extern __shared__ __align__(16) double lds[];
    double *re = lds, *im = lds + kLdsPoints;
    ItemAt at;
    if (!item_at(pref, K, &at)) return;
    const FidJob &q = jobs[at.k];
    const long long local = at.local();
    const int lg1 = q.lg1, lg2 = q.lg2, lgC = kLgLds - lg1, n2 = 1 << lg2, n_in = q.n_in;
    const long long t = local >> (lg2 - lgC);                        // n2 / C groups of columns per trace
    const int col0 = (int)(local & ((1 << (lg2 - lgC)) - 1)) << lgC;   // the group's first column
    const double2 *__restrict__ x = q.x + t * n_in;
    for (int e = threadIdx.x; e < kLdsPoints; e += kThreads) {
        const int c = e & ((1 << lgC) - 1), j1 = e >> lgC;
        const int s = (j1 << lg2) + col0 + c;
        const double2 val = s < n_in ? x[s] : make_double2(0.0, 0.0);
        const int at = swz(e);
        re[at] = val.x;
        im[at] = val.y;
    }
    __syncthreads();
    lds_fft(re, im, kLdsPoints, lgC, lg1, tw);
    double2 *__restrict__ work = q.work + t * q.n;
    const int up = kLgMax - q.lg;   // omega_n^(j2 q1) = omega_{2^22}^(j2 q1 2^22 / n)
    for (int e = threadIdx.x; e < kLdsPoints; e += kThreads) {
        const int c = e & ((1 << lgC) - 1), q1 = e >> lgC, j2 = col0 + c;
        const FidTw w = fid_split_twiddle(hi, lo, (j2 * q1) << up);
        const int at = swz(e);
        const Cx val = cmul(Cx{re[at], im[at]}, Cx{w.re, w.im});
        work[(q1 << lg2) + j2] = make_double2(val.re, val.im);
    }
}

__global__ __launch_bounds__(kThreads) void fid_pass2_kernel(const FidJob *__restrict__ jobs, const long long *__restrict__ pref,
                                                             int K, const FidTw *__restrict__ tw)
{
    extern __shared__ __align__(16) double lds[];
    double *re = lds, *im = lds + kLdsPoints;
    ItemAt at;
    if (!item_at(pref, K, &at)) return;
    const FidJob &q = jobs[at.k];
    const long long local = at.local();
    const int lg1 = q.lg1, lg2 = q.lg2, lgR = kLgLds - lg2, n = q.n;
    const long long t = local >> (lg1 - lgR);                        // n1 / R groups of rows per trace
    const int row0 = (int)(local & ((1 << (lg1 - lgR)) - 1)) << lgR;   // the group's first row
    const double2 *__restrict__ work = q.work + t * n + ((long long)row0 << lg2);   // R rows: 4096 contiguous points
    for (int e = threadIdx.x; e < kLdsPoints; e += kThreads) {
        const int r = e >> lg2, j2 = e & ((1 << lg2) - 1);
        const double2 val = work[e];
        const int at = swz((j2 << lgR) + r);
        re[at] = val.x;
        im[at] = val.y;
    }
    __syncthreads();
    lds_fft(re, im, kLdsPoints, lgR, lg2, tw);
    double2 *__restrict__ z = q.z + t * n;
    for (int e = threadIdx.x; e < kLdsPoints; e += kThreads) {
        const int r = e & ((1 << lgR) - 1), q2 = e >> lgR;
        const int xq = row0 + r + (q2 << lg1);   // X's index q = q1 + n1 q2
        const int at = swz(e);
        z[n - 1 - (xq ^ (n >> 1))] = make_double2(re[at], im[at]);
    }
}

// the running lexicographic maximum: (re, im, the flat index in Y's order); `bad`: a value that is not finite was seen
struct Best {
    double re, im;
    long long idx;
    int bad;
};
__device__ __forceinline__ Best best_init() { return Best{-INFINITY, -INFINITY, LLONG_MAX, 0}; }
__device__ __forceinline__ void best_take(Best &a, double re, double im, long long idx, int bad)
{
    const bool better = re > a.re || (re == a.re && (im > a.im || (im == a.im && idx < a.idx)));
    if (better) {
        a.re = re;
        a.im = im;
        a.idx = idx;
    }
    a.bad |= bad;
}

// the workgroup's maximum in thread 0 (maxima are exact: the order of the reduction is free)
__device__ __forceinline__ Best best_of_workgroup(Best mine, Best *s_best)
{
    for (int o = kWave / 2; o > 0; o >>= 1)
        best_take(mine, __shfl_xor(mine.re, o), __shfl_xor(mine.im, o), __shfl_xor(mine.idx, o), __shfl_xor(mine.bad, o));
    if (threadIdx.x % kWave == 0) s_best[threadIdx.x / kWave] = mine;
    __syncthreads();
    Best all = s_best[0];
    for (int wv = 1; wv < kWaves; ++wv) best_take(all, s_best[wv].re, s_best[wv].im, s_best[wv].idx, s_best[wv].bad);
    return all;
}

__global__ __launch_bounds__(kThreads) void fid_max_part_kernel(const FidJob *__restrict__ jobs, const long long *__restrict__ pref,
                                                                int K)
{
    __shared__ Best s_best[kWaves];
    ItemAt at;
    if (!item_at(pref, K, &at)) return;
    const FidJob &q = jobs[at.k];
    const int chunk = (int)at.local(), n = q.n;
    const long long total = (long long)q.T * n, from = (long long)chunk * kMaxChunk;
    const long long to = from + kMaxChunk < total ? from + kMaxChunk : total;
    const double2 *__restrict__ z = q.z;
    Best mine = best_init();
    // (Z[t n + j] is Y[t n + n - 1 - j]; the branch is the workgroup's: one job)
    if (q.lg >= 0) {   // n is a power of two: the point within the trace by a mask
        for (long long p = from + threadIdx.x; p < to; p += kThreads) {
            const double2 val = z[p];
            const long long j = p & (n - 1);
            best_take(mine, val.x, val.y, p + (n - 1) - 2 * j, !(isfinite(val.x) && isfinite(val.y)));
        }
    } else {   // a finish-only job, n any length: by a remainder (one 64-bit division per item, a 32-bit one per value)
        const unsigned un = (unsigned)n;
        const long long t0 = from / un;
        const unsigned j0 = (unsigned)(from - t0 * un);
        for (long long p = from + threadIdx.x; p < to; p += kThreads) {
            const double2 val = z[p];
            const unsigned at = j0 + (unsigned)(p - from), dt = at / un, j = at - dt * un;   // (at < n + 8192 < 2^32)
            best_take(mine, val.x, val.y, (t0 + dt) * (long long)un + (un - 1 - j), !(isfinite(val.x) && isfinite(val.y)));
        }
    }
    const Best all = best_of_workgroup(mine, s_best);
    if (threadIdx.x == 0) q.part[chunk] = make_double4(all.re, all.im, all.bad ? 0.0 : (double)all.idx, all.bad ? 1.0 : 0.0);
}

__global__ __launch_bounds__(kThreads) void fid_max_kernel(const FidJob *__restrict__ jobs)
{
    __shared__ Best s_best[kWaves];
    const FidJob &q = jobs[blockIdx.x];
    Best mine = best_init();
    for (int p = threadIdx.x; p < q.parts; p += kThreads) {
        const double4 part = q.part[p];
        best_take(mine, part.x, part.y, (long long)part.z, part.w != 0.0);
    }
    const Best all = best_of_workgroup(mine, s_best);
    if (threadIdx.x == 0) {
        const double nan = __builtin_nan("");
        double *row = q.row;
        row[0] = all.bad ? 2.0 : (all.re == 0.0 && all.im == 0.0 ? 1.0 : 0.0);
        row[1] = all.bad ? nan : all.re;
        row[2] = all.bad ? nan : all.im;
        row[3] = all.bad ? nan : (double)all.idx;
        row[4] = (double)q.n;
        row[5] = (double)q.T;
    }
}

__global__ __launch_bounds__(kThreads) void fid_finish_kernel(const FidJob *__restrict__ jobs, const long long *__restrict__ pref,
                                                              int K)
{
    ItemAt at;
    if (!item_at(pref, K, &at)) return;
    const FidJob &q = jobs[at.k];
    const int n = q.n, T = q.T, from = (int)at.local() * kFinishChunk;
    const double status = q.row[0], mr = q.row[1], mi = q.row[2];
    const bool first = fabs(mr) >= fabs(mi);
    const double rat = first ? mi / mr : mr / mi;
    const double scl = first ? 1.0 / (mr + mi * rat) : 1.0 / (mi + mr * rat);
    const double2 *__restrict__ z = q.z;
    for (int j = from + (int)threadIdx.x; j < n && j < from + kFinishChunk; j += kThreads) {
        double u = 0.0, v = 0.0;   // (np.sum's start: a sum of -0.0 alone comes out as +0.0)
        for (int t = 0; t < T; ++t) {
            const double2 val = z[(long long)t * n + j];
            const double a = val.x, b = val.y;
            const double qr = first ? (a + b * rat) * scl : (a * rat + b) * scl;
            const double qi = first ? (b - a * rat) * scl : (b * rat - a) * scl;
            u = u + qr;
            v = v + qi;
        }
        if (status != 0.0) u = v = __builtin_nan("");
        q.u[j] = u;
        q.v[j] = v;
    }
}

// the twiddle tables, made once per process on the host (fid_twiddle.h)
struct FidTables {
    std::vector<FidTw> stage;
    std::vector<FidTwDD> hi, lo;
    FidTables() : stage(kFidStage), hi(kFidSplit), lo(kFidSplit)
    {
        fid_fill_stage_table(stage.data());
        fid_fill_split_tables(hi.data(), lo.data());
    }
};
const FidTables &fid_tables()
{
    static const FidTables t;
    return t;
}

}  // namespace

// ---- the pieces of a call (fid_internal.h) --------------------------------------------------------------------------

dim3 fid_item_grid(long long items)
{
    const unsigned gx = (unsigned)std::min<long long>(items, kGridX);
    return dim3(gx, (unsigned)((items + gx - 1) / gx));
}

int fid_log2_exact(int64_t n)
{
    if (n <= 0 || (n & (n - 1))) return -1;
    int lg = 0;
    while (((int64_t)1 << lg) < n) ++lg;
    return lg;
}

FidPlan fid_plan(const FidShape *shapes, size_t nk)
{
    FidPlan plan;
    plan.tab = ItemTables(kFidLaunchTables, nk);
    for (size_t k = 0; k < nk; ++k) {
        const int64_t n = shapes[k].n;
        const int lg = fid_log2_exact(n);   // (-1: a finish-only job)
        const bool is_short = lg >= 0 && lg <= kLgLds, is_long = lg > kLgLds;
        const int lg1 = lg / 2, lg2 = lg - lg1;
        const long long Tk = shapes[k].T, total = Tk * n;
        plan.tab.add(kFidShort, k, is_short ? Tk : 0);
        plan.tab.add(kFidPass1, k, is_long ? Tk << (lg2 - (kLgLds - lg1)) : 0);
        plan.tab.add(kFidPass2, k, is_long ? Tk << (lg1 - (kLgLds - lg2)) : 0);
        plan.tab.add(kFidMaxPart, k, (total + kMaxChunk - 1) / kMaxChunk);
        plan.tab.add(kFidFinish, k, (n + kFinishChunk - 1) / kFinishChunk);
        if (is_short) plan.max_short = std::max(plan.max_short, (int)n);
        if (is_long) plan.work_values += total;
        plan.values += total;
        plan.in_values += Tk * shapes[k].n_in;
        plan.points += n;
    }
    return plan;
}

std::vector<FidJob> fid_job_table(const FidPlan &plan, const FidShape *shapes, const double2 *const *x_of, const FidBuffers &buf)
{
    const size_t nk = plan.tab.K;
    const long long *p_max = plan.tab.row(kFidMaxPart);
    std::vector<FidJob> jobs(nk);
    size_t at_work = 0, at_z = 0, at_u = 0;
    for (size_t k = 0; k < nk; ++k) {
        const int lg = fid_log2_exact(shapes[k].n);   // (-1: a finish-only job)
        const bool is_long = lg > kLgLds;
        const size_t total = (size_t)shapes[k].T * (size_t)shapes[k].n;
        jobs[k] = FidJob{x_of[k], is_long ? buf.work + at_work : nullptr, buf.z + at_z, buf.u ? buf.u + at_u : nullptr,
                         buf.v ? buf.v + at_u : nullptr, buf.rows ? buf.rows + k * kRow : nullptr, buf.part ? buf.part + p_max[k] : nullptr,
                         (int32_t)shapes[k].n_in, (int32_t)shapes[k].n, shapes[k].T, lg, lg < 0 ? 0 : lg / 2, lg < 0 ? 0 : lg - lg / 2,
                         (int32_t)(p_max[k + 1] - p_max[k])};
        if (is_long) at_work += total;
        at_z += total;
        at_u += (size_t)shapes[k].n;
    }
    return jobs;
}

hipError_t fid_upload_tables(const FidDeviceTables &dst, hipStream_t st)
{
    const FidTables &tables = fid_tables();
    hipError_t e = hipMemcpyAsync(dst.tw, tables.stage.data(), kFidStage * sizeof(FidTw), hipMemcpyHostToDevice, st);
    if (e != hipSuccess) return e;
    e = hipMemcpyAsync(dst.hi, tables.hi.data(), kFidSplit * sizeof(FidTwDD), hipMemcpyHostToDevice, st);
    if (e != hipSuccess) return e;
    return hipMemcpyAsync(dst.lo, tables.lo.data(), kFidSplit * sizeof(FidTwDD), hipMemcpyHostToDevice, st);
}

hipError_t fid_launch_transforms(const FidPlan &plan, const FidJob *d_jobs, const long long *d_pref, const FidDeviceTables &tables,
                                 hipStream_t st)
{
    const ItemTables &tab = plan.tab;
    const int K = (int)tab.K;
    const size_t block_lds = 2 * (size_t)kLdsPoints * sizeof(double);
    const int plane = std::max(plan.max_short, 16);   // (swz stays inside an aligned block of 16)
    hipError_t e = launch_items(fid_short_kernel, tab.items(kFidShort), kThreads, 2 * (size_t)plane * sizeof(double), st, d_jobs,
                                tab.device(d_pref, kFidShort), K, plane, tables.tw);
    if (e != hipSuccess) return e;
    e = launch_items(fid_pass1_kernel, tab.items(kFidPass1), kThreads, block_lds, st, d_jobs, tab.device(d_pref, kFidPass1), K,
                     tables.tw, tables.hi, tables.lo);
    if (e != hipSuccess) return e;
    return launch_items(fid_pass2_kernel, tab.items(kFidPass2), kThreads, block_lds, st, d_jobs, tab.device(d_pref, kFidPass2), K,
                        tables.tw);
}

hipError_t fid_launch_finish(const FidPlan &plan, const FidJob *d_jobs, const long long *d_pref, hipStream_t st)
{
    const ItemTables &tab = plan.tab;
    const int K = (int)tab.K;
    hipError_t e = launch_items(fid_max_part_kernel, tab.items(kFidMaxPart), kThreads, 0, st, d_jobs, tab.device(d_pref, kFidMaxPart), K);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(fid_max_kernel, dim3((unsigned)K), dim3(kThreads), 0, st, d_jobs);   // (a workgroup per spectrum)
    if ((e = hipGetLastError()) != hipSuccess) return e;
    return launch_items(fid_finish_kernel, tab.items(kFidFinish), kThreads, 0, st, d_jobs, tab.device(d_pref, kFidFinish), K);
}

}  // namespace nmrfit

// fid_any.hip -- raw FIDs of any length on the GPU (opt-in; include/nmrfit_amd_fid_any.h holds the definition): the
// chirp-z (Bluestein) transform of a trace whose transform length N is no power of two, as three transforms of length
// M = 2^m >= 2 N - 1 by fid.hip's kernels, launched through fid_internal.h on job tables made here, and four element-wise
// stages between them:
//   fida_load_kernel       (a) a[k] = x'[k] c[k] for k < n_in', 0 up to M: what the first transform loads
//   fida_filter_kernel     (b) b[k] = conj(c[k]), b[M - k] = conj(c[k]), 0 elsewhere: once per distinct N of the call
//   fida_product_kernel    (c) P[q] = A[q] B[q] in natural order; both operands are read through the permutation the
//                          transform kernels store with: entry M - 1 - (q ^ M/2) holds the value of index q
//   fida_store_kernel      (d) X[q] = fft(P)[(-q) mod M] / M * c[q] read through the same permutation, stored centred
//                          and reversed: Z[j] = Y[N - 1 - j], Y[i] = X[(i + N - floor(N/2)) mod N]
// Every launch is a flat list of work items (1024 points of a trace) found by the prefix-table search of fid.hip; a
// launch without items is not made.  The permuted reads flip the top bit of the index and reverse the order: 64
// consecutive lanes read 64 consecutive values on every side.  No LDS, no atomics, no scratch memory.  The chirp values
// are the host's table (fid_chirp.h), one per distinct N.  The spectra of the stage are FINISH-ONLY jobs of the call's
// main job table: fid.hip's finishing launches take their Z from (d).
// P overwrites a (dead once A is stored) and fft(P) overwrites A (dead once P is stored): two planes of T M values per
// spectrum.  The filter's transform B is a job (T = 1) of the same launches as the A transforms.
#include "fid_chirp.h"
#include "fid_device.h"
#include "fid_internal.h"
#include "nmrfit_amd_fid_any.h"

#include <map>
#include <vector>

namespace nmrfit {
namespace {

#pragma clang fp contract(off)   // (every product and sum of the definition is rounded once)

constexpr int kThreads = 256;

// What the stages read and write: one record per spectrum on the chirp path, then one per distinct N (the filter's).
// Every pointer is device memory.
struct AnyJob {
    const double2 *x;   // x': T traces of n_in points                      (a spectrum's record)
    double2 *a;         // T planes of M: a, later P                        (a filter's record: b, one plane)
    const double2 *A;   // T planes of M as the transform kernels store: A, later fft(P)
    const double2 *B;   // one plane of M as the transform kernels store
    double2 *z;         // T traces of N points of the main job table's Z
    const FidTw *c;     // the chirp table of N
    double inv_m;       // 1 / M
    int32_t N, M, n_in, T;
};

enum { kLoad = 0, kFilter = 1, kProduct = 2, kStore = 3, kAnyTables = 4 };

__global__ __launch_bounds__(kThreads) void fida_load_kernel(const AnyJob *__restrict__ jobs, const long long *__restrict__ pref, int K)
{
    ItemAt at;
    if (!item_at(pref, K, &at)) return;
    const AnyJob &q = jobs[at.k];
    const int M = q.M, n_in = q.n_in;
    long long t;
    int from;
    item_place(at.local(), M, &t, &from);
    const double2 *__restrict__ x = q.x + t * n_in;
    const FidTw *__restrict__ c = q.c;
    double2 *__restrict__ a = q.a + t * M;
    for (int i = from + (int)threadIdx.x; i < M && i < from + kFidChunk; i += kThreads) {
        double2 out = make_double2(0.0, 0.0);
        if (i < n_in) {
            const double2 val = x[i];
            const FidTw w = c[i];
            const Cx p = cmul(Cx{val.x, val.y}, Cx{w.re, w.im});
            out = make_double2(p.re, p.im);
        }
        a[i] = out;
    }
}

__global__ __launch_bounds__(kThreads) void fida_filter_kernel(const AnyJob *__restrict__ jobs, const long long *__restrict__ pref, int K)
{
    ItemAt at;
    if (!item_at(pref, K, &at)) return;
    const AnyJob &q = jobs[at.k];
    const int M = q.M, N = q.N;
    const int from = (int)at.local() * kFidChunk;
    const FidTw *__restrict__ c = q.c;
    double2 *__restrict__ b = q.a;
    for (int i = from + (int)threadIdx.x; i < M && i < from + kFidChunk; i += kThreads) {
        double2 out = make_double2(0.0, 0.0);
        const int at = i < N ? i : (M - i < N ? M - i : -1);   // (M >= 2 N - 1: the two runs do not meet)
        if (at >= 0) {
            const FidTw w = c[at];
            out = make_double2(w.re, -w.im);
        }
        b[i] = out;
    }
}

__global__ __launch_bounds__(kThreads) void fida_product_kernel(const AnyJob *__restrict__ jobs, const long long *__restrict__ pref,
                                                                int K)
{
    ItemAt at;
    if (!item_at(pref, K, &at)) return;
    const AnyJob &q = jobs[at.k];
    const int M = q.M, half = M >> 1;
    long long t;
    int from;
    item_place(at.local(), M, &t, &from);
    const double2 *__restrict__ A = q.A + t * M;
    const double2 *__restrict__ B = q.B;
    double2 *__restrict__ P = q.a + t * M;
    for (int i = from + (int)threadIdx.x; i < M && i < from + kFidChunk; i += kThreads) {
        const int e = M - 1 - (i ^ half);
        const double2 va = A[e], vb = B[e];
        const Cx out = cmul(Cx{va.x, va.y}, Cx{vb.x, vb.y});
        P[i] = make_double2(out.re, out.im);
    }
}

__global__ __launch_bounds__(kThreads) void fida_store_kernel(const AnyJob *__restrict__ jobs, const long long *__restrict__ pref, int K)
{
    ItemAt at;
    if (!item_at(pref, K, &at)) return;
    const AnyJob &q = jobs[at.k];
    const int M = q.M, half = M >> 1, N = q.N, turn = N - (N >> 1);
    const double inv_m = q.inv_m;
    long long t;
    int from;
    item_place(at.local(), N, &t, &from);
    const double2 *__restrict__ p = q.A + t * M;
    const FidTw *__restrict__ c = q.c;
    double2 *__restrict__ z = q.z + t * N;
    for (int j = from + (int)threadIdx.x; j < N && j < from + kFidChunk; j += kThreads) {
        // Z[j] = Y[i], i = N - 1 - j;  Y[i] = X[(i + N - floor(N/2)) mod N]
        int xq = N - 1 - j + turn;
        if (xq >= N) xq -= N;
        // p[xq] = fft(P)[(M - xq) mod M] / M, and entry e of fft(P) is at M - 1 - (e ^ M/2)
        const double2 val = p[M - 1 - (((M - xq) & (M - 1)) ^ half)];
        const FidTw w = c[xq];
        const Cx out = cmul(Cx{val.x * inv_m, val.y * inv_m}, Cx{w.re, w.im});
        z[j] = make_double2(out.re, out.im);
    }
}

}  // namespace

int64_t fid_any_conv_length(int64_t N) { return (int64_t)1 << fid_chirp_log2(N); }

int64_t fid_any_values(const FidAnyAsk *asks, size_t count)
{
    std::map<int64_t, int> seen;
    int64_t values = 0;
    for (size_t i = 0; i < count; ++i) {
        const int64_t M = fid_any_conv_length(asks[i].N);
        values += 2 * (int64_t)asks[i].T * M;
        if (seen.emplace(asks[i].N, 0).second) values += 2 * M;
    }
    return values;
}

struct FidAnyStage::Impl {
    std::vector<FidAnyAsk> asks;
    std::vector<int64_t> lengths;       // the distinct N in the order of their first spectrum
    std::vector<size_t> length_of;      // ask -> its entry of `lengths`
    std::vector<size_t> chirp_at;       // distinct N -> its first entry of `chirp`
    std::vector<FidTw> chirp;           // the chirp tables, one after the other
    std::vector<FidShape> shapes_ab;    // the first transforms: every spectrum's a (T planes), then every filter (T = 1)
    FidPlan plan_ab, plan_p;            // ... and the transform of P: the spectra alone
    ItemTables tab;                     // kAnyTables prefix tables over the records
    size_t o_jobs_ab = 0, o_jobs_p = 0, o_pref_ab = 0, o_pref_p = 0, o_recs = 0, o_pref = 0, o_chirp = 0, o_a = 0, o_z = 0, o_work = 0;
    // device memory, set by upload()
    const FidJob *d_jobs_ab = nullptr, *d_jobs_p = nullptr;
    const long long *d_pref_ab = nullptr, *d_pref_p = nullptr, *d_pref = nullptr;
    const AnyJob *d_recs = nullptr;
    size_t records() const { return asks.size() + lengths.size(); }
};

FidAnyStage::FidAnyStage() : impl_(new Impl) {}
FidAnyStage::~FidAnyStage() { delete impl_; }

void FidAnyStage::plan(const std::vector<FidAnyAsk> &asks)
{
    Impl &s = *impl_;
    s.asks = asks;
    if (asks.empty()) return;
    std::map<int64_t, size_t> seen;
    for (const FidAnyAsk &a : asks) {
        auto it = seen.find(a.N);
        if (it == seen.end()) {
            it = seen.emplace(a.N, s.lengths.size()).first;
            s.lengths.push_back(a.N);
            s.chirp_at.push_back(s.chirp.size());
            s.chirp.resize(s.chirp.size() + (size_t)a.N);
            fid_fill_chirp_table(a.N, s.chirp.data() + s.chirp_at.back());
        }
        s.length_of.push_back(it->second);
    }
    const size_t na = asks.size(), nr = s.records();
    for (const FidAnyAsk &a : asks) {
        const int64_t M = fid_any_conv_length(a.N);
        s.shapes_ab.push_back(FidShape{M, M, a.T});
    }
    for (int64_t N : s.lengths) {
        const int64_t M = fid_any_conv_length(N);
        s.shapes_ab.push_back(FidShape{M, M, 1});
    }
    s.plan_ab = fid_plan(s.shapes_ab.data(), nr);
    s.plan_p = fid_plan(s.shapes_ab.data(), na);
    s.tab = ItemTables(kAnyTables, nr);
    for (size_t r = 0; r < nr; ++r) {
        const bool spectrum = r < na;
        const int64_t M = s.shapes_ab[r].n;
        const int64_t T = s.shapes_ab[r].T;
        s.tab.add(kLoad, r, spectrum ? trace_items(T, M) : 0);
        s.tab.add(kFilter, r, spectrum ? 0 : trace_items(1, M));
        s.tab.add(kProduct, r, spectrum ? trace_items(T, M) : 0);
        s.tab.add(kStore, r, spectrum ? trace_items(T, asks[r].N) : 0);
    }
}

void FidAnyStage::carve(Carver &c)
{
    Impl &s = *impl_;
    if (s.asks.empty()) return;
    const size_t na = s.asks.size(), nr = s.records();
    s.o_jobs_ab = c.take(nr * sizeof(FidJob));
    s.o_jobs_p = c.take(na * sizeof(FidJob));
    s.o_pref_ab = c.take(s.plan_ab.tab.bytes());
    s.o_pref_p = c.take(s.plan_p.tab.bytes());
    s.o_recs = c.take(nr * sizeof(AnyJob));
    s.o_pref = c.take(s.tab.bytes());
    s.o_chirp = c.take(s.chirp.size() * sizeof(FidTw));
    s.o_a = c.take((size_t)s.plan_ab.values * sizeof(double2));      // a / P of every spectrum, then b of every distinct N
    s.o_z = c.take((size_t)s.plan_ab.values * sizeof(double2));      // A / fft(P) of every spectrum, then B
    s.o_work = c.take((size_t)s.plan_ab.work_values * sizeof(double2));
}

hipError_t FidAnyStage::upload(unsigned char *base, const double2 *const *x_of, double2 *const *z_of, hipStream_t st)
{
    Impl &s = *impl_;
    if (s.asks.empty()) return hipSuccess;
    const size_t na = s.asks.size(), nr = s.records();
    double2 *d_a = reinterpret_cast<double2 *>(base + s.o_a), *d_z = reinterpret_cast<double2 *>(base + s.o_z);
    const FidTw *d_chirp = reinterpret_cast<const FidTw *>(base + s.o_chirp);
    // both job tables cut the same buffers: the spectra come first in both, so the transform of P finds every P where the
    // first transform found a, and stores over A
    const FidBuffers buf{reinterpret_cast<double2 *>(base + s.o_work), d_z, nullptr, nullptr, nullptr, nullptr};
    std::vector<const double2 *> x_planes(nr);
    std::vector<size_t> plane_at(nr);
    {
        size_t at = 0;
        for (size_t r = 0; r < nr; ++r) {
            plane_at[r] = at;
            x_planes[r] = d_a + at;
            at += (size_t)s.shapes_ab[r].T * (size_t)s.shapes_ab[r].n;
        }
    }
    const std::vector<FidJob> jobs_ab = fid_job_table(s.plan_ab, s.shapes_ab.data(), x_planes.data(), buf),
                              jobs_p = fid_job_table(s.plan_p, s.shapes_ab.data(), x_planes.data(), buf);
    std::vector<AnyJob> recs(nr);
    for (size_t r = 0; r < nr; ++r) {
        const bool spectrum = r < na;
        const size_t d = spectrum ? s.length_of[r] : r - na;
        const int64_t N = s.lengths[d], M = s.shapes_ab[r].n;
        recs[r] = AnyJob{spectrum ? x_of[r] : nullptr,
                         d_a + plane_at[r],
                         spectrum ? d_z + plane_at[r] : nullptr,
                         spectrum ? d_z + plane_at[na + d] : nullptr,
                         spectrum ? z_of[r] : nullptr,
                         d_chirp + s.chirp_at[d],
                         1.0 / (double)M,
                         (int32_t)N,
                         (int32_t)M,
                         spectrum ? (int32_t)s.asks[r].n_in : 0,
                         s.shapes_ab[r].T};
    }
    FidJob *d_jobs_ab = reinterpret_cast<FidJob *>(base + s.o_jobs_ab), *d_jobs_p = reinterpret_cast<FidJob *>(base + s.o_jobs_p);
    long long *d_pref_ab = reinterpret_cast<long long *>(base + s.o_pref_ab), *d_pref_p = reinterpret_cast<long long *>(base + s.o_pref_p),
              *d_pref = reinterpret_cast<long long *>(base + s.o_pref);
    AnyJob *d_recs = reinterpret_cast<AnyJob *>(base + s.o_recs);
    // (pageable host memory: the copies have left the host arrays when hipMemcpyAsync returns)
    hipError_t e;
    if ((e = hipMemcpyAsync(d_jobs_ab, jobs_ab.data(), nr * sizeof(FidJob), hipMemcpyHostToDevice, st)) != hipSuccess) return e;
    if ((e = hipMemcpyAsync(d_jobs_p, jobs_p.data(), na * sizeof(FidJob), hipMemcpyHostToDevice, st)) != hipSuccess) return e;
    if ((e = hipMemcpyAsync(d_pref_ab, s.plan_ab.tab.pref.data(), s.plan_ab.tab.bytes(), hipMemcpyHostToDevice, st)) != hipSuccess) return e;
    if ((e = hipMemcpyAsync(d_pref_p, s.plan_p.tab.pref.data(), s.plan_p.tab.bytes(), hipMemcpyHostToDevice, st)) != hipSuccess) return e;
    if ((e = hipMemcpyAsync(d_recs, recs.data(), nr * sizeof(AnyJob), hipMemcpyHostToDevice, st)) != hipSuccess) return e;
    if ((e = hipMemcpyAsync(d_pref, s.tab.pref.data(), s.tab.bytes(), hipMemcpyHostToDevice, st)) != hipSuccess) return e;
    if ((e = hipMemcpyAsync(const_cast<FidTw *>(d_chirp), s.chirp.data(), s.chirp.size() * sizeof(FidTw), hipMemcpyHostToDevice, st)) != hipSuccess) return e;
    s.d_jobs_ab = d_jobs_ab;
    s.d_jobs_p = d_jobs_p;
    s.d_pref_ab = d_pref_ab;
    s.d_pref_p = d_pref_p;
    s.d_pref = d_pref;
    s.d_recs = d_recs;
    return hipSuccess;
}

hipError_t FidAnyStage::launch(const FidDeviceTables &tables, hipStream_t st) const
{
    const Impl &s = *impl_;
    if (s.asks.empty()) return hipSuccess;
    const int R = (int)s.records();
    const auto stage = [&](void (*kernel)(const AnyJob *, const long long *, int), int which) {
        return launch_items(kernel, s.tab.items(which), kThreads, 0, st, s.d_recs, s.tab.device(s.d_pref, which), R);
    };
    hipError_t e;
    // ---- ten launches: (a), (b), the transforms of a and b (3), (c), the transform of P (3), (d)
    if ((e = stage(fida_load_kernel, kLoad)) != hipSuccess) return e;
    if ((e = stage(fida_filter_kernel, kFilter)) != hipSuccess) return e;
    if ((e = fid_launch_transforms(s.plan_ab, s.d_jobs_ab, s.d_pref_ab, tables, st)) != hipSuccess) return e;
    if ((e = stage(fida_product_kernel, kProduct)) != hipSuccess) return e;
    if ((e = fid_launch_transforms(s.plan_p, s.d_jobs_p, s.d_pref_p, tables, st)) != hipSuccess) return e;
    return stage(fida_store_kernel, kStore);
}

}  // namespace nmrfit

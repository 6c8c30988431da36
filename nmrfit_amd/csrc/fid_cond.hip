// fid_cond.hip -- the conditioning of raw FIDs between "FID in memory" and the transform, on the GPU (opt-in;
// include/nmrfit_amd_fid_cond.h holds the definition): the removal of a Bruker group delay in its two forms and a window.
// The transforms are fid.hip's, launched through fid_internal.h on job tables made here; the call's body (fid_call.hip)
// composes the stage (FidCondStage) with the main transform.
//   fidc_ramp_kernel       form 1: B[q] = X[q] rho_s(q) in natural order; X is read through the permutation the transform
//                          kernels store with: X[q] is entry s - 1 - (q ^ s/2) of the trace
//   fidc_store_kernel      form 1: y[j] = fft(B)[(-j) mod s] / s read through the same permutation, folded, truncated to
//                          s - skip points and multiplied by the window: the trace as the main transform loads it
//   fidc_window_kernel     no form 1: x'[j] = x[j] W[j]
//   fidc_spectrum_kernel   form 2: Z[j] <- Z[j] rho_n(n - 1 - j) in place (the device holds Z_t[j] = Y_t[n - 1 - j])
// Every launch is a flat list of work items (1024 points of a trace) over the spectra that need the stage, found by the
// prefix-table search of fid.hip; a spectrum contributes no items to a stage it does not need and a launch without items
// is not made.  Both permuted reads flip the top bit of the index and reverse the order: 64 consecutive lanes read 64
// consecutive values (descending for the ramp stage, ascending for the store), so neither side of a stage is strided.
// No LDS, no atomics, no scratch memory.  The ramp values are the double-double product of fid_ramp.h.
#include "fid_device.h"
#include "fid_internal.h"
#include "fid_ramp.h"
#include "nmrfit_amd_fid_cond.h"

#include <cstring>
#include <map>
#include <utility>
#include <vector>

namespace nmrfit {
namespace {

#pragma clang fp contract(off)   // (every product and sum of the definition is rounded once)

constexpr int kThreads = 256;
static_assert(NMRFIT_FID_FORM_FID == 1, "FidCondAsk::conditioned() names the form by its number");

// What the stages of one spectrum read and write.  Every pointer is device memory; a stage the spectrum does not need
// leaves its pointers null and has no items.
struct CondJob {
    const double2 *x;        // the traces as uploaded: T of s points
    const double2 *p;        // form 1: what the transform kernels stored, T traces of s points (first X, later fft(B))
    double2 *b;              // form 1: B in natural order, T traces of s points
    double2 *cond;           // the conditioned traces: T of n_out points
    double2 *z;              // form 2: Z of the main transform, T traces of n points
    const double *w;         // the window (n_out doubles) or null
    const FidTwDD *hi, *lo;  // the ramp tables: of (g, s) in form 1, of (g, n) in form 2
    double inv_s;            // 1 / s
    int32_t s, n_out, n, T, add;
};

enum { kRamp = 0, kStore = 1, kWindow = 2, kSpectrum = 3, kCondTables = 4 };

__global__ __launch_bounds__(kThreads) void fidc_ramp_kernel(const CondJob *__restrict__ jobs, const long long *__restrict__ pref,
                                                             int K)
{
    ItemAt at;
    if (!item_at(pref, K, &at)) return;
    const CondJob &q = jobs[at.k];
    const int s = q.s, half = s >> 1;
    long long t;
    int from;
    item_place(at.local(), s, &t, &from);
    const double2 *__restrict__ p = q.p + t * s;
    double2 *__restrict__ b = q.b + t * s;
    for (int i = from + (int)threadIdx.x; i < s && i < from + kFidChunk; i += kThreads) {
        const double2 val = p[s - 1 - (i ^ half)];
        const FidTw w = fid_ramp_value(q.hi, q.lo, i);
        const Cx out = cmul(Cx{val.x, val.y}, Cx{w.re, w.im});
        b[i] = make_double2(out.re, out.im);
    }
}

__global__ __launch_bounds__(kThreads) void fidc_store_kernel(const CondJob *__restrict__ jobs, const long long *__restrict__ pref,
                                                              int K)
{
    ItemAt at;
    if (!item_at(pref, K, &at)) return;
    const CondJob &q = jobs[at.k];
    const int s = q.s, half = s >> 1, n_out = q.n_out, add = q.add;
    const double inv_s = q.inv_s;
    long long t;
    int from;
    item_place(at.local(), n_out, &t, &from);
    const double2 *__restrict__ p = q.p + t * s;
    const double *__restrict__ w = q.w;
    double2 *__restrict__ cond = q.cond + t * n_out;
    for (int j = from + (int)threadIdx.x; j < n_out && j < from + kFidChunk; j += kThreads) {
        // y[j] = fft(B)[(s - j) mod s] / s, and entry e of fft(B) is at s - 1 - (e ^ s/2)
        const double2 a = p[s - 1 - (((s - j) & (s - 1)) ^ half)];
        double re = a.x * inv_s, im = a.y * inv_s;
        if (j < add) {   // the fold: + y[s - 1 - j] = fft(B)[j + 1] / s   (j + 1 <= add < s)
            const double2 f = p[s - 1 - ((j + 1) ^ half)];
            re = re + f.x * inv_s;
            im = im + f.y * inv_s;
        }
        if (w) {
            const double wj = w[j];
            re = re * wj;
            im = im * wj;
        }
        cond[j] = make_double2(re, im);
    }
}

__global__ __launch_bounds__(kThreads) void fidc_window_kernel(const CondJob *__restrict__ jobs, const long long *__restrict__ pref,
                                                               int K)
{
    ItemAt at;
    if (!item_at(pref, K, &at)) return;
    const CondJob &q = jobs[at.k];
    const int n_out = q.n_out;
    long long t;
    int from;
    item_place(at.local(), n_out, &t, &from);
    const double2 *__restrict__ x = q.x + t * n_out;
    const double *__restrict__ w = q.w;
    double2 *__restrict__ cond = q.cond + t * n_out;
    for (int j = from + (int)threadIdx.x; j < n_out && j < from + kFidChunk; j += kThreads) {
        const double2 a = x[j];
        const double wj = w[j];
        cond[j] = make_double2(a.x * wj, a.y * wj);
    }
}

__global__ __launch_bounds__(kThreads) void fidc_spectrum_kernel(const CondJob *__restrict__ jobs, const long long *__restrict__ pref,
                                                                 int K)
{
    ItemAt at;
    if (!item_at(pref, K, &at)) return;
    const CondJob &q = jobs[at.k];
    const int n = q.n;
    long long t;
    int from;
    item_place(at.local(), n, &t, &from);
    double2 *__restrict__ z = q.z + t * n;
    for (int j = from + (int)threadIdx.x; j < n && j < from + kFidChunk; j += kThreads) {
        const double2 val = z[j];
        const FidTw w = fid_ramp_value(q.hi, q.lo, n - 1 - j);   // (Z[j] is Y[n - 1 - j])
        const Cx out = cmul(Cx{val.x, val.y}, Cx{w.re, w.im});
        z[j] = make_double2(out.re, out.im);
    }
}

}  // namespace

struct FidCondStage::Impl {
    std::vector<FidCondAsk> asks;
    std::vector<size_t> window_at;
    std::vector<FidShape> shapes1;      // form 1's two transforms of length s over its own spectra
    FidPlan plan1;
    ItemTables tab;                     // kCondTables prefix tables over the spectra of the call
    std::vector<FidTwDD> ramps;         // the ramp tables: one pair per distinct (g, n) of the call
    std::vector<size_t> ramp_of;        // spectrum -> its pair's first entry of `ramps`
    int64_t cond_values = 0;            // sum T n_out over the conditioned spectra
    std::vector<const double2 *> x_main;
    size_t o_jobs_a = 0, o_jobs_b = 0, o_pref1 = 0, o_cjobs = 0, o_cpref = 0, o_ramps = 0, o_win = 0, o_p = 0, o_b = 0, o_work1 = 0,
           o_cond = 0;
    // device memory, set by upload()
    const FidJob *d_jobs_a = nullptr, *d_jobs_b = nullptr;
    const long long *d_pref1 = nullptr, *d_cpref = nullptr;
    const CondJob *d_cjobs = nullptr;
    const double2 *d_cond = nullptr;
    static int ramp_log2(const FidCondAsk &a) { return a.form == NMRFIT_FID_FORM_FID ? a.lg_s : fid_log2_exact(a.n); }
};

FidCondStage::FidCondStage() : impl_(new Impl) {}
FidCondStage::~FidCondStage() { delete impl_; }
const double2 *const *FidCondStage::x_of() const { return impl_->x_main.data(); }

void FidCondStage::plan(const std::vector<FidCondAsk> &asks, const std::vector<size_t> &window_at)
{
    Impl &s = *impl_;
    s.asks = asks;
    s.window_at = window_at;
    const size_t nk = asks.size();
    s.tab = ItemTables(kCondTables, nk);
    std::map<std::pair<uint64_t, int>, size_t> ramp_at;   // (g's bits, log2 n) -> the pair's first entry in `ramps`
    s.ramp_of.assign(nk, 0);
    for (size_t k = 0; k < nk; ++k) {
        const FidCondAsk &a = asks[k];
        const bool f1 = a.form == NMRFIT_FID_FORM_FID;
        if (f1) s.shapes1.push_back(FidShape{a.n_in, a.n_in, a.T});
        s.tab.add(kRamp, k, f1 ? trace_items(a.T, a.n_in) : 0);
        s.tab.add(kStore, k, f1 ? trace_items(a.T, a.n_out) : 0);
        s.tab.add(kWindow, k, !f1 && a.window >= 0 ? trace_items(a.T, a.n_out) : 0);
        s.tab.add(kSpectrum, k, a.form == NMRFIT_FID_FORM_SPECTRUM ? trace_items(a.T, a.n) : 0);
        if (a.conditioned()) s.cond_values += (int64_t)a.T * a.n_out;
        if (a.form == NMRFIT_FID_FORM_NONE) continue;
        const int lg = Impl::ramp_log2(a);
        uint64_t bits;
        std::memcpy(&bits, &a.g, sizeof bits);
        const auto key = std::make_pair(bits, lg);
        auto it = ramp_at.find(key);
        if (it == ramp_at.end()) {
            const size_t at = s.ramps.size();
            s.ramps.resize(at + (size_t)fid_ramp_hi_count(lg) + (size_t)fid_ramp_lo_count(lg));
            fid_fill_ramp_tables(a.g, lg, s.ramps.data() + at, s.ramps.data() + at + fid_ramp_hi_count(lg));
            it = ramp_at.emplace(key, at).first;
        }
        s.ramp_of[k] = it->second;
    }
    s.plan1 = fid_plan(s.shapes1.data(), s.shapes1.size());
}

void FidCondStage::carve(Carver &c)
{
    Impl &s = *impl_;
    const size_t nk = s.asks.size(), nk1 = s.shapes1.size();
    s.o_jobs_a = c.take(nk1 * sizeof(FidJob));
    s.o_jobs_b = c.take(nk1 * sizeof(FidJob));
    s.o_pref1 = c.take(s.plan1.tab.bytes());
    s.o_cjobs = c.take(nk * sizeof(CondJob));
    s.o_cpref = c.take(s.tab.bytes());
    s.o_ramps = c.take(s.ramps.size() * sizeof(FidTwDD));
    s.o_win = c.take(s.window_at.back() * sizeof(double));
    s.o_p = c.take((size_t)s.plan1.values * sizeof(double2));
    s.o_b = c.take((size_t)s.plan1.values * sizeof(double2));
    s.o_work1 = c.take((size_t)s.plan1.work_values * sizeof(double2));
    s.o_cond = c.take((size_t)s.cond_values * sizeof(double2));
}

hipError_t FidCondStage::upload(unsigned char *base, const double2 *d_x, double2 *d_z, const double *windows, hipStream_t st)
{
    Impl &s = *impl_;
    const size_t nk = s.asks.size(), nk1 = s.shapes1.size();
    FidJob *d_jobs_a = reinterpret_cast<FidJob *>(base + s.o_jobs_a), *d_jobs_b = reinterpret_cast<FidJob *>(base + s.o_jobs_b);
    long long *d_pref1 = reinterpret_cast<long long *>(base + s.o_pref1), *d_cpref = reinterpret_cast<long long *>(base + s.o_cpref);
    CondJob *d_cjobs = reinterpret_cast<CondJob *>(base + s.o_cjobs);
    FidTwDD *d_ramps = reinterpret_cast<FidTwDD *>(base + s.o_ramps);
    double *d_win = reinterpret_cast<double *>(base + s.o_win);
    double2 *d_p = reinterpret_cast<double2 *>(base + s.o_p), *d_b = reinterpret_cast<double2 *>(base + s.o_b),
            *d_cond = reinterpret_cast<double2 *>(base + s.o_cond);
    const FidBuffers buf1{reinterpret_cast<double2 *>(base + s.o_work1), d_p, nullptr, nullptr, nullptr, nullptr};
    std::vector<const double2 *> x_a(nk1), x_b(nk1);
    std::vector<CondJob> cjobs(nk);
    s.x_main.resize(nk);
    size_t at_x = 0, at_1 = 0, at_cond = 0, at_z = 0, i1 = 0;
    for (size_t k = 0; k < nk; ++k) {
        const FidCondAsk &a = s.asks[k];
        const size_t raw = (size_t)a.T * (size_t)a.n_in, out = (size_t)a.T * (size_t)a.n_out;
        CondJob &cj = cjobs[k];
        cj = CondJob{d_x + at_x, nullptr, nullptr, nullptr, nullptr, a.window >= 0 ? d_win + s.window_at[a.window] : nullptr,
                     nullptr, nullptr, 1.0 / (double)a.n_in, (int32_t)a.n_in, (int32_t)a.n_out, (int32_t)a.n, a.T, a.add};
        if (a.form != NMRFIT_FID_FORM_NONE) {
            cj.hi = d_ramps + s.ramp_of[k];
            cj.lo = cj.hi + fid_ramp_hi_count(Impl::ramp_log2(a));
        }
        if (a.form == NMRFIT_FID_FORM_FID) {
            cj.p = d_p + at_1;
            cj.b = d_b + at_1;
            x_a[i1] = d_x + at_x;
            x_b[i1] = d_b + at_1;
            at_1 += raw;
            ++i1;
        }
        if (a.form == NMRFIT_FID_FORM_SPECTRUM) cj.z = d_z + at_z;
        if (a.conditioned()) {
            cj.cond = d_cond + at_cond;
            at_cond += out;
        }
        s.x_main[k] = a.conditioned() ? cj.cond : d_x + at_x;
        at_x += raw;
        at_z += (size_t)a.T * (size_t)a.n;
    }
    // (pageable host memory: the copies have left the host arrays when hipMemcpyAsync returns)
    hipError_t e;
    if (nk1) {
        const std::vector<FidJob> jobs_a = fid_job_table(s.plan1, s.shapes1.data(), x_a.data(), buf1),
                                  jobs_b = fid_job_table(s.plan1, s.shapes1.data(), x_b.data(), buf1);
        if ((e = hipMemcpyAsync(d_jobs_a, jobs_a.data(), nk1 * sizeof(FidJob), hipMemcpyHostToDevice, st)) != hipSuccess) return e;
        if ((e = hipMemcpyAsync(d_jobs_b, jobs_b.data(), nk1 * sizeof(FidJob), hipMemcpyHostToDevice, st)) != hipSuccess) return e;
        if ((e = hipMemcpyAsync(d_pref1, s.plan1.tab.pref.data(), s.plan1.tab.bytes(), hipMemcpyHostToDevice, st)) != hipSuccess) return e;
    }
    if (s.tab.items(kRamp) || s.tab.items(kWindow) || s.tab.items(kSpectrum)) {
        if ((e = hipMemcpyAsync(d_cjobs, cjobs.data(), nk * sizeof(CondJob), hipMemcpyHostToDevice, st)) != hipSuccess) return e;
        if ((e = hipMemcpyAsync(d_cpref, s.tab.pref.data(), s.tab.bytes(), hipMemcpyHostToDevice, st)) != hipSuccess) return e;
    }
    if (!s.ramps.empty() &&
        (e = hipMemcpyAsync(d_ramps, s.ramps.data(), s.ramps.size() * sizeof(FidTwDD), hipMemcpyHostToDevice, st)) != hipSuccess)
        return e;
    if (s.window_at.back() &&
        (e = hipMemcpyAsync(d_win, windows, s.window_at.back() * sizeof(double), hipMemcpyHostToDevice, st)) != hipSuccess)
        return e;
    s.d_jobs_a = d_jobs_a;
    s.d_jobs_b = d_jobs_b;
    s.d_pref1 = d_pref1;
    s.d_cpref = d_cpref;
    s.d_cjobs = d_cjobs;
    s.d_cond = d_cond;
    return hipSuccess;
}

// form 1: the transform of the traces, the ramp, the transform back, the store; then the window of the others
hipError_t FidCondStage::launch_before(const FidDeviceTables &tables, hipStream_t st) const
{
    const Impl &s = *impl_;
    const int K = (int)s.asks.size();
    const auto stage = [&](void (*kernel)(const CondJob *, const long long *, int), int which) {
        return launch_items(kernel, s.tab.items(which), kThreads, 0, st, s.d_cjobs, s.tab.device(s.d_cpref, which), K);
    };
    hipError_t e;
    if (s.tab.items(kRamp)) {
        if ((e = fid_launch_transforms(s.plan1, s.d_jobs_a, s.d_pref1, tables, st)) != hipSuccess) return e;
        if ((e = stage(fidc_ramp_kernel, kRamp)) != hipSuccess) return e;
        if ((e = fid_launch_transforms(s.plan1, s.d_jobs_b, s.d_pref1, tables, st)) != hipSuccess) return e;
        if ((e = stage(fidc_store_kernel, kStore)) != hipSuccess) return e;
    }
    return stage(fidc_window_kernel, kWindow);
}

// form 2: the ramp on the main transform's Z
hipError_t FidCondStage::launch_after(hipStream_t st) const
{
    const Impl &s = *impl_;
    return launch_items(fidc_spectrum_kernel, s.tab.items(kSpectrum), kThreads, 0, st, s.d_cjobs, s.tab.device(s.d_cpref, kSpectrum),
                        (int)s.asks.size());
}

// Runs of consecutive conditioned spectra are contiguous on both sides: one copy each; a spectrum with nothing asked
// enters the main transform as it was given.
int FidCondStage::download(int device, hipStream_t st, const double *fid, double *conditioned_out) const
{
    const Impl &s = *impl_;
    const size_t nk = s.asks.size();
    size_t at_out = 0, at_x = 0, at_cond = 0, k = 0;
    while (k < nk) {
        const bool dev = s.asks[k].conditioned();
        size_t vals = 0, raw = 0;
        for (; k < nk && s.asks[k].conditioned() == dev; ++k) {
            vals += (size_t)s.asks[k].T * (size_t)s.asks[k].n_out;
            raw += (size_t)s.asks[k].T * (size_t)s.asks[k].n_in;
        }
        if (dev) {
            const int rc = staged_d2h(device, st, conditioned_out + 2 * at_out, s.d_cond + at_cond, vals * sizeof(double2));
            if (rc != NMRFIT_OK) return rc;
            at_cond += vals;
        } else {
            std::memcpy(conditioned_out + 2 * at_out, fid + 2 * at_x, vals * sizeof(double2));
        }
        at_out += vals;
        at_x += raw;
    }
    return NMRFIT_OK;
}

}  // namespace nmrfit

// fid_cond.hip -- the conditioning of raw FIDs between "FID in memory" and the transform, on the GPU (opt-in;
// include/nmrfit_amd_fid_cond.h holds the definition): the removal of a Bruker group delay in its two forms and a window.
// The transforms and the finishing stage are fid.hip's, launched through fid_internal.h on job tables made here.
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
#include "fid_any_internal.h"
#include "fid_device.h"
#include "fid_internal.h"
#include "fid_ramp.h"
#include "nmrfit_amd_fid_cond.h"
#include "weights_internal.h"

#include <cmath>
#include <cstring>
#include <map>
#include <string>
#include <utility>
#include <vector>

namespace nmrfit {
namespace {

#pragma clang fp contract(off)   // (every product and sum of the definition is rounded once)

constexpr int kThreads = 256;
constexpr int kRow = NMRFIT_FID_ROW;
constexpr int kLgMax = NMRFIT_FID_MAX_LOG2;
constexpr int kChunk = 1024;   // points of a trace per work item

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

// the item's trace and first point: a trace of `len` points is ceil(len / 1024) items
__device__ __forceinline__ void item_place(long long local, int len, long long *t, int *from)
{
    const int chunks = (len + kChunk - 1) / kChunk;
    *t = local / chunks;
    *from = (int)(local - *t * chunks) * kChunk;
}

__global__ __launch_bounds__(kThreads) void fidc_ramp_kernel(const CondJob *__restrict__ jobs, const long long *__restrict__ pref,
                                                             int K)
{
    const long long item = work_item(pref[K]);
    if (item < 0) return;
    const int k = find_job(pref, K, item);
    const CondJob &q = jobs[k];
    const int s = q.s, half = s >> 1;
    long long t;
    int from;
    item_place(item - pref[k], s, &t, &from);
    const double2 *__restrict__ p = q.p + t * s;
    double2 *__restrict__ b = q.b + t * s;
    for (int i = from + (int)threadIdx.x; i < s && i < from + kChunk; i += kThreads) {
        const double2 val = p[s - 1 - (i ^ half)];
        const FidTw w = fid_ramp_value(q.hi, q.lo, i);
        const Cx out = cmul(Cx{val.x, val.y}, Cx{w.re, w.im});
        b[i] = make_double2(out.re, out.im);
    }
}

__global__ __launch_bounds__(kThreads) void fidc_store_kernel(const CondJob *__restrict__ jobs, const long long *__restrict__ pref,
                                                              int K)
{
    const long long item = work_item(pref[K]);
    if (item < 0) return;
    const int k = find_job(pref, K, item);
    const CondJob &q = jobs[k];
    const int s = q.s, half = s >> 1, n_out = q.n_out, add = q.add;
    const double inv_s = q.inv_s;
    long long t;
    int from;
    item_place(item - pref[k], n_out, &t, &from);
    const double2 *__restrict__ p = q.p + t * s;
    const double *__restrict__ w = q.w;
    double2 *__restrict__ cond = q.cond + t * n_out;
    for (int j = from + (int)threadIdx.x; j < n_out && j < from + kChunk; j += kThreads) {
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
    const long long item = work_item(pref[K]);
    if (item < 0) return;
    const int k = find_job(pref, K, item);
    const CondJob &q = jobs[k];
    const int n_out = q.n_out;
    long long t;
    int from;
    item_place(item - pref[k], n_out, &t, &from);
    const double2 *__restrict__ x = q.x + t * n_out;
    const double *__restrict__ w = q.w;
    double2 *__restrict__ cond = q.cond + t * n_out;
    for (int j = from + (int)threadIdx.x; j < n_out && j < from + kChunk; j += kThreads) {
        const double2 a = x[j];
        const double wj = w[j];
        cond[j] = make_double2(a.x * wj, a.y * wj);
    }
}

__global__ __launch_bounds__(kThreads) void fidc_spectrum_kernel(const CondJob *__restrict__ jobs, const long long *__restrict__ pref,
                                                                 int K)
{
    const long long item = work_item(pref[K]);
    if (item < 0) return;
    const int k = find_job(pref, K, item);
    const CondJob &q = jobs[k];
    const int n = q.n;
    long long t;
    int from;
    item_place(item - pref[k], n, &t, &from);
    double2 *__restrict__ z = q.z + t * n;
    for (int j = from + (int)threadIdx.x; j < n && j < from + kChunk; j += kThreads) {
        const double2 val = z[j];
        const FidTw w = fid_ramp_value(q.hi, q.lo, n - 1 - j);   // (Z[j] is Y[n - 1 - j])
        const Cx out = cmul(Cx{val.x, val.y}, Cx{w.re, w.im});
        z[j] = make_double2(out.re, out.im);
    }
}

long long trace_items(int64_t T, int64_t len) { return T * ((len + kChunk - 1) / kChunk); }

// the jobs of a call as the checks leave them
struct Asked {
    int32_t form = 0, window = -1, lg_s = 0, add = 0;
    int64_t n_out = 0;
    bool conditioned() const { return form == NMRFIT_FID_FORM_FID || window >= 0; }
};

}  // namespace

int fid_condition_transform_run(const std::string &who, bool any_length, int device, int32_t K, const int64_t *n_in, const int64_t *n,
                                const int32_t *T, const double *fid, const int32_t *form, const double *g, const int32_t *window_of,
                                int32_t M, const int64_t *window_len, const double *windows, double *u_out, double *v_out,
                                double *rows_out, double *transform_out, double *conditioned_out)
{
    if (K <= 0 || !n_in || !n || !T || !fid || !form || !g || !window_of || !u_out || !v_out || !rows_out)
        return refuse(NMRFIT_E_INVALID, who + ": the number of spectra must be > 0 and n_in, n, T, fid, form, g, window_of, u_out, "
                                              "v_out, rows_out non-null");
    if (M < 0 || (M > 0 && (!window_len || !windows)))
        return refuse(NMRFIT_E_INVALID, who + ": the number of windows must be >= 0, and window_len and windows non-null when it is > 0");
    std::vector<size_t> window_at((size_t)M + 1, 0);
    for (int32_t m = 0; m < M; ++m) {
        if (window_len[m] <= 0 || window_len[m] > ((int64_t)1 << kLgMax))
            return refuse(NMRFIT_E_INVALID, who + ": a window has 1 .. 2^" + std::to_string(kLgMax) + " values (window " + std::to_string(m) + ")");
        window_at[m + 1] = window_at[m] + (size_t)window_len[m];
    }
    const size_t nk = (size_t)K;
    std::vector<Asked> asked(nk);
    for (int32_t k = 0; k < K; ++k) {
        const std::string at = " (spectrum " + std::to_string(k) + ")";
        Asked &a = asked[k];
        if (T[k] <= 0 || n_in[k] <= 0) return refuse(NMRFIT_E_INVALID, who + ": every spectrum needs T > 0 and n_in > 0" + at);
        if (form[k] < NMRFIT_FID_FORM_NONE || form[k] > NMRFIT_FID_FORM_SPECTRUM)
            return refuse(NMRFIT_E_INVALID, who + ": form is 0 (none), 1 (fid) or 2 (spectrum)" + at);
        a.form = form[k];
        a.n_out = n_in[k];
        if (a.form != NMRFIT_FID_FORM_NONE && !(std::isfinite(g[k]) && g[k] > 0.0))
            return refuse(NMRFIT_E_INVALID, who + ": a group delay is finite and > 0 where a form is set" + at);
        if (a.form == NMRFIT_FID_FORM_FID) {
            a.lg_s = fid_log2_exact(n_in[k]);
            if (a.lg_s < 1 || a.lg_s > kLgMax)
                return refuse(NMRFIT_E_UNSUPPORTED, who + ": form 1 (fid) needs a trace length that is a power of two, 2 .. 2^" +
                                                        std::to_string(kLgMax) + at + ": use form 2 (spectrum)");
            const double skip = std::floor(g[k] + 2.0);
            if (!((double)n_in[k] >= 2.0 * skip))
                return refuse(NMRFIT_E_INVALID, who + ": form 1 (fid) needs a trace of at least 2 floor(g + 2) points" + at);
            a.n_out = n_in[k] - (int64_t)skip;
            a.add = (int32_t)std::max<int64_t>((int64_t)skip - 6, 0);
        }
        if (window_of[k] < -1 || window_of[k] >= M) return refuse(NMRFIT_E_INVALID, who + ": window_of is -1 or the index of a window" + at);
        a.window = window_of[k];
        if (a.window >= 0 && window_len[a.window] != a.n_out)
            return refuse(NMRFIT_E_INVALID, who + ": a window has as many values as the conditioned trace has points" + at);
        if (n[k] < a.n_out)
            return refuse(NMRFIT_E_INVALID, who + ": a transform length is at least the conditioned trace's length" + at);
    }
    for (int32_t m = 0; m < M; ++m)
        for (size_t i = window_at[m]; i < window_at[m + 1]; ++i)
            if (!std::isfinite(windows[i]))
                return refuse(NMRFIT_E_INVALID, who + ": a window value is not finite (window " + std::to_string(m) + ")");
    const int64_t max_values = (int64_t)1 << 26;
    int64_t values = 0;
    std::vector<FidAnyAsk> asks;   // the spectra on the chirp path (any_length alone)
    std::vector<size_t> of_any;
    for (int32_t k = 0; k < K; ++k) {
        const int lg = fid_log2_exact(n[k]);
        const std::string at = " (spectrum " + std::to_string(k) + ")";
        if (any_length && lg < 0) {
            if (n[k] < kFidAnyMin || n[k] > kFidAnyMax)
                return refuse(NMRFIT_E_UNSUPPORTED, who + ": a transform length is a power of two, 2 .. 2^" + std::to_string(kLgMax) +
                                                        ", or any other length, 3 .. 2^21 - 1" + at);
            if (asked[k].form == NMRFIT_FID_FORM_SPECTRUM)
                return refuse(NMRFIT_E_UNSUPPORTED, who + ": form 2 (spectrum) needs a transform length that is a power of two" + at +
                                                        ": its ramp tables are split at 2^11; use form 1 (fid), or zero fill");
            asks.push_back(FidAnyAsk{n[k], asked[k].n_out, T[k]});
            of_any.push_back((size_t)k);
        } else if (lg < 1 || lg > kLgMax) {
            if (any_length)
                return refuse(NMRFIT_E_UNSUPPORTED, who + ": a transform length is a power of two, 2 .. 2^" + std::to_string(kLgMax) +
                                                        ", or any other length, 3 .. 2^21 - 1" + at);
            return refuse(NMRFIT_E_UNSUPPORTED, who + ": a transform length is a power of two, 2 .. 2^" + std::to_string(kLgMax) +
                                                    " (spectrum " + std::to_string(k) + "): zero fill to the next power of two");
        }
        if (values <= max_values)   // (each term < 2^54: the sum cannot overflow)
            values += (int64_t)T[k] * n[k] + (asked[k].form == NMRFIT_FID_FORM_FID ? (int64_t)T[k] * n_in[k] : 0);
    }
    const bool too_many = K > kWeightsMaxSpectra || values > max_values;
    if (!too_many && !asks.empty()) values += fid_any_values(asks.data(), asks.size());   // (K < 2^16 terms < 2^54)
    if (too_many || values > max_values)
        return refuse(NMRFIT_E_UNSUPPORTED, who + ": a call takes at most " + std::to_string(kWeightsMaxSpectra) + " spectra and " +
                                                std::to_string(max_values) + " transformed values (T n summed over the spectra, "
                                                "plus T n_in of those in form 1" +
                                                (any_length ? ", plus 2 T M of those whose n is no power of two and 2 M per distinct such n)" : ")"));
    int rc = use_device(device);
    if (rc != NMRFIT_OK) return rc;
    StreamLease lease(device);
    NMRFIT_HIP(lease.take());
    hipStream_t st = lease.s;

    // ---- the plans: the main transform over all spectra, form 1's two transforms over its own
    std::vector<FidShape> shapes(nk), shapes1;
    std::vector<size_t> of1;   // the spectra in form 1
    for (size_t k = 0; k < nk; ++k) {
        shapes[k] = FidShape{asked[k].n_out, n[k], T[k]};
        if (asked[k].form == NMRFIT_FID_FORM_FID) {
            shapes1.push_back(FidShape{n_in[k], n_in[k], T[k]});
            of1.push_back(k);
        }
    }
    const size_t nk1 = of1.size();
    const FidPlan plan = fid_plan(shapes.data(), nk), plan1 = fid_plan(shapes1.data(), nk1);
    FidAnyStage any;
    any.plan(asks);
    std::vector<long long> cpref((size_t)kCondTables * (nk + 1), 0);
    long long *p_ramp = cpref.data(), *p_store = p_ramp + nk + 1, *p_win = p_store + nk + 1, *p_spec = p_win + nk + 1;
    int64_t raw_values = 0, cond_values = 0;
    for (size_t k = 0; k < nk; ++k) {
        const Asked &a = asked[k];
        const bool f1 = a.form == NMRFIT_FID_FORM_FID;
        p_ramp[k + 1] = p_ramp[k] + (f1 ? trace_items(T[k], n_in[k]) : 0);
        p_store[k + 1] = p_store[k] + (f1 ? trace_items(T[k], a.n_out) : 0);
        p_win[k + 1] = p_win[k] + (!f1 && a.window >= 0 ? trace_items(T[k], a.n_out) : 0);
        p_spec[k + 1] = p_spec[k] + (a.form == NMRFIT_FID_FORM_SPECTRUM ? trace_items(T[k], n[k]) : 0);
        raw_values += (int64_t)T[k] * n_in[k];
        if (a.conditioned()) cond_values += (int64_t)T[k] * a.n_out;
    }

    // ---- the ramp tables: one pair per distinct (g, n) of the call
    std::map<std::pair<uint64_t, int>, size_t> ramp_at;   // (g's bits, log2 n) -> the pair's first entry in `ramps`
    std::vector<FidTwDD> ramps;
    std::vector<size_t> ramp_of(nk, 0);
    for (size_t k = 0; k < nk; ++k) {
        if (asked[k].form == NMRFIT_FID_FORM_NONE) continue;
        const int lg = asked[k].form == NMRFIT_FID_FORM_FID ? asked[k].lg_s : fid_log2_exact(n[k]);
        uint64_t bits;
        std::memcpy(&bits, &g[k], sizeof bits);
        const auto key = std::make_pair(bits, lg);
        auto it = ramp_at.find(key);
        if (it == ramp_at.end()) {
            const size_t at = ramps.size();
            ramps.resize(at + (size_t)fid_ramp_hi_count(lg) + (size_t)fid_ramp_lo_count(lg));
            fid_fill_ramp_tables(g[k], lg, ramps.data() + at, ramps.data() + at + fid_ramp_hi_count(lg));
            it = ramp_at.emplace(key, at).first;
        }
        ramp_of[k] = it->second;
    }

    // ---- one allocation for the call's buffers
    Scratch mem;
    Carver c;
    const size_t o_jobs = c.take(nk * sizeof(FidJob)), o_pref = c.take(plan.pref.size() * sizeof(long long));
    const size_t o_jobs_a = c.take(nk1 * sizeof(FidJob)), o_jobs_b = c.take(nk1 * sizeof(FidJob)),
                 o_pref1 = c.take(plan1.pref.size() * sizeof(long long));
    const size_t o_cjobs = c.take(nk * sizeof(CondJob)), o_cpref = c.take(cpref.size() * sizeof(long long));
    const size_t o_tw = c.take(kFidStage * sizeof(FidTw)), o_hi = c.take(kFidSplit * sizeof(FidTwDD)),
                 o_lo = c.take(kFidSplit * sizeof(FidTwDD));
    const size_t o_ramps = c.take(ramps.size() * sizeof(FidTwDD)), o_win = c.take(window_at[M] * sizeof(double));
    const size_t o_x = c.take((size_t)raw_values * sizeof(double2));
    const size_t o_p = c.take((size_t)plan1.values * sizeof(double2)), o_b = c.take((size_t)plan1.values * sizeof(double2)),
                 o_work1 = c.take((size_t)plan1.work_values * sizeof(double2));
    const size_t o_cond = c.take((size_t)cond_values * sizeof(double2));
    const size_t o_work = c.take((size_t)plan.work_values * sizeof(double2)), o_z = c.take((size_t)plan.values * sizeof(double2));
    const size_t o_u = c.take((size_t)plan.points * sizeof(double)), o_v = c.take((size_t)plan.points * sizeof(double));
    const size_t o_rows = c.take(nk * kRow * sizeof(double)), o_part = c.take((size_t)plan.parts() * sizeof(double4));
    any.carve(c);
    unsigned char *base = nullptr;
    NMRFIT_HIP(mem.alloc(&base, c.total));
    FidJob *d_jobs = reinterpret_cast<FidJob *>(base + o_jobs), *d_jobs_a = reinterpret_cast<FidJob *>(base + o_jobs_a),
           *d_jobs_b = reinterpret_cast<FidJob *>(base + o_jobs_b);
    long long *d_pref = reinterpret_cast<long long *>(base + o_pref), *d_pref1 = reinterpret_cast<long long *>(base + o_pref1),
              *d_cpref = reinterpret_cast<long long *>(base + o_cpref);
    CondJob *d_cjobs = reinterpret_cast<CondJob *>(base + o_cjobs);
    const FidDeviceTables tables{reinterpret_cast<FidTw *>(base + o_tw), reinterpret_cast<FidTwDD *>(base + o_hi),
                                 reinterpret_cast<FidTwDD *>(base + o_lo)};
    FidTwDD *d_ramps = reinterpret_cast<FidTwDD *>(base + o_ramps);
    double *d_win = reinterpret_cast<double *>(base + o_win);
    double2 *d_x = reinterpret_cast<double2 *>(base + o_x), *d_p = reinterpret_cast<double2 *>(base + o_p),
            *d_b = reinterpret_cast<double2 *>(base + o_b), *d_cond = reinterpret_cast<double2 *>(base + o_cond);
    const FidBuffers buf{reinterpret_cast<double2 *>(base + o_work), reinterpret_cast<double2 *>(base + o_z),
                         reinterpret_cast<double *>(base + o_u),     reinterpret_cast<double *>(base + o_v),
                         reinterpret_cast<double *>(base + o_rows),  reinterpret_cast<double4 *>(base + o_part)};
    const FidBuffers buf1{reinterpret_cast<double2 *>(base + o_work1), d_p, nullptr, nullptr, nullptr, nullptr};

    // ---- the job tables
    std::vector<const double2 *> x_main(nk), x_a(nk1), x_b(nk1);
    std::vector<CondJob> cjobs(nk);
    {
        size_t at_x = 0, at_1 = 0, at_cond = 0, at_z = 0, i1 = 0;
        for (size_t k = 0; k < nk; ++k) {
            const Asked &a = asked[k];
            const size_t raw = (size_t)T[k] * (size_t)n_in[k], out = (size_t)T[k] * (size_t)a.n_out;
            CondJob &cj = cjobs[k];
            cj = CondJob{d_x + at_x, nullptr, nullptr, nullptr, nullptr, a.window >= 0 ? d_win + window_at[a.window] : nullptr,
                         nullptr, nullptr, 1.0 / (double)n_in[k], (int32_t)n_in[k], (int32_t)a.n_out, (int32_t)n[k], T[k], a.add};
            if (a.form != NMRFIT_FID_FORM_NONE) {
                const int lg = a.form == NMRFIT_FID_FORM_FID ? a.lg_s : fid_log2_exact(n[k]);
                cj.hi = d_ramps + ramp_of[k];
                cj.lo = cj.hi + fid_ramp_hi_count(lg);
            }
            if (a.form == NMRFIT_FID_FORM_FID) {
                cj.p = d_p + at_1;
                cj.b = d_b + at_1;
                x_a[i1] = d_x + at_x;
                x_b[i1] = d_b + at_1;
                at_1 += raw;
                ++i1;
            }
            if (a.form == NMRFIT_FID_FORM_SPECTRUM) cj.z = buf.z + at_z;
            if (a.conditioned()) {
                cj.cond = d_cond + at_cond;
                at_cond += out;
            }
            x_main[k] = a.conditioned() ? cj.cond : d_x + at_x;
            at_x += raw;
            at_z += (size_t)T[k] * (size_t)n[k];
        }
    }
    const std::vector<FidJob> jobs = fid_job_table(plan, shapes.data(), x_main.data(), buf);
    const std::vector<FidJob> jobs_a = fid_job_table(plan1, shapes1.data(), x_a.data(), buf1),
                              jobs_b = fid_job_table(plan1, shapes1.data(), x_b.data(), buf1);

    // ---- uploads (pageable host memory: the copies have left the host arrays when hipMemcpyAsync returns)
    NMRFIT_HIP(hipMemcpyAsync(d_jobs, jobs.data(), nk * sizeof(FidJob), hipMemcpyHostToDevice, st));
    NMRFIT_HIP(hipMemcpyAsync(d_pref, plan.pref.data(), plan.pref.size() * sizeof(long long), hipMemcpyHostToDevice, st));
    NMRFIT_HIP(fid_upload_tables(tables, st));
    NMRFIT_HIP(hipMemcpyAsync(d_x, fid, (size_t)raw_values * sizeof(double2), hipMemcpyHostToDevice, st));
    if (nk1) {
        NMRFIT_HIP(hipMemcpyAsync(d_jobs_a, jobs_a.data(), nk1 * sizeof(FidJob), hipMemcpyHostToDevice, st));
        NMRFIT_HIP(hipMemcpyAsync(d_jobs_b, jobs_b.data(), nk1 * sizeof(FidJob), hipMemcpyHostToDevice, st));
        NMRFIT_HIP(hipMemcpyAsync(d_pref1, plan1.pref.data(), plan1.pref.size() * sizeof(long long), hipMemcpyHostToDevice, st));
    }
    const bool any_stage = p_ramp[nk] || p_win[nk] || p_spec[nk];
    if (any_stage) {
        NMRFIT_HIP(hipMemcpyAsync(d_cjobs, cjobs.data(), nk * sizeof(CondJob), hipMemcpyHostToDevice, st));
        NMRFIT_HIP(hipMemcpyAsync(d_cpref, cpref.data(), cpref.size() * sizeof(long long), hipMemcpyHostToDevice, st));
    }
    if (!ramps.empty()) NMRFIT_HIP(hipMemcpyAsync(d_ramps, ramps.data(), ramps.size() * sizeof(FidTwDD), hipMemcpyHostToDevice, st));
    if (window_at[M]) NMRFIT_HIP(hipMemcpyAsync(d_win, windows, window_at[M] * sizeof(double), hipMemcpyHostToDevice, st));
    if (!asks.empty()) {
        std::vector<const double2 *> x_any(asks.size());
        std::vector<double2 *> z_any(asks.size());
        for (size_t i = 0; i < asks.size(); ++i) {
            x_any[i] = x_main[of_any[i]];
            z_any[i] = jobs[of_any[i]].z;
        }
        NMRFIT_HIP(any.upload(base, x_any.data(), z_any.data(), st));
    }

    // ---- the launches: at most 16, at most 27 with spectra on the chirp path
    const long long *d_ramp = d_cpref, *d_store = d_ramp + nk + 1, *d_window = d_store + nk + 1, *d_spec = d_window + nk + 1;
    const dim3 block(kThreads);
    if (p_ramp[nk]) {
        NMRFIT_HIP(fid_launch_transforms(plan1, d_jobs_a, d_pref1, tables, st));
        hipLaunchKernelGGL(fidc_ramp_kernel, fid_item_grid(p_ramp[nk]), block, 0, st, d_cjobs, d_ramp, (int)K);
        NMRFIT_HIP(hipGetLastError());
        NMRFIT_HIP(fid_launch_transforms(plan1, d_jobs_b, d_pref1, tables, st));
        hipLaunchKernelGGL(fidc_store_kernel, fid_item_grid(p_store[nk]), block, 0, st, d_cjobs, d_store, (int)K);
        NMRFIT_HIP(hipGetLastError());
    }
    if (p_win[nk]) {
        hipLaunchKernelGGL(fidc_window_kernel, fid_item_grid(p_win[nk]), block, 0, st, d_cjobs, d_window, (int)K);
        NMRFIT_HIP(hipGetLastError());
    }
    NMRFIT_HIP(fid_launch_transforms(plan, d_jobs, d_pref, tables, st));
    NMRFIT_HIP(any.launch(tables, plan, d_jobs, d_pref, st));
    if (p_spec[nk]) {
        hipLaunchKernelGGL(fidc_spectrum_kernel, fid_item_grid(p_spec[nk]), block, 0, st, d_cjobs, d_spec, (int)K);
        NMRFIT_HIP(hipGetLastError());
    }
    NMRFIT_HIP(fid_launch_finish(plan, d_jobs, d_pref, st));

    // ---- downloads
    if ((rc = staged_d2h(device, st, rows_out, buf.rows, nk * kRow * sizeof(double))) != NMRFIT_OK) return rc;
    if ((rc = staged_d2h(device, st, u_out, buf.u, (size_t)plan.points * sizeof(double))) != NMRFIT_OK) return rc;
    if ((rc = staged_d2h(device, st, v_out, buf.v, (size_t)plan.points * sizeof(double))) != NMRFIT_OK) return rc;
    if (transform_out && (rc = staged_d2h(device, st, transform_out, buf.z, (size_t)plan.values * sizeof(double2))) != NMRFIT_OK) return rc;
    if (conditioned_out) {
        // runs of consecutive conditioned spectra are contiguous on both sides: one copy each; a spectrum with nothing asked
        // enters the main transform as it was given
        size_t at_out = 0, at_x = 0, at_cond = 0, k = 0;
        while (k < nk) {
            const bool dev = asked[k].conditioned();
            size_t vals = 0, raw = 0;
            for (; k < nk && asked[k].conditioned() == dev; ++k) {
                vals += (size_t)T[k] * (size_t)asked[k].n_out;
                raw += (size_t)T[k] * (size_t)n_in[k];
            }
            if (dev) {
                if ((rc = staged_d2h(device, st, conditioned_out + 2 * at_out, d_cond + at_cond, vals * sizeof(double2))) != NMRFIT_OK) return rc;
                at_cond += vals;
            } else {
                std::memcpy(conditioned_out + 2 * at_out, fid + 2 * at_x, vals * sizeof(double2));
            }
            at_out += vals;
            at_x += raw;
        }
    }
    return NMRFIT_OK;
}

}  // namespace nmrfit

using namespace nmrfit;

#pragma GCC visibility push(default)   // the C-ABI: the only symbols the library exports (build.sh: -fvisibility=hidden)

int nmrfit_fid_condition_transform(int device, int32_t K, const int64_t *n_in, const int64_t *n, const int32_t *T,
                                   const double *fid, const int32_t *form, const double *g, const int32_t *window_of, int32_t M,
                                   const int64_t *window_len, const double *windows, double *u_out, double *v_out,
                                   double *rows_out, double *transform_out, double *conditioned_out)
{
    return fid_condition_transform_run("nmrfit_fid_condition_transform", false, device, K, n_in, n, T, fid, form, g, window_of, M,
                                       window_len, windows, u_out, v_out, rows_out, transform_out, conditioned_out);
}

#pragma GCC visibility pop

// fid_call.hip -- the three entry points of the raw-FID path (include/nmrfit_amd_fid.h, nmrfit_amd_fid_cond.h,
// nmrfit_amd_fid_any.h hold the definitions) and their one body: argument checks, plans, the plans of the two stages,
// the carve of the call's one allocation, uploads, launches, downloads.  An entry point is a descriptor -- its name, what
// it takes, and the few words of its messages that differ -- and one call of the body.  The kernels and the pieces of a
// call are fid.hip's, the conditioning fid_cond.hip's, the chirp path fid_any.hip's (fid_internal.h).  Host code.
//   the launches of a call: form 1's two transforms with the ramp and the store between and after them (at most 8), the
//   window (1), the main transform (at most 3), the chirp path (10), form 2's ramp (1), the finishing stage (3)
#include "fid_internal.h"
#include "nmrfit_amd_fid.h"
#include "nmrfit_amd_fid_any.h"
#include "nmrfit_amd_fid_cond.h"
#include "weights_internal.h"

#include <cmath>
#include <string>
#include <vector>

namespace nmrfit {
namespace {

constexpr int kRow = NMRFIT_FID_ROW;
constexpr int kLgMax = NMRFIT_FID_MAX_LOG2;

struct FidEntry {
    const char *name;
    bool cond;         // takes form, g, window_of and the windows (a plain call: form 0 and no window everywhere)
    bool any_length;   // sends the lengths that are no powers of two through the chirp stage
    const char *non_null, *at_least, *budget;   // the words of the messages that differ
};
constexpr FidEntry kPlain{"nmrfit_fid_transform", false, false, "n_in, n, T, fid, u_out, v_out, rows_out", "the trace's length",
                          "(T n summed over the spectra)"};
constexpr FidEntry kCond{"nmrfit_fid_condition_transform", true, false, "n_in, n, T, fid, form, g, window_of, u_out, v_out, rows_out",
                         "the conditioned trace's length", "(T n summed over the spectra, plus T n_in of those in form 1)"};
constexpr FidEntry kAny{"nmrfit_fid_transform_any", true, true, kCond.non_null, kCond.at_least,
                        "(T n summed over the spectra, plus T n_in of those in form 1, plus 2 T M of those whose n is no power of two "
                        "and 2 M per distinct such n)"};

int fid_call(const FidEntry &entry, int device, int32_t K, const int64_t *n_in, const int64_t *n, const int32_t *T, const double *fid,
             const int32_t *form, const double *g, const int32_t *window_of, int32_t M, const int64_t *window_len,
             const double *windows, double *u_out, double *v_out, double *rows_out, double *transform_out, double *conditioned_out)
{
    // ---- the argument checks, in the order of the headers
    const std::string who = entry.name;
    if (K <= 0 || !n_in || !n || !T || !fid || (entry.cond && (!form || !g || !window_of)) || !u_out || !v_out || !rows_out)
        return refuse(NMRFIT_E_INVALID, who + ": the number of spectra must be > 0 and " + entry.non_null + " non-null");
    if (M < 0 || (M > 0 && (!window_len || !windows)))
        return refuse(NMRFIT_E_INVALID, who + ": the number of windows must be >= 0, and window_len and windows non-null when it is > 0");
    std::vector<size_t> window_at((size_t)M + 1, 0);
    for (int32_t m = 0; m < M; ++m) {
        if (window_len[m] <= 0 || window_len[m] > ((int64_t)1 << kLgMax))
            return refuse(NMRFIT_E_INVALID, who + ": a window has 1 .. 2^" + std::to_string(kLgMax) + " values (window " + std::to_string(m) + ")");
        window_at[m + 1] = window_at[m] + (size_t)window_len[m];
    }
    const size_t nk = (size_t)K;
    std::vector<FidCondAsk> asked(nk);
    for (int32_t k = 0; k < K; ++k) {
        const std::string at = " (spectrum " + std::to_string(k) + ")";
        if (T[k] <= 0 || n_in[k] <= 0) return refuse(NMRFIT_E_INVALID, who + ": every spectrum needs T > 0 and n_in > 0" + at);
        FidCondAsk &a = asked[k];
        a = FidCondAsk{n_in[k], n_in[k], n[k], T[k], NMRFIT_FID_FORM_NONE, -1, 0, 0, 0.0};
        if (entry.cond) {
            if (form[k] < NMRFIT_FID_FORM_NONE || form[k] > NMRFIT_FID_FORM_SPECTRUM)
                return refuse(NMRFIT_E_INVALID, who + ": form is 0 (none), 1 (fid) or 2 (spectrum)" + at);
            a.form = form[k];
            a.g = g[k];
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
            if (window_of[k] < -1 || window_of[k] >= M)
                return refuse(NMRFIT_E_INVALID, who + ": window_of is -1 or the index of a window" + at);
            a.window = window_of[k];
            if (a.window >= 0 && window_len[a.window] != a.n_out)
                return refuse(NMRFIT_E_INVALID, who + ": a window has as many values as the conditioned trace has points" + at);
        }
        if (n[k] < a.n_out) return refuse(NMRFIT_E_INVALID, who + ": a transform length is at least " + entry.at_least + at);
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
        const std::string lengths = who + ": a transform length is a power of two, 2 .. 2^" + std::to_string(kLgMax);
        if (entry.any_length && lg < 0) {
            if (n[k] < kFidAnyMin || n[k] > kFidAnyMax)
                return refuse(NMRFIT_E_UNSUPPORTED, lengths + ", or any other length, 3 .. 2^21 - 1" + at);
            if (asked[k].form == NMRFIT_FID_FORM_SPECTRUM)
                return refuse(NMRFIT_E_UNSUPPORTED, who + ": form 2 (spectrum) needs a transform length that is a power of two" + at +
                                                        ": its ramp tables are split at 2^11; use form 1 (fid), or zero fill");
            asks.push_back(FidAnyAsk{n[k], asked[k].n_out, T[k]});
            of_any.push_back((size_t)k);
        } else if (lg < 1 || lg > kLgMax) {
            if (entry.any_length) return refuse(NMRFIT_E_UNSUPPORTED, lengths + ", or any other length, 3 .. 2^21 - 1" + at);
            return refuse(NMRFIT_E_UNSUPPORTED, lengths + at + ": zero fill to the next power of two");
        }
        if (values <= max_values)   // (each term < 2^54: the sum cannot overflow)
            values += (int64_t)T[k] * n[k] + (asked[k].form == NMRFIT_FID_FORM_FID ? (int64_t)T[k] * n_in[k] : 0);
    }
    const bool too_many = K > kWeightsMaxSpectra || values > max_values;
    if (!too_many && !asks.empty()) values += fid_any_values(asks.data(), asks.size());   // (K < 2^16 terms < 2^54)
    if (too_many || values > max_values)
        return refuse(NMRFIT_E_UNSUPPORTED, who + ": a call takes at most " + std::to_string(kWeightsMaxSpectra) + " spectra and " +
                                                std::to_string(max_values) + " transformed values " + entry.budget);
    int rc = use_device(device);
    if (rc != NMRFIT_OK) return rc;
    StreamLease lease(device);
    NMRFIT_HIP(lease.take());
    hipStream_t st = lease.s;

    // ---- the plans: the main transform over all spectra, then the two stages'
    std::vector<FidShape> shapes(nk);
    for (size_t k = 0; k < nk; ++k) shapes[k] = FidShape{asked[k].n_out, n[k], T[k]};
    const FidPlan plan = fid_plan(shapes.data(), nk);
    int64_t raw_values = 0;
    for (size_t k = 0; k < nk; ++k) raw_values += (int64_t)T[k] * n_in[k];
    FidCondStage cond;
    cond.plan(asked, window_at);
    FidAnyStage any;
    any.plan(asks);

    // ---- one allocation for the call's buffers
    Scratch mem;
    Carver c;
    const size_t o_jobs = c.take(nk * sizeof(FidJob)), o_pref = c.take(plan.tab.bytes());
    const size_t o_tw = c.take(kFidStage * sizeof(FidTw)), o_hi = c.take(kFidSplit * sizeof(FidTwDD)),
                 o_lo = c.take(kFidSplit * sizeof(FidTwDD));
    const size_t o_x = c.take((size_t)raw_values * sizeof(double2));
    const size_t o_work = c.take((size_t)plan.work_values * sizeof(double2)), o_z = c.take((size_t)plan.values * sizeof(double2));
    const size_t o_u = c.take((size_t)plan.points * sizeof(double)), o_v = c.take((size_t)plan.points * sizeof(double));
    const size_t o_rows = c.take(nk * kRow * sizeof(double)), o_part = c.take((size_t)plan.tab.items(kFidMaxPart) * sizeof(double4));
    cond.carve(c);
    any.carve(c);
    unsigned char *base = nullptr;
    NMRFIT_HIP(mem.alloc(&base, c.total));
    FidJob *d_jobs = reinterpret_cast<FidJob *>(base + o_jobs);
    long long *d_pref = reinterpret_cast<long long *>(base + o_pref);
    const FidDeviceTables tables{reinterpret_cast<FidTw *>(base + o_tw), reinterpret_cast<FidTwDD *>(base + o_hi),
                                 reinterpret_cast<FidTwDD *>(base + o_lo)};
    double2 *d_x = reinterpret_cast<double2 *>(base + o_x);
    const FidBuffers buf{reinterpret_cast<double2 *>(base + o_work), reinterpret_cast<double2 *>(base + o_z),
                         reinterpret_cast<double *>(base + o_u),     reinterpret_cast<double *>(base + o_v),
                         reinterpret_cast<double *>(base + o_rows),  reinterpret_cast<double4 *>(base + o_part)};

    // ---- uploads (pageable host memory: the copies have left the host arrays when hipMemcpyAsync returns)
    NMRFIT_HIP(cond.upload(base, d_x, buf.z, windows, st));
    const std::vector<FidJob> jobs = fid_job_table(plan, shapes.data(), cond.x_of(), buf);
    NMRFIT_HIP(hipMemcpyAsync(d_jobs, jobs.data(), nk * sizeof(FidJob), hipMemcpyHostToDevice, st));
    NMRFIT_HIP(hipMemcpyAsync(d_pref, plan.tab.pref.data(), plan.tab.bytes(), hipMemcpyHostToDevice, st));
    NMRFIT_HIP(fid_upload_tables(tables, st));
    NMRFIT_HIP(hipMemcpyAsync(d_x, fid, (size_t)raw_values * sizeof(double2), hipMemcpyHostToDevice, st));
    if (!asks.empty()) {
        std::vector<const double2 *> x_any(asks.size());
        std::vector<double2 *> z_any(asks.size());
        for (size_t i = 0; i < asks.size(); ++i) {
            x_any[i] = cond.x_of()[of_any[i]];
            z_any[i] = jobs[of_any[i]].z;
        }
        NMRFIT_HIP(any.upload(base, x_any.data(), z_any.data(), st));
    }

    // ---- the launches: at most 16, at most 26 with spectra on the chirp path
    NMRFIT_HIP(cond.launch_before(tables, st));
    NMRFIT_HIP(fid_launch_transforms(plan, d_jobs, d_pref, tables, st));
    NMRFIT_HIP(any.launch(tables, st));
    NMRFIT_HIP(cond.launch_after(st));
    NMRFIT_HIP(fid_launch_finish(plan, d_jobs, d_pref, st));

    // ---- downloads
    if ((rc = staged_d2h(device, st, rows_out, buf.rows, nk * kRow * sizeof(double))) != NMRFIT_OK) return rc;
    if ((rc = staged_d2h(device, st, u_out, buf.u, (size_t)plan.points * sizeof(double))) != NMRFIT_OK) return rc;
    if ((rc = staged_d2h(device, st, v_out, buf.v, (size_t)plan.points * sizeof(double))) != NMRFIT_OK) return rc;
    if (transform_out && (rc = staged_d2h(device, st, transform_out, buf.z, (size_t)plan.values * sizeof(double2))) != NMRFIT_OK) return rc;
    if (conditioned_out) return cond.download(device, st, fid, conditioned_out);
    return NMRFIT_OK;
}

}  // namespace
}  // namespace nmrfit

using namespace nmrfit;

#pragma GCC visibility push(default)   // the C-ABI: the only symbols the library exports (build.sh: -fvisibility=hidden)

int nmrfit_fid_transform(int device, int32_t K, const int64_t *n_in, const int64_t *n, const int32_t *T, const double *fid,
                         double *u_out, double *v_out, double *rows_out, double *transform_out)
{
    return fid_call(kPlain, device, K, n_in, n, T, fid, nullptr, nullptr, nullptr, 0, nullptr, nullptr, u_out, v_out, rows_out,
                    transform_out, nullptr);
}

int nmrfit_fid_condition_transform(int device, int32_t K, const int64_t *n_in, const int64_t *n, const int32_t *T,
                                   const double *fid, const int32_t *form, const double *g, const int32_t *window_of, int32_t M,
                                   const int64_t *window_len, const double *windows, double *u_out, double *v_out,
                                   double *rows_out, double *transform_out, double *conditioned_out)
{
    return fid_call(kCond, device, K, n_in, n, T, fid, form, g, window_of, M, window_len, windows, u_out, v_out, rows_out,
                    transform_out, conditioned_out);
}

int nmrfit_fid_transform_any(int device, int32_t K, const int64_t *n_in, const int64_t *n, const int32_t *T, const double *fid,
                             const int32_t *form, const double *g, const int32_t *window_of, int32_t M, const int64_t *window_len,
                             const double *windows, double *u_out, double *v_out, double *rows_out, double *transform_out,
                             double *conditioned_out)
{
    return fid_call(kAny, device, K, n_in, n, T, fid, form, g, window_of, M, window_len, windows, u_out, v_out, rows_out,
                    transform_out, conditioned_out);
}

#pragma GCC visibility pop

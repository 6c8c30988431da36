// fid_internal.h -- the host side of the raw-FID call in the pieces its one body (fid_call.hip) composes: the prefix
// tables of a flat launch and the launch itself, the plan of a job table, the job table, the transform and finishing
// launches on a resident job table (fid.hip), and the two stages a call may add to them, each with the four verbs
// plan / carve / upload / launch: the conditioning (fid_cond.hip) and the chirp-z path (fid_any.hip).  The kernels stay
// inside their files.  Host code.
#pragma once
#include "fid_device.h"
#include "fid_twiddle.h"
#include "host_call.h"

#include <vector>

namespace nmrfit {

// The work items of the launches of a stage over K records: `tables` prefix tables of K + 1 numbers, one after the
// other, uploaded as one block.
struct ItemTables {
    size_t K = 0;
    std::vector<long long> pref;
    ItemTables() = default;
    ItemTables(int tables, size_t K_) : K(K_), pref((size_t)tables * (K_ + 1), 0) {}
    long long *row(int i) { return pref.data() + (size_t)i * (K + 1); }
    const long long *row(int i) const { return pref.data() + (size_t)i * (K + 1); }
    void add(int i, size_t k, long long items) { row(i)[k + 1] = row(i)[k] + items; }   // record k's items of table i
    long long items(int i) const { return row(i)[K]; }
    size_t bytes() const { return pref.size() * sizeof(long long); }
    const long long *device(const long long *d_base, int i) const { return d_base + (size_t)i * (K + 1); }
};

// the grid of a flat list of work items (an item is blockIdx.y * gridDim.x + blockIdx.x)
dim3 fid_item_grid(long long items);

// One flat launch: a launch without items is not made.  The HIP error of the launch.
template <typename... Params, typename... Args>
hipError_t launch_items(void (*kernel)(Params...), long long items, int block, size_t lds_bytes, hipStream_t st, Args... args)
{
    if (items == 0) return hipSuccess;
    hipLaunchKernelGGL(kernel, fid_item_grid(items), dim3((unsigned)block), lds_bytes, st, args...);
    return hipGetLastError();
}

// the items of an element-wise stage over T traces of `len` points (fid_device.h, item_place)
inline long long trace_items(int64_t T, int64_t len) { return T * ((len + kFidChunk - 1) / kFidChunk); }

// One spectrum of a call.  Every pointer is device memory.
struct FidJob {
    const double2 *x;    // T traces of n_in points
    double2 *work;       // T traces of n points between the passes (n > 4096)
    double2 *z;          // T traces of n points: Y in the output order
    double *u, *v;       // n points each
    double *row;         // [NMRFIT_FID_ROW]
    double4 *part;       // the partial maxima: (re, im, flat index, not-finite flag)
    int32_t n_in, n, T, lg, lg1, lg2, parts;
};

// what a plan is made from: a spectrum's lengths (n a power of two, 2 .. 2^22, n >= n_in > 0) and trace count.  Any other
// n plans a FINISH-ONLY job (fid_any.hip writes its Z): no transform items, lg = -1.
struct FidShape {
    int64_t n_in, n;
    int32_t T;
};

// The work items of every launch over K spectra (five tables: short, pass 1, pass 2, partial maxima, finish) and what
// the buffers of the job table have to hold.
enum { kFidShort = 0, kFidPass1 = 1, kFidPass2 = 2, kFidMaxPart = 3, kFidFinish = 4, kFidLaunchTables = 5 };
struct FidPlan {
    ItemTables tab;
    int max_short = 0;                                             // the longest LDS-resident transform
    int64_t values = 0, in_values = 0, work_values = 0, points = 0;   // sum T n, sum T n_in, sum T n over n > 4096, sum n
};

int fid_log2_exact(int64_t n);   // -1 unless n is a power of two
FidPlan fid_plan(const FidShape *shapes, size_t K);

// the device buffers a job table is cut from, spectrum after spectrum (u .. part may be null for a table that is only
// transformed: fid_launch_finish is then not called on it)
struct FidBuffers {
    double2 *work, *z;
    double *u, *v, *rows;
    double4 *part;
};
// x_of[k]: where the traces of spectrum k lie
std::vector<FidJob> fid_job_table(const FidPlan &plan, const FidShape *shapes, const double2 *const *x_of, const FidBuffers &buf);

// the twiddle tables of a call in device memory (copies of the process's host tables)
struct FidDeviceTables {
    FidTw *tw;
    FidTwDD *hi, *lo;
};
hipError_t fid_upload_tables(const FidDeviceTables &dst, hipStream_t st);

// Short, pass 1, pass 2 on a resident job table (d_pref: the plan's tables as uploaded); then the three finishing
// launches (partial maxima of every job, maxima, quotient and sum).  The HIP error of the first launch that failed.
hipError_t fid_launch_transforms(const FidPlan &plan, const FidJob *d_jobs, const long long *d_pref, const FidDeviceTables &tables,
                                 hipStream_t st);
hipError_t fid_launch_finish(const FidPlan &plan, const FidJob *d_jobs, const long long *d_pref, hipStream_t st);

// ---- the conditioning stage (fid_cond.hip) ----------------------------------------------------------------------------

// one spectrum of a call as the checks leave it (a plain call: form 0, no window, n_out = n_in everywhere)
struct FidCondAsk {
    int64_t n_in, n_out, n;   // the trace as given, as it enters the main transform, the transform length
    int32_t T, form, window, lg_s, add;
    double g;
    bool conditioned() const { return form == 1 || window >= 0; }   // (1: NMRFIT_FID_FORM_FID)
};

// The conditioning of one call: plan() on the host (window_at: where each window begins in `windows`, and their sum),
// carve() its pieces of the call's one allocation, upload() the tables (d_x: the traces as uploaded, d_z: the main job
// table's Z), launch_before() and launch_after() the main transform: at most eight launches and one.  x_of(): where each
// spectrum's traces enter the main transform.  download(): conditioned_out.  A call with nothing asked takes, uploads
// and launches nothing.
class FidCondStage {
public:
    FidCondStage();
    ~FidCondStage();
    FidCondStage(const FidCondStage &) = delete;
    FidCondStage &operator=(const FidCondStage &) = delete;
    void plan(const std::vector<FidCondAsk> &asks, const std::vector<size_t> &window_at);
    void carve(Carver &c);
    hipError_t upload(unsigned char *base, const double2 *d_x, double2 *d_z, const double *windows, hipStream_t st);
    const double2 *const *x_of() const;
    hipError_t launch_before(const FidDeviceTables &tables, hipStream_t st) const;
    hipError_t launch_after(hipStream_t st) const;
    int download(int device, hipStream_t st, const double *fid, double *conditioned_out) const;

private:
    struct Impl;
    Impl *impl_;
};

// ---- the chirp stage (fid_any.hip) ------------------------------------------------------------------------------------

constexpr int64_t kFidAnyMin = 3, kFidAnyMax = ((int64_t)1 << 21) - 1;   // the lengths the chirp path takes (no power of two)

// a spectrum of the call that takes the chirp path: N is no power of two, n_in <= N points enter the transform
struct FidAnyAsk {
    int64_t N, n_in;
    int32_t T;
};

// M = 2^m, the smallest power of two >= 2 N - 1
int64_t fid_any_conv_length(int64_t N);
// what the chirp path adds to the values of a call: 2 T M per spectrum on it, 2 M per distinct N (nmrfit_amd_fid_any.h, BUDGET)
int64_t fid_any_values(const FidAnyAsk *asks, size_t count);

// The chirp stage of one call: plan() on the host, carve() its pieces of the call's one allocation, upload() the tables
// (x_of[i]: the traces of ask i as they enter the transform, z_of[i]: its T traces of N points of the main job table's Z,
// both device memory), launch() the ten launches.  A stage without asks takes, uploads and launches nothing.
class FidAnyStage {
public:
    FidAnyStage();
    ~FidAnyStage();
    FidAnyStage(const FidAnyStage &) = delete;
    FidAnyStage &operator=(const FidAnyStage &) = delete;
    void plan(const std::vector<FidAnyAsk> &asks);
    void carve(Carver &c);
    hipError_t upload(unsigned char *base, const double2 *const *x_of, double2 *const *z_of, hipStream_t st);
    hipError_t launch(const FidDeviceTables &tables, hipStream_t st) const;

private:
    struct Impl;
    Impl *impl_;
};

}  // namespace nmrfit

// fid_internal.h -- the host side of fid.hip in the pieces another translation unit can compose (fid_cond.hip does): the
// plan of a job table (the work items of every launch as prefix tables over the spectra), the job table itself, the
// transform launches on a resident job table, and the finishing launches.  The kernels stay inside fid.hip.  Host code.
#pragma once
#include "fid_twiddle.h"
#include "host_call.h"

#include <vector>

namespace nmrfit {

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
// n plans a FINISH-ONLY job (fid_any.hip writes its Z): no transform items, lg = -1, and its partial maxima are items of
// fid_any.hip's launch, which does not take n for a power of two.
struct FidShape {
    int64_t n_in, n;
    int32_t T;
};

// The work items of every launch over K spectra: six prefix tables of K + 1 numbers, one after the other (short, pass 1,
// pass 2, partial maxima, finish, partial maxima of the finish-only jobs), and what the buffers of the job table have to
// hold.
struct FidPlan {
    size_t K = 0;
    std::vector<long long> pref;
    int max_short = 0;                                             // the longest LDS-resident transform
    int64_t values = 0, in_values = 0, work_values = 0, points = 0;   // sum T n, sum T n_in, sum T n over n > 4096, sum n
    const long long *table(int which) const { return pref.data() + (size_t)which * (K + 1); }
    long long items(int which) const { return table(which)[K]; }
    long long parts() const;   // the partial maxima of all spectra: what FidBuffers::part holds
};
enum { kFidShort = 0, kFidPass1 = 1, kFidPass2 = 2, kFidMaxPart = 3, kFidFinish = 4, kFidMaxPartAny = 5, kFidLaunchTables = 6 };
inline long long FidPlan::parts() const { return items(kFidMaxPart) + items(kFidMaxPartAny); }

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

// the grid of a flat list of work items (an item is blockIdx.y * gridDim.x + blockIdx.x)
dim3 fid_item_grid(long long items);

// Short, pass 1, pass 2 on a resident job table (d_pref: the plan's tables as uploaded); a launch without items is not
// made.  Then the three finishing launches; the partial maxima of finish-only jobs are there already (fid_any.hip's
// launch on the kFidMaxPartAny table).  The HIP error of the first launch that failed.
hipError_t fid_launch_transforms(const FidPlan &plan, const FidJob *d_jobs, const long long *d_pref, const FidDeviceTables &tables,
                                 hipStream_t st);
hipError_t fid_launch_finish(const FidPlan &plan, const FidJob *d_jobs, const long long *d_pref, hipStream_t st);

}  // namespace nmrfit

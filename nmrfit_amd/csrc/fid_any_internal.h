// fid_any_internal.h -- what fid_cond.hip and fid_any.hip share: the body of the two conditioning entry points (one code
// path, in fid_cond.hip: nmrfit_fid_condition_transform refuses lengths that are not powers of two, nmrfit_fid_transform_any
// sends them through the chirp stage) and the chirp stage of a call as the body composes it (fid_any.hip).  Host code.
#pragma once
#include "fid_internal.h"

#include <string>
#include <vector>

namespace nmrfit {

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
// both device memory), launch() the eleven launches.  A stage without asks takes, uploads and launches nothing.
class FidAnyStage {
public:
    FidAnyStage();
    ~FidAnyStage();
    FidAnyStage(const FidAnyStage &) = delete;
    FidAnyStage &operator=(const FidAnyStage &) = delete;
    void plan(const std::vector<FidAnyAsk> &asks);
    void carve(Carver &c);
    hipError_t upload(unsigned char *base, const double2 *const *x_of, double2 *const *z_of, hipStream_t st);
    // (main_plan, d_main_jobs, d_main_pref: the call's main job table, whose finish-only jobs are this stage's spectra)
    hipError_t launch(const FidDeviceTables &tables, const FidPlan &main_plan, const FidJob *d_main_jobs, const long long *d_main_pref,
                      hipStream_t st) const;

private:
    struct Impl;
    Impl *impl_;
};

// the body of nmrfit_fid_condition_transform (any_length false) and nmrfit_fid_transform_any (true); `who` names the
// entry point in the messages
int fid_condition_transform_run(const std::string &who, bool any_length, int device, int32_t K, const int64_t *n_in, const int64_t *n,
                                const int32_t *T, const double *fid, const int32_t *form, const double *g, const int32_t *window_of,
                                int32_t M, const int64_t *window_len, const double *windows, double *u_out, double *v_out,
                                double *rows_out, double *transform_out, double *conditioned_out);

}  // namespace nmrfit

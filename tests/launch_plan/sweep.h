// sweep.h -- the grid of objective launches that pins the launch plan (csrc/objective_plan.h), what is recorded of every
// case, and how the record is folded: one 64-bit FNV-1a hash over a fixed field list, and a count of cases per outcome
// class.  Two programs walk it and must print the same: plan_sweep.hip next to this file calls the plan directly
// (tests/test_launch_plan_cpu.py), and profiles/r12/launch_objective_record.hip calls launch_objective itself with the
// kernel units, the workspace and the HIP launches replaced by recorders.
#pragma once
#include <cstdint>
#include <cstdio>
#include <map>

namespace sweep {

struct Context {   // the fields of nmrfit_ctx a launch's geometry depends on
    int compute_units;
    int64_t target_waves;
    int variant, fit_im, wide_workgroups, pair_waves;
};

struct Mode {   // what the caller of launch_objective passes besides the shapes
    const char *name;
    bool residual;        // dR
    int rows_fit_im;
    bool defer;           // an ObjectiveDeferred record
    bool fused;           // a PsoFused record ...
    bool fused_rows;      // ... with x_in set
    unsigned pbest, tail, pending;
};
constexpr Mode kModes[] = {
    {"objective", false, 0, false, false, false, 0, 0, 0},
    {"residual", true, 0, false, false, false, 0, 0, 0},
    {"rows_fit_im=1", true, 1, false, false, false, 0, 0, 0},
    {"rows_fit_im=2", true, 2, false, false, false, 0, 0, 0},
    {"fused", false, 0, true, true, true, 0, 0, 0},
    {"fused+pbest", false, 0, true, true, true, 1, 0, 0},
    {"fused+pbest+tail", false, 0, true, true, true, 1, 1, 0},
    {"fused+pbest+tail+pending", false, 0, true, true, true, 1, 1, 1},
    {"fused+pbest+tail+pending, no record", false, 0, false, true, true, 1, 1, 1},
    // beyond the nine above: the remaining ways into an error return, and the deferred sum without a swarm update
    {"objective, deferred", false, 0, true, false, false, 0, 0, 0},
    {"rows_fit_im=1, deferred", true, 1, true, false, false, 0, 0, 0},
    {"rows_fit_im=3", true, 3, false, false, false, 0, 0, 0},
    {"fused residual", true, 0, true, true, true, 1, 1, 0},
    {"fused record without rows, pending", false, 0, true, true, false, 1, 1, 1},
};
constexpr int kCus[] = {256, 64};
constexpr int64_t kTargetWaves[] = {0, 1024};
constexpr int kVariants[] = {0, 1, 6, 7, 8};
constexpr int kFitIm[] = {0, 1, 2};
constexpr int kWide[] = {0, 1};
constexpr int kPairWaves[] = {-1, 0, 1};
constexpr int64_t kN[] = {1, 512, 513, 2048, 4096, 8192, 12000, 16384, 65536, 100000};
constexpr int64_t kS[] = {0, 1, 2, 3, 204, 1023, 1024, 2047, 2048, 4096, 16384};
constexpr int32_t kP[] = {1, 6, 24, 132, 133, 452, 606, 960};

// the kernel unit a launch ran, in the order of objective_launch.h's launch_objective_* functions
constexpr const char *kUnitNames[] = {"none", "default", "farfield", "farfield32", "norec", "rows_im", "pair", "ab"};

struct Outcome {
    int64_t code = 0, unit = -1;   // (unit -1: no kernel unit was called)
    // the ObjectiveLaunch the unit received
    int64_t nseg = 0, seg_len = 0, blk_chunks = 0, seg_blocks = 0, n_blocks = 0, blocks = 0, lds = 0, wpb = 0, pair = 0,
            aux_off = 0, fit_im = 0, xrow_off = 0, pbest = 0, tail = 0;
    int64_t out_is_partial = 0, ensure_size = -1;   // (-1: the partial buffer was not asked for)
    int64_t defer_needed = 0, defer_pbest_done = 0, defer_tail_done = 0, defer_need_flush = 0, defer_n_blocks = 0;
    int64_t last_waves = -1, last_wpb = -1, last_nseg = -1, last_seg_len = -1;   // (-1: ctx->last was left alone)
    int64_t host_launches = 0;   // finalize kernels launched by launch_objective itself
    int64_t message = 0;         // text_hash of what set_error received (0: nothing)
};

inline int64_t text_hash(const char *s)
{
    uint64_t h = 0xcbf29ce484222325ull;
    for (; *s; ++s) h = (h ^ (unsigned char)*s) * 0x100000001b3ull;
    return (int64_t)h;
}

class Record {
  public:
    void add(const Outcome &o)
    {
        const int64_t f[] = {o.code, o.unit, o.nseg, o.seg_len, o.blk_chunks, o.seg_blocks, o.n_blocks, o.blocks, o.lds,
                             o.wpb, o.pair, o.aux_off, o.fit_im, o.xrow_off, o.pbest, o.tail, o.out_is_partial,
                             o.ensure_size, o.defer_needed, o.defer_pbest_done, o.defer_tail_done, o.defer_need_flush,
                             o.defer_n_blocks, o.last_waves, o.last_wpb, o.last_nseg, o.last_seg_len, o.host_launches, o.message};
        for (int64_t v : f)
            for (int b = 0; b < 8; ++b) {
                hash_ ^= (uint64_t)(v >> (8 * b)) & 0xffu;
                hash_ *= 0x100000001b3ull;
            }
        // the outcome class, packed: formatted when printed
        const int64_t seg = o.nseg == 0 ? 0 : o.nseg == 1 ? 1 : o.nseg == 4 ? 2 : o.nseg == 8 ? 3 : 4;
        ++classes_[((((((-o.code * 8 + (o.unit + 1)) * 8 + seg) * 16 + o.wpb) * 2 + o.pair) * 2 + (o.pbest != 0)) * 2 + (o.tail != 0)) * 2 +
                   o.defer_need_flush];
        ++cases_;
    }
    void print(const char *build, int seg_rule) const
    {
        printf("build=%s seg_rule=%d cases=%lld hash=%016llx classes=%zu\n", build, seg_rule, (long long)cases_,
               (unsigned long long)hash_, classes_.size());
        static const char *const kSeg[] = {"-", "1", "4", "8", "other"};
        for (const auto &c : classes_) {
            const int64_t k = c.first;
            printf("  code=%-2d unit=%-10s nseg=%-5s wpb=%d pair=%d pbest=%d tail=%d flush=%d  %lld\n", -(int)(k >> 14),
                   kUnitNames[(k >> 11) & 7], kSeg[(k >> 8) & 7], (int)((k >> 4) & 15), (int)((k >> 3) & 1), (int)((k >> 2) & 1),
                   (int)((k >> 1) & 1), (int)(k & 1), (long long)c.second);
        }
    }

  private:
    uint64_t hash_ = 0xcbf29ce484222325ull;
    long long cases_ = 0;
    std::map<int64_t, long long> classes_;
};

// run(context, mode, N, S, P) -> Outcome, for every case of the grid in one fixed order
template <class Run>
void walk(Record &rec, Run &&run)
{
    for (int cus : kCus)
        for (int64_t tw : kTargetWaves)
            for (int variant : kVariants)
                for (int fit_im : kFitIm)
                    for (int wide : kWide)
                        for (int pw : kPairWaves) {
                            const Context c{cus, tw, variant, fit_im, wide, pw};
                            for (const Mode &m : kModes)
                                for (int64_t N : kN)
                                    for (int64_t S : kS)
                                        for (int32_t P : kP) rec.add(run(c, m, N, S, P));
                        }
}

}  // namespace sweep

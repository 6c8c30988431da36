// plan_sweep.hip -- walks plan_objective (csrc/objective_plan.h) over the grid of sweep.h, on the CPU: no HIP call, no
// GPU.  Prints the record of what launch_objective makes of every plan -- for the product library and for the A/B
// library, which differ only in what becomes of the A/B unit -- in the format of profiles/r12/launch_objective_record.hip,
// and checks the invariants of every planned launch.  tests/test_launch_plan_cpu.py compiles and runs it.
//   plan_sweep <seg_rule: 4 | 3>
#include "objective_plan.h"
#include "sweep.h"

#include <cstdlib>
#include <cstring>

using namespace nmrfit;

namespace {

ObjectivePlanInput plan_input(const sweep::Context &c, const sweep::Mode &m, int64_t N, int64_t S, int32_t P, int seg_rule)
{
    ObjectivePlanInput in{};
    in.S = S;
    in.P = P;
    in.N = N;
    in.compute_units = c.compute_units;
    in.target_waves = c.target_waves;
    in.variant = c.variant;
    in.fit_im = c.fit_im;
    in.wide_workgroups = c.wide_workgroups != 0;
    in.pair_waves = c.pair_waves;
    in.residual = m.residual;
    in.rows_fit_im = m.rows_fit_im;
    in.defer = m.defer;
    in.fused = m.fused;
    in.fused_rows = m.fused_rows;
    in.pbest = m.fused && m.pbest != 0u;
    in.tail = m.fused && m.tail != 0u;
    in.pending = m.fused && m.pending != 0u;
    in.seg_rule = seg_rule;
    return in;
}

// what launch_objective does with a plan, as the recording harness sees it (`ab`: in the A/B library)
sweep::Outcome carry_out(const ObjectivePlan &p, const sweep::Mode &m, bool ab)
{
    sweep::Outcome o;
    if (p.code != NMRFIT_OK) {
        o.code = p.code;
        o.message = sweep::text_hash(p.message);
        return o;
    }
    o.defer_need_flush = p.need_flush;
    if (p.unit == kUnitNone) return o;
    if (!p.direct_f) o.ensure_size = p.partial_doubles;
    if (p.unit == kUnitAB && !ab) {
        o.code = NMRFIT_E_UNSUPPORTED;
        o.message = sweep::text_hash("this kernel variant exists in A/B builds of the library only (-DNMRFIT_AB_BUILD)");
        return o;
    }
    o.unit = p.unit;
    o.nseg = p.nseg;
    o.seg_len = p.seg_len;
    o.blk_chunks = p.blk_chunks;
    o.seg_blocks = p.seg_blocks;
    o.n_blocks = p.n_blocks;
    o.blocks = p.blocks;
    o.lds = (int64_t)p.lds;
    o.wpb = p.wpb;
    o.pair = p.pair;
    o.aux_off = p.aux_off;
    o.fit_im = p.fit_im;
    o.xrow_off = p.xrow_off;
    o.pbest = p.pbest ? m.pbest : 0;
    o.tail = p.tail ? m.tail : 0;
    o.out_is_partial = !p.direct_f;
    if (m.defer) {
        o.defer_needed = !p.direct_f;
        o.defer_n_blocks = p.direct_f ? 0 : p.n_blocks;
        o.defer_pbest_done = p.pbest;
        o.defer_tail_done = p.tail;
    } else if (!p.direct_f) {
        o.host_launches = 1;
    }
    o.last_waves = p.waves;
    o.last_wpb = p.wpb;
    o.last_nseg = p.nseg;
    o.last_seg_len = p.seg_len;
    return o;
}

long long g_violations = 0;
void violation(const char *what, const ObjectivePlanInput &in, const sweep::Mode &m)
{
    if (++g_violations <= 20)
        printf("VIOLATION %s: mode '%s' S=%lld N=%lld P=%d cus=%d target_waves=%lld variant=%d fit_im=%d wide=%d pair_waves=%d seg_rule=%d\n",
               what, m.name, (long long)in.S, (long long)in.N, (int)in.P, in.compute_units, (long long)in.target_waves, in.variant,
               in.fit_im, (int)in.wide_workgroups, in.pair_waves, in.seg_rule);
}
#define HOLDS(cond) \
    do { \
        if (!(cond)) violation(#cond, in, m); \
    } while (0)

// what holds of every planned launch
void check_launch(const ObjectivePlanInput &in, const sweep::Mode &m, const ObjectivePlan &p)
{
    const int64_t S = in.S, N = in.N;
    const BlockPlan bp = block_plan(N);
    const int64_t row_bytes = (4 + 3 * (int64_t)in.P) * (int64_t)sizeof(double);
    HOLDS(p.lds + (p.pair ? kPairStaticLds : kObjectiveStaticLds) + 16 <= 160 * 1024);
    HOLDS(p.blocks >= 1);
    HOLDS(p.nseg * p.seg_len >= N && N > (p.nseg - 1) * p.seg_len);
    HOLDS(p.seg_len % bp.blk_len == 0 && p.seg_blocks == p.seg_len / bp.blk_len);
    HOLDS(p.n_blocks == bp.n_blocks && p.blk_chunks == bp.blk_chunks);
    HOLDS(p.wpb == 4 || p.wpb == 8);
    HOLDS(p.wpb != 8 || (p.nseg == 8 && !in.residual && p.fit_im == 0 && in.wide_workgroups));
    HOLDS((p.unit == kUnitPair) == p.pair);
    HOLDS(!p.pair || (p.variant == NMRFIT_VARIANT_DEFAULT && p.nseg == 4 && p.wpb == 4 && p.fit_im == 0 && !in.residual &&
                      p.blocks == (S + 1) / 2 && in.pair_waves != 0));
    HOLDS(p.pair || p.blocks == (S * p.nseg + p.wpb - 1) / p.wpb);
    HOLDS(!p.pbest || (in.fused_rows && p.nseg == p.wpb));
    HOLDS(!p.tail || (p.pbest && S <= (int64_t)kDeferredPerLane * 64 * p.wpb));
    HOLDS(!in.fused_rows || (p.xrow_off % 16 == 0 && ((int64_t)p.lds - (int64_t)p.xrow_off) % row_bytes == 0 &&
                             (int64_t)p.lds - (int64_t)p.xrow_off == p.rows * row_bytes));
    // the row copies the kernels count on without being told: swarm_prologue / personal_best of a workgroup that is one
    // particle, and objective_pair_body (B's rows start `rows per particle` rows behind A's), derive them from the tail flag
    HOLDS(!(in.fused_rows && !p.pair && p.nseg == p.wpb) || p.rows == (p.tail ? 3 : 1));
    HOLDS(!(in.fused_rows && p.pair) || p.rows == 2 * (p.tail ? 3 : 1));
    HOLDS(p.unit != kUnitFarfield32 || (!in.residual && p.fit_im == 0));
    HOLDS((p.partial_doubles != 0) == (p.nseg != 1 && p.nseg != p.wpb) && p.direct_f == (p.partial_doubles == 0));
    HOLDS(!in.pending || p.tail);
}

}  // namespace

int main(int argc, char **argv)
{
    const int seg_rule = argc > 1 && strcmp(argv[1], "3") == 0 ? 3 : 4;
    sweep::Record product, ab;
    long long launches = 0;
    sweep::walk(product, [&](const sweep::Context &c, const sweep::Mode &m, int64_t N, int64_t S, int32_t P) {
        const ObjectivePlanInput in = plan_input(c, m, N, S, P, seg_rule);
        const ObjectivePlan p = plan_objective(in);
        if (p.code == NMRFIT_OK && p.unit != kUnitNone) {
            ++launches;
            check_launch(in, m, p);
        }
        ab.add(carry_out(p, m, true));
        return carry_out(p, m, false);
    });
    product.print("product", seg_rule);
    ab.print("ab", seg_rule);
    printf("planned launches checked=%lld violations=%lld\n", launches, g_violations);
    return g_violations ? 1 : 0;
}

// launch_objective_record.hip -- records what launch_objective (csrc/objective.hip) decides for every case of the grid
// in tests/launch_plan/sweep.h, without a GPU: objective.hip is compiled into this program with the kernel units
// (launch_objective_*), the workspace (ensure), the error sink and the HIP launches replaced by recorders.  It depends on
// launch_objective's signature alone, so the same file records the commit before the launch plan moved into
// objective_plan.h and the commit after; the two outputs in this directory are identical.
//
//   hipcc --offload-arch=gfx950 --cuda-host-only -O2 -std=c++17 -Iinclude -I<commit>/nmrfit_amd/csrc -Itests/launch_plan \
//         profiles/r12/launch_objective_record.hip -o record        (the A/B library's side: add -DNMRFIT_AB_BUILD)
//   ./record; NMRFIT_SEG_RULE=3 ./record
#include "objective_launch.h"
#include "objective_lds.h"
#include "objective_math.h"
#include "sweep.h"

#include <cstdlib>

namespace {
sweep::Outcome g_out;
double g_partial[1];
}  // namespace

// no kernel is launched: the finalize launches of launch_objective are counted instead
#undef hipLaunchKernelGGL
#define hipLaunchKernelGGL(...) ((void)++g_out.host_launches)
#define hipGetLastError() hipSuccess

#include "objective.hip"

namespace nmrfit {

void set_error(const std::string &msg) { g_out.message = sweep::text_hash(msg.c_str()); }
int hip_fail(hipError_t, const char *, const char *, int) { return NMRFIT_E_HIP; }
int ensure(nmrfit_ctx *, double **buf, int64_t *, int64_t need)
{
    g_out.ensure_size = need;
    *buf = g_partial;
    return NMRFIT_OK;
}

static int record_unit(int unit, const ObjectiveLaunch &a)
{
    g_out.unit = unit;
    g_out.nseg = a.nseg;
    g_out.seg_len = a.seg_len;
    g_out.blk_chunks = a.blk_chunks;
    g_out.seg_blocks = a.seg_blocks;
    g_out.n_blocks = a.n_blocks;
    g_out.blocks = a.blocks;
    g_out.lds = (int64_t)a.lds;
    g_out.wpb = a.wpb;
    g_out.pair = a.pair;
    g_out.aux_off = a.aux_off;
    g_out.fit_im = a.fit_im;
    g_out.xrow_off = a.upd.xrow_off;
    g_out.pbest = a.upd.pbest;
    g_out.tail = a.upd.tail;
    g_out.out_is_partial = a.out == g_partial;
    return NMRFIT_OK;
}
int launch_objective_default(const ObjectiveLaunch &a) { return record_unit(0, a); }
int launch_objective_farfield(const ObjectiveLaunch &a) { return record_unit(1, a); }
int launch_objective_farfield32(const ObjectiveLaunch &a) { return record_unit(2, a); }
int launch_objective_norec(const ObjectiveLaunch &a) { return record_unit(3, a); }
int launch_objective_rows_im(const ObjectiveLaunch &a) { return record_unit(4, a); }
int launch_objective_pair(const ObjectiveLaunch &a) { return record_unit(5, a); }
#ifdef NMRFIT_AB_BUILD
int launch_objective_ab(int, const ObjectiveLaunch &a) { return record_unit(6, a); }
#endif

}  // namespace nmrfit

int main()
{
    const char *e = getenv("NMRFIT_SEG_RULE");
    nmrfit_ctx ctx;
    double x[1], f[1], r[1];
    sweep::Record rec;
    sweep::walk(rec, [&](const sweep::Context &c, const sweep::Mode &m, int64_t N, int64_t S, int32_t P) {
        g_out = sweep::Outcome{};
        ctx.compute_units = c.compute_units;
        ctx.target_waves = c.target_waves;
        ctx.variant = c.variant;
        ctx.fit_im = c.fit_im;
        ctx.wide_workgroups = c.wide_workgroups != 0;
        ctx.pair_waves = c.pair_waves;
        ctx.N = N;
        ctx.d_partial = nullptr;
        ctx.last = nmrfit::LaunchGeom{-1, -1, -1, -1};
        nmrfit::PsoFused fused{};
        if (m.fused_rows) fused.x_in = x;
        fused.pbest = m.pbest;
        fused.tail = m.tail;
        fused.pending = m.pending;
        nmrfit::ObjectiveDeferred defer{};
        g_out.code = nmrfit::launch_objective(&ctx, S, P, x, f, m.residual ? r : nullptr, m.defer ? &defer : nullptr,
                                              m.fused ? &fused : nullptr, m.rows_fit_im);
        g_out.defer_needed = defer.needed;
        g_out.defer_pbest_done = defer.pbest_done;
        g_out.defer_tail_done = defer.tail_done;
        g_out.defer_need_flush = defer.need_flush;
        g_out.defer_n_blocks = defer.n_blocks;
        g_out.last_waves = ctx.last.waves;
        g_out.last_wpb = ctx.last.waves_per_workgroup;
        g_out.last_nseg = ctx.last.nseg;
        g_out.last_seg_len = ctx.last.seg_len;
        return g_out;
    });
#ifdef NMRFIT_AB_BUILD
    rec.print("ab", e && atoi(e) == 3 ? 3 : 4);
#else
    rec.print("product", e && atoi(e) == 3 ? 3 : 4);
#endif
    return 0;
}

// objective.hip -- host side of the hot path: the launch itself (launch_objective), which carries out the plan that
// objective_plan.h makes of it (segments per particle, waves per workgroup, the LDS budget that picks the kernel form:
// every rule lives there); plus the small kernels around it (block-sum finalisation, grid preparation; the post-fit
// reconstruction is result.hip).  The objective kernel is objective_kernel.h; its instantiations live in objective_{default,farfield,norec}.hip, the DEFAULT kernel's pair form
// (two particles per workgroup) in objective_pair.h / objective_pair.hip.
#include "objective_launch.h"
#include "objective_lds.h"
#include "objective_math.h"
#include "objective_plan.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>

namespace nmrfit {
namespace {

// f[i] = sqrt( (sum of the particle's per-block sums, in grid order) / N ); with the imaginary
// part: the mean of the real and imaginary RMSE (two sums per block)
__global__ void finalize_kernel(const double *__restrict__ partial, int64_t S, int64_t n_chunks, int64_t N,
                                int fit_im, double *__restrict__ f)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= S) return;
    f[i] = finalize_value(partial + i * n_chunks * (fit_im ? 2 : 1), n_chunks, N, fit_im);
}

// residual rows of both channels (launch_objective, rows_fit_im): the two RMSEs of every row from the same per-block
// sums in the same order -- 0.5 * (f2[2 i] + f2[2 i + 1]) is what finalize_kernel gives
__global__ void finalize_rows_im_kernel(const double *__restrict__ partial, int64_t S, int64_t n_blocks, int64_t N,
                                        double *__restrict__ f2)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= S) return;
    const double *p = partial + i * n_blocks * 2;
    double ss = 0.0, si = 0.0;
    for (int64_t c = 0; c < n_blocks; ++c) {
        ss += p[2 * c];
        si += p[2 * c + 1];
    }
    f2[2 * i] = sqrt(ss / (double)N);
    f2[2 * i + 1] = sqrt(si / (double)N);
}

// per-chunk (min, max) of the centred grid: one wave per chunk
__global__ void chunk_minmax_kernel(const double *__restrict__ wc, int64_t N, int64_t n_chunks,
                                    double2 *__restrict__ out)
{
    const int64_t c = (int64_t)blockIdx.x * (blockDim.x / kWave) + (threadIdx.x >> 6);
    if (c < n_chunks) chunk_minmax_wave(wc, N, c, threadIdx.x & (kWave - 1), out);
}

__global__ void centre_kernel(const double *__restrict__ w, int64_t N, double w0, double *__restrict__ wc)
{
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j < N) wc[grid_slot(j)] = w[j] - w0;
}

__global__ void scatter_grid_kernel(const double *__restrict__ src, int64_t N, double *__restrict__ dst)
{
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j < N) dst[grid_slot(j)] = src[j];
}

}  // namespace

// Builds the derived device arrays of a context (centred grid, chunk table).
int prepare_grid(nmrfit_ctx *ctx, const double *d_w_raw)
{
    const int64_t N = ctx->N;
    hipLaunchKernelGGL(centre_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, ctx->stream, d_w_raw, N,
                       ctx->w0, ctx->d_wc);
    NMRFIT_HIP(hipGetLastError());
    const int waves_per_block = 4;
    hipLaunchKernelGGL(chunk_minmax_kernel, dim3((unsigned)((ctx->n_chunks + waves_per_block - 1) / waves_per_block)),
                       dim3(kWave * waves_per_block), 0, ctx->stream, ctx->d_wc, N, ctx->n_chunks, ctx->d_chunk);
    NMRFIT_HIP(hipGetLastError());
    return NMRFIT_OK;
}

int scatter_grid(nmrfit_ctx *ctx, const double *d_src, double *d_dst)
{
    const int64_t N = ctx->N;
    hipLaunchKernelGGL(scatter_grid_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, ctx->stream, d_src, N, d_dst);
    NMRFIT_HIP(hipGetLastError());
    return NMRFIT_OK;
}

// objective_launch.h's view of resolve_lds (objective_plan.h), for the units that size launches of their own (batch.hip, lsq.hip)
size_t objective_lds(int variant, int32_t P, bool residual, int fit_im, int *variant_out, unsigned *aux_off, int wpb,
                     int slices, int rows)
{
    const ResolvedLds r = resolve_lds(variant, P, residual, fit_im, wpb, slices, rows);
    *variant_out = r.variant;
    *aux_off = r.aux_off;
    return r.lds;
}

// Every decision is plan_objective's (objective_plan.h); here the plan is carried out.
int launch_objective(nmrfit_ctx *ctx, int64_t S, int32_t P, const double *dX, double *df, double *dR,
                     ObjectiveDeferred *defer, const PsoFused *fused, int rows_fit_im)
{
    if (defer) *defer = ObjectiveDeferred{};
    static const int seg_rule = [] {
        const char *e = getenv("NMRFIT_SEG_RULE");   // A/B knob: 3 = the round-3 rule (~16 tasks per SIMD)
        return e && atoi(e) == 3 ? 3 : 4;
    }();
    ObjectivePlanInput in{};
    in.S = S;
    in.P = P;
    in.N = ctx->N;
    in.compute_units = ctx->compute_units;
    in.target_waves = ctx->target_waves;
    in.variant = ctx->variant;
    in.fit_im = ctx->fit_im;
    in.wide_workgroups = ctx->wide_workgroups;
    in.pair_waves = ctx->pair_waves;
    in.residual = dR != nullptr;
    in.rows_fit_im = rows_fit_im;
    in.defer = defer != nullptr;
    in.fused = fused != nullptr;
    in.fused_rows = fused && fused->x_in;
    in.pbest = fused && fused->pbest != 0u;
    in.tail = fused && fused->tail != 0u;
    in.pending = fused && fused->pending != 0u;
    in.seg_rule = seg_rule;
    const ObjectivePlan plan = plan_objective(in);
    if (plan.code != NMRFIT_OK) {
        set_error(plan.message);
        return plan.code;
    }
    if (plan.need_flush) {   // nothing is launched: the caller folds in a launch of its own and comes back
        defer->need_flush = true;
        return NMRFIT_OK;
    }
    if (plan.unit == kUnitNone) return NMRFIT_OK;   // no particles

    ObjectiveLaunch la{};
    static_cast<ObjectiveGeometry &>(la) = plan;
    la.ctx = ctx;
    la.S = S;
    la.P = P;
    la.dX = dX;
    la.out = df;
    la.dR = dR;
    if (!plan.direct_f) {
        int rc = ensure(ctx, &ctx->d_partial, &ctx->cap_partial, plan.partial_doubles);
        if (rc != NMRFIT_OK) return rc;
        la.out = ctx->d_partial;
    }
    if (in.fused_rows) {
        la.upd = *fused;
        la.upd.xrow_off = plan.xrow_off;
        if (!plan.pbest) la.upd.pbest = 0u;
        if (!plan.tail) la.upd.tail = 0u;
    }
    int rc = NMRFIT_OK;
    switch (plan.unit) {
        case kUnitDefault: rc = launch_objective_default(la); break;
        case kUnitPair: rc = launch_objective_pair(la); break;
        case kUnitFarfield: rc = launch_objective_farfield(la); break;
        case kUnitFarfield32: rc = launch_objective_farfield32(la); break;
        case kUnitNorec: rc = launch_objective_norec(la); break;
        case kUnitRowsIm: rc = launch_objective_rows_im(la); break;
        default:
#ifdef NMRFIT_AB_BUILD
            rc = launch_objective_ab(plan.variant, la);
#else
            set_error("this kernel variant exists in A/B builds of the library only (-DNMRFIT_AB_BUILD)");
            rc = NMRFIT_E_UNSUPPORTED;
#endif
            break;
    }
    if (rc != NMRFIT_OK) return rc;
    // per-block sums: the caller's own kernel adds them (pso_tail_kernel), or one of the finalize kernels here
    if (!plan.direct_f && defer) {
        defer->needed = true;
        defer->partial = ctx->d_partial;
        defer->n_blocks = plan.n_blocks;
        defer->fit_im = plan.fit_im;
    } else if (!plan.direct_f) {
        const dim3 grid((unsigned)((S + 255) / 256)), block(256);
        if (plan.unit == kUnitRowsIm)
            hipLaunchKernelGGL(finalize_rows_im_kernel, grid, block, 0, ctx->stream, ctx->d_partial, S, (int64_t)plan.n_blocks, in.N, df);
        else
            hipLaunchKernelGGL(finalize_kernel, grid, block, 0, ctx->stream, ctx->d_partial, S, (int64_t)plan.n_blocks, in.N, plan.fit_im, df);
        NMRFIT_HIP(hipGetLastError());
    }
    if (defer) {
        defer->pbest_done = plan.pbest;
        defer->tail_done = plan.tail;
    }
    ctx->last.waves = plan.waves;
    ctx->last.waves_per_workgroup = plan.wpb;
    ctx->last.nseg = (int32_t)plan.nseg;
    ctx->last.seg_len = plan.seg_len;
    return NMRFIT_OK;
}

}  // namespace nmrfit

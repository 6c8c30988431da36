// objective_pair.hip -- the pair form of the DEFAULT objective kernel (objective_pair.h: two particles per workgroup, a wave
// holds a segment of both and fetches every chunk of the grid once for the two).  A translation unit of its own: it
// compiles next to the others, and objective_default.hip stays what it was.
#include "objective_pair.h"

namespace nmrfit {

int launch_objective_pair(const ObjectiveLaunch &a)
{
    nmrfit_ctx *const ctx = a.ctx;
    if (a.dR || a.fit_im != 0 || a.nseg != kWavesPerBlock || a.wpb != kWavesPerBlock || !a.pair) {
        set_error("internal: the pair form takes objective launches of the real channel with four segments per particle");
        return NMRFIT_E_STATE;
    }
    // nmrfit_prof_enable: HIP events on the launch stream around this kernel alone (launch_variant)
    const bool prof = ctx->prof_cap > 0 && ctx->prof_nk < ctx->prof_cap;
    unsigned long long *clk = prof ? ctx->d_clk : nullptr;
    if (prof) NMRFIT_HIP(hipEventRecord(ctx->prof_k0[(size_t)ctx->prof_nk], ctx->stream));
    hipLaunchKernelGGL((objective_kernel_pair<kWavesPerBlock>), dim3((unsigned)a.blocks), dim3(kWave * kWavesPerBlock), a.lds,
                       ctx->stream, ctx->d_wc, ctx->d_u, ctx->d_v, ctx->d_wt, ctx->d_chunk, a.dX, a.S, (int)a.P, ctx->N, ctx->w0,
                       ctx->wspan, a.seg_len, a.blk_chunks, a.seg_blocks, a.n_blocks, ctx->lane_step, ctx->grid_dev * 11.0e10,
                       a.out, clk, a.upd);
    NMRFIT_HIP(hipGetLastError());
    if (prof) {
        NMRFIT_HIP(hipEventRecord(ctx->prof_k1[(size_t)ctx->prof_nk], ctx->stream));
        ++ctx->prof_nk;
    }
    return NMRFIT_OK;
}

}  // namespace nmrfit

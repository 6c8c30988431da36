// objective_rows_im.hip -- the instantiations of objective_kernel that write residual rows of BOTH channels
// (include/nmrfit_amd_lsq_im.h): <DEFAULT, residual rows, fit_im = 1> and <DEFAULT, residual rows, fit_im = 2>.  A
// translation unit of its own: they compile next to the others, and objective_default.hip stays what it was.
#include "objective_kernel.h"

namespace nmrfit {
namespace {

template <int FIT_IM>
int launch_rows_im(const ObjectiveLaunch &a)
{
    nmrfit_ctx *const ctx = a.ctx;
    hipLaunchKernelGGL((objective_kernel<NMRFIT_VARIANT_DEFAULT, true, FIT_IM, kWavesPerBlock>), dim3((unsigned)a.blocks),
                       dim3(kWave * kWavesPerBlock), a.lds, ctx->stream, ctx->d_wc, ctx->d_u, ctx->d_v, ctx->d_wt, ctx->d_chunk,
                       a.dX, a.S, (int)a.P, ctx->N, ctx->w0, ctx->wspan, a.nseg, a.seg_len, a.blk_chunks, a.seg_blocks,
                       a.n_blocks, ctx->lane_step, ctx->grid_dev * 11.0e10, a.out, a.dR, (unsigned long long *)nullptr, a.upd,
                       a.aux_off);
    NMRFIT_HIP(hipGetLastError());
    return NMRFIT_OK;
}

}  // namespace

int launch_objective_rows_im(const ObjectiveLaunch &a)
{
    if (!a.dR || a.wpb != kWavesPerBlock || (a.fit_im != 1 && a.fit_im != 2)) {
        set_error("internal: launch_objective_rows_im without rows, or with a mode that is not 1 or 2");
        return NMRFIT_E_STATE;
    }
    return a.fit_im == 1 ? launch_rows_im<1>(a) : launch_rows_im<2>(a);
}

}  // namespace nmrfit

// objective_launch.h -- what objective.hip (host side: the launch, planned by objective_plan.h) hands to the translation units
// that hold the kernel instantiations, one per selectable variant so that they compile in parallel.
#pragma once
#include "nmrfit_internal.h"
#include "pso_update.h"

namespace nmrfit {

// The geometry of one objective launch: decided by plan_objective (objective_plan.h), read by the kernel units.
struct ObjectiveGeometry {
    int nseg = 0;
    int64_t seg_len = 0;
    int blk_chunks = 0;
    int seg_blocks = 0;    // blocks per segment (seg_len / block length)
    int n_blocks = 0;      // blocks per grid
    int64_t blocks = 0;    // workgroups
    size_t lds = 0;        // dynamic LDS per workgroup
    int fit_im = 0;
    unsigned aux_off = 0;
    int wpb = 0;           // waves per workgroup (4, or 8: has_eight_wave_form)
    bool pair = false;     // the pair form: a workgroup is two particles (objective_pair.h); `blocks` counts pairs
};
struct ObjectiveLaunch : ObjectiveGeometry {
    nmrfit_ctx *ctx;
    int64_t S;
    int32_t P;
    const double *dX;
    double *out;           // f[S], or per-block sums when a particle is spread over several workgroups
    double *dR;            // residual rows (else null)
    PsoFused upd;
};

// Which instantiations exist with eight-wave workgroups (one workgroup = one particle cut into eight segments):
// the objective launches without the imaginary channel of the three kernels fit() can select.
constexpr bool is_farfield(int variant) { return variant == NMRFIT_VARIANT_FARFIELD || variant == NMRFIT_VARIANT_FARFIELD32; }
constexpr bool has_eight_wave_form(int variant)
{
    return variant == NMRFIT_VARIANT_DEFAULT || is_farfield(variant) || variant == NMRFIT_VARIANT_NOREC;
}
constexpr int kWideWaves = 8;
// objective_kernel's own __shared__ block (wsums: 2 x kMaxBlocks block sums + 8 parked values) + alignment slack
constexpr size_t kObjectiveStaticLds = (size_t)(2 * kMaxBlocks + 8) * sizeof(double) + 64;
// The LDS of a CU, and whether a workgroup's share fits in it: its dynamic LDS, its kernel's static LDS, 16 bytes of
// slack, and (swarm generations) the row copies not yet counted in `dynamic`.
constexpr size_t kCuLdsBytes = 160 * 1024;
constexpr bool lds_fits(size_t dynamic, size_t static_lds, size_t rows_bytes = 0)
{
    return dynamic + static_lds + 16 + rows_bytes <= kCuLdsBytes;
}

// The kernel variant a launch actually runs (the requested one may not fit in LDS, or may not implement the imaginary
// part) and the dynamic LDS its records need (objective_plan.h: resolve_lds).  `slices`: copies of the per-peak records in a workgroup
// (1 when its waves are segments of one particle, else wpb); `rows`: row copies kept for a fused swarm generation.
size_t objective_lds(int variant, int32_t P, bool residual, int fit_im, int *variant_out, unsigned *aux_off, int wpb,
                     int slices, int rows);

int launch_objective_default(const ObjectiveLaunch &a);    // objective_default.hip
int launch_objective_farfield(const ObjectiveLaunch &a);   // objective_farfield.hip
int launch_objective_norec(const ObjectiveLaunch &a);      // objective_norec.hip
int launch_objective_farfield32(const ObjectiveLaunch &a); // objective_farfield32.hip (objective launches, fit_im = 0)
int launch_objective_rows_im(const ObjectiveLaunch &a);   // objective_rows_im.hip (DEFAULT, residual rows of both channels)
int launch_objective_pair(const ObjectiveLaunch &a);      // objective_pair.hip (DEFAULT, objective launches, two particles per workgroup)
#ifdef NMRFIT_AB_BUILD
int launch_objective_ab(int variant, const ObjectiveLaunch &a);   // objective_ab.hip: BASELINE, NOSKIP
#endif

}  // namespace nmrfit

// objective_finish.h -- how objective_body (objective_kernel.h) ends: f of a particle whose one wave holds all of it, and
// the fused personal-best step of a swarm generation.  (The ending of a workgroup that is one particle stays in
// objective_body itself: moved into a function it changed the kernels' instruction streams.)  A particle spread over
// several workgroups ends in the chunk's block-end stores instead (objective_chunk_stages.h) and is added up by
// finalize_kernel or the swarm's select kernel.
#pragma once
#include "objective_math.h"

namespace nmrfit {
namespace {

// Personal best of this particle, when this wave / workgroup holds all of it and the swarm asked for it
// (fused generations only: the updated row sits in LDS): pyswarm's `i_update = fx < fp; p[i_update] =
// x[i_update]; fp[i_update] = fx[i_update]`.  Particle-local: nobody else reads or writes this row in this launch.
// (A struct of references with a call operator: see objective_prologue.h.)
template <bool WRITE_R>
struct PersonalBest {
    double *&wsums;
    const int &P;
    const int64_t &pblock;
    unsigned char *&lds_raw;
    unsigned long long *__restrict__ &clk;
    __device__ void operator()(const double f) const
    {
        if constexpr (!WRITE_R) {
            if (wsums[2 * kMaxBlocks + 1] != 0.0) {
                // What this needs -- p, S, the row's place in LDS -- was parked in LDS by the prologue (wsums[..+2..4])
                // and is read back here: kept in scalar registers across the chunk loop those few values tipped the
                // headline kernel, which has neither a scalar nor a vector register to spare, into scratch memory.
                // fp[S] sits right behind p[S x D] (PsoFused).
                const int64_t D2 = 4 + 3 * (int64_t)P;
                // (as many segments as waves per workgroup: workgroup = particle -- no need for the prologue's 64-bit division result)
                const int64_t part = pblock;
                double *pb = reinterpret_cast<double *>((uintptr_t)__double_as_longlong(wsums[2 * kMaxBlocks + 2]));
                double *fpb = pb + __double_as_longlong(wsums[2 * kMaxBlocks + 3]) * D2;
                const double *row = reinterpret_cast<const double *>(lds_raw + (unsigned)__double_as_longlong(wsums[2 * kMaxBlocks + 4]));
                const int ln = threadIdx.x & (kWave - 1);
                const double fp_old = wsums[2 * kMaxBlocks + 5];   // (requested by the kernel's first instructions)
                const long long pflip = __double_as_longlong(wsums[2 * kMaxBlocks + 7]);   // (0: no deferred fold)
                if (pflip != 0) {
                    // deferred form: the other (p, fp) buffer gets this particle's row and value whether it improved
                    // or not (PsoFused::pflip; the old row was parked in row 2 of the LDS area by the prologue)
                    const bool better = f < fp_old;
                    const double *keep = row + 2 * D2;
                    for (int64_t d = ln; d < D2; d += kWave) pb[pflip + part * D2 + d] = better ? row[d] : keep[d];
                    if (ln == 0) fpb[pflip + part] = better ? f : fp_old;
                    phase_stamp(clk, 5);   // personal best on its way to memory
                } else if (f < fp_old) {
                    for (int64_t d = ln; d < D2; d += kWave) pb[part * D2 + d] = row[d];
                    if (ln == 0) fpb[part] = f;
                }
            }
        }
    }
};

// One segment per particle: the wave has the whole sum and writes f (returned: a device batch's wave goes on with it).
template <bool WRITE_R, int FIT_IM>
__device__ __forceinline__ double finish_wave(const double ss, const double ss_im, const int64_t N, const int64_t particle, const int lane,
                                              double *out)
{
    double f = 0.0;
    if (FIT_IM == 0)
        f = sqrt(ss / (double)N);
    else   // (rmse_real + rmse_imag) / 2, equations.py:205-209
        f = 0.5 * (sqrt(ss / (double)N) + sqrt(ss_im / (double)N));
    if constexpr (WRITE_R && FIT_IM != 0) {   // residual rows of both channels: the two RMSEs, not their mean (out: [S][2])
        if (lane == 0) {
            out[2 * particle] = sqrt(ss / (double)N);
            out[2 * particle + 1] = sqrt(ss_im / (double)N);
        }
    } else {
        if (lane == 0) out[particle] = f;
    }
    return f;
}

}  // namespace
}  // namespace nmrfit

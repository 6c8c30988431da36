// lsq.hip -- the least-squares pieces of a fit on the device (include/nmrfit_amd_lsq.h): from D + 1 residual rows that
// are already in device memory, the forward-difference Jacobian J (N x D, the layout scipy receives), the residual r, and
// the normal equations A = J^T J, g = J^T r; plus the residual-rows launch over every fit of a resident batch.
//
// lsq_normal_kernel is the stages of lsq_tile.h -- which states the plan -- with J and r written out of the tile: the tile
// of J as ONE contiguous run of 64 D doubles (row-major N x D: the tile's rows follow each other in memory).  A and g are
// the same thing to the kernel: g_i is the "pair" (i, D).  
#include "lsq_tile.h"
#include "objective_kernel.h"

namespace nmrfit {
namespace {

__global__ __launch_bounds__(kLsqThreads) void lsq_normal_kernel(const LsqJob *__restrict__ jobs)
{
    extern __shared__ double T[];   // [kLsqTile][pitch]
    const LsqJob &q = jobs[blockIdx.y];
    if ((int)blockIdx.x >= q.nseg) return;   // (a batch's launch is as wide as its longest grid needs)
    const int D = q.D, pitch = (D + 1) | 1;
    const int64_t N = q.N;
    const int tid = threadIdx.x, jl = tid & (kLsqTile - 1);
    // (the wave's index where the compiler can see that it is one value per wave: the column loop of lsq_form then counts in
    // scalar registers -- 132 VGPRs; with `tid >> 6` 138, above the kernel's bar of 136.  The meat kernels have no scalar
    // registers to spare for it: lsq_meat_im_kernel would park six in vector lanes)
    const int i0 = __builtin_amdgcn_readfirstlane(tid >> 6);
    const bool sums = q.partial != nullptr;
    const int nout = sums ? D * (D + 1) / 2 + D : 0;
    int pa[kLsqAcc], pb[kLsqAcc];
    double acc[kLsqAcc];
    lsq_own_pairs(nout, [D](int o, int *a, int *b) { lsq_pair(o, D, a, b); }, pa, pb, acc);
    int64_t t0, t1;
    lsq_tile_range(N, q.seg_tiles, &t0, &t1);
    for (int64_t t = t0; t < t1; ++t) {
        const int64_t j0 = t * kLsqTile;
        const int nj = (int)((N - j0 < kLsqTile) ? N - j0 : kLsqTile);
        const bool have = jl < nj;
        lsq_form(T, pitch, q.R, q.c, q.s, N, D, j0, have, i0, 0, D + 1);
        __syncthreads();
        if (q.J) {   // rows j0 .. j0 + nj of the row-major N x D matrix: nj D consecutive doubles
            double *__restrict__ Jt = q.J + j0 * D;
            for (int e = tid; e < nj * D; e += kLsqThreads) {
                const int jj = e / D;
                Jt[e] = T[jj * pitch + (e - jj * D)];
            }
        }
        if (q.r && i0 == 0 && have) q.r[j0 + jl] = T[jl * pitch + D];
        if (sums) lsq_accumulate<false>(T, pitch, T, pitch, nullptr, nj, pa, pb, acc);
        __syncthreads();
    }
    if (sums) lsq_store_partial(q.partial, nout, acc);
}

// the segments' sums one after the other, segment 0 first; A comes back whole (both triangles from the same sum)
__global__ __launch_bounds__(kLsqThreads) void lsq_reduce_kernel(const LsqJob *__restrict__ jobs)
{
    const LsqJob &q = jobs[blockIdx.x];
    if (!q.partial) return;
    const int D = q.D, nout = D * (D + 1) / 2 + D;
    for (int o = threadIdx.x; o < nout; o += kLsqThreads) {
        const double sum = lsq_segment_sum(q.partial, q.nseg, nout, o);
        int a, b;
        lsq_pair(o, D, &a, &b);
        if (b == D) {
            if (q.g) q.g[a] = sum;
        } else if (q.A) {
            q.A[a * D + b] = sum;
            q.A[b * D + a] = sum;
        }
    }
}

// J and r of one fit of any D, element by element
__global__ __launch_bounds__(kLsqThreads) void lsq_jacobian_plain_kernel(LsqJob q)
{
    const int64_t N = q.N, D = q.D;
    const int64_t stride = (int64_t)gridDim.x * kLsqThreads;
    for (int64_t e = (int64_t)blockIdx.x * kLsqThreads + threadIdx.x; e < N * D; e += stride) {
        const int64_t j = e / D, i = e - j * D;
        if (q.J) q.J[e] = (q.R[(i + 1) * N + j] - q.R[j]) * q.c[i];
        if (q.r && i == 0) q.r[j] = q.R[j] * q.s;
    }
}

// Residual rows of every fit of a resident batch: workgroup b belongs to fit b / blocks_per_fit, wave = parameter row,
// one segment (the wave walks the fit's whole grid and writes f itself, block sums in grid order).  The body is the lone
// residual kernel's -- objective_body<DEFAULT, WRITE_R> -- on the fit's own block structure, which follows from its N
// alone: rows and f are what nmrfit_residual_batch gives on a context of the same spectrum, bit for bit.
// FIT_IM 1, 2 (a batch has one mode): rows of both channels, R [2][S][N] and f [S][2] per fit -- what
// nmrfit_residual_batch_im gives (include/nmrfit_amd_lsq_im.h).  Instantiation 0 is the kernel as it was.
template <int FIT_IM>
__global__ __launch_bounds__(kWave *kWavesPerBlock, objective_min_waves(NMRFIT_VARIANT_DEFAULT, FIT_IM)) void residual_rows_batch_kernel(
    const RowsFit *__restrict__ fits, int blocks_per_fit, const unsigned aux_off)
{
    extern __shared__ __align__(16) unsigned char lds_raw[];
    __shared__ double wsums[kWsumsCount];
    const int fit = (int)(blockIdx.x / (unsigned)blocks_per_fit);
    const int64_t lblock = (int64_t)(blockIdx.x - (unsigned)fit * (unsigned)blocks_per_fit);
    const RowsFit &d = fits[fit];
    if (lblock * kWavesPerBlock >= d.S) return;   // (a fit with fewer rows than the batch's largest: whole workgroups idle)
    if (threadIdx.x == 0) wsums[2 * kMaxBlocks + 1] = 0.0;   // no personal bests here
    const int64_t g = lblock * kWavesPerBlock + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const PsoFused none{};
    objective_body<NMRFIT_VARIANT_DEFAULT, true, FIT_IM, kWavesPerBlock>(lds_raw, g, lblock, d.wc, d.u, d.v, d.wt, d.chunk, d.X, d.S, d.P, d.N,
                                                                   d.w0, d.wspan, 1, d.seg_len, d.blk_chunks, d.n_blocks, d.n_blocks,
                                                                   d.lane_step, d.rec_devk, d.f, d.R, nullptr, none, aux_off, wsums);
}

}  // namespace

int launch_lsq(hipStream_t st, const LsqJob *d_jobs, int32_t K, int32_t Dmax, bool sums)
{
    if (K <= 0) return NMRFIT_OK;
    if (Dmax > kLsqMaxD) {
        set_error("normal equations: D = 4 + 3 P above " + std::to_string(kLsqMaxD));
        return NMRFIT_E_UNSUPPORTED;
    }
    const size_t lds = (size_t)kLsqTile * (size_t)((Dmax + 1) | 1) * sizeof(double);
    hipLaunchKernelGGL(lsq_normal_kernel, dim3((unsigned)kLsqMaxSegments, (unsigned)K), dim3(kLsqThreads), lds, st, d_jobs);
    NMRFIT_HIP(hipGetLastError());
    if (sums) {
        hipLaunchKernelGGL(lsq_reduce_kernel, dim3((unsigned)K), dim3(kLsqThreads), 0, st, d_jobs);
        NMRFIT_HIP(hipGetLastError());
    }
    return NMRFIT_OK;
}

int launch_lsq_plain(hipStream_t st, const LsqJob &job)
{
    const int64_t n = job.N * job.D;
    if (n <= 0) return NMRFIT_OK;
    const int64_t blocks = std::min<int64_t>((n + kLsqThreads - 1) / kLsqThreads, 4096);
    hipLaunchKernelGGL(lsq_jacobian_plain_kernel, dim3((unsigned)blocks), dim3(kLsqThreads), 0, st, job);
    NMRFIT_HIP(hipGetLastError());
    return NMRFIT_OK;
}

bool rows_batch_lds(int32_t Pmax, int fit_im, size_t *lds, unsigned *aux_off)
{
    int v = NMRFIT_VARIANT_DEFAULT;
    *lds = objective_lds(NMRFIT_VARIANT_DEFAULT, Pmax, true, fit_im, &v, aux_off, kWavesPerBlock, kWavesPerBlock, 0);
    return v == NMRFIT_VARIANT_DEFAULT && lds_fits(*lds, kObjectiveStaticLds);
}

int launch_rows_batch(hipStream_t st, const RowsFit *d_fits, int32_t K, int64_t Smax, size_t lds, unsigned aux_off, int fit_im)
{
    if (K <= 0 || Smax <= 0) return NMRFIT_OK;
    const int64_t blocks_per_fit = (Smax + kWavesPerBlock - 1) / kWavesPerBlock;
    if (blocks_per_fit * (int64_t)K > 0x7fffffffLL) {
        set_error("batch too large for one launch");
        return NMRFIT_E_INVALID;
    }
    const dim3 grid((unsigned)(blocks_per_fit * K)), block(kWave * kWavesPerBlock);
    if (fit_im == 0)
        hipLaunchKernelGGL(residual_rows_batch_kernel<0>, grid, block, lds, st, d_fits, (int)blocks_per_fit, aux_off);
    else if (fit_im == 1)
        hipLaunchKernelGGL(residual_rows_batch_kernel<1>, grid, block, lds, st, d_fits, (int)blocks_per_fit, aux_off);
    else
        hipLaunchKernelGGL(residual_rows_batch_kernel<2>, grid, block, lds, st, d_fits, (int)blocks_per_fit, aux_off);
    NMRFIT_HIP(hipGetLastError());
    return NMRFIT_OK;
}

}  // namespace nmrfit

// lsq_cov_im.hip -- the "meat" of the sandwich covariance of a fit made on BOTH channels (include/nmrfit_amd_cov_im.h):
// from the two planes of D + 1 residual rows that the both-channel rows launch of the same call has just written, the
// three blocks Mt_rr, Mt_ii, Mt_ri of Mt_ab = Jt_a^T diag(q_ab) Jt_b, Jt_ch = [J_ch | r_ch] (C = D + 1 columns: the last
// one carries the derivative of 1 / rho_ch); and nmrfit_sandwich_im, the call on a context.
//
// lsq_meat_im_kernel is lsq_meat_kernel (lsq_cov.hip) with one column and one operand more.  A workgroup owns a segment
// of the grid (lsq_segments) and one JOB of a fit: a symmetric block's upper triangle, C (C + 1) / 2 <= 3003 entries, or a
// band of rows of the cross block, at most 39 x 77 = 3003 -- twelve sums per thread either way.  Per tile of 64 points it
// forms T[j][i < D] = (R_b[i + 1][j] - R_b[0][j]) * c_i and T[j][D] = R_b[0][j] * s in LDS at an odd pitch, for a cross job
// also the band's own columns of channel a (Ta: the whole launch stays below 64 KiB of LDS at D = 76), and one wave
// forms the q of the job's kind from the RESIDENT weights, s and sincos(p0 + p1 * (j / N)) in fp64.  Then
//     acc = fma(q_j * Ta[j][x], T[j][y], acc)
// point after point.  The expressions and the order over j are lsq_meat_kernel's: the D x D corner of Mt_rr is its M bit
// for bit, and q_ri is a multiple of sigma_u^2 - sigma_v^2, formed once on the host: the cross block is exactly 0 when the
// two are equal.  Per-segment sums go to memory; lsq_meat_im_reduce_kernel adds them segment 0 first, writes both
// triangles of a symmetric block from the one sum and every cross entry once.  No atomics; every order is fixed by N.
// The kernel does not know the imaginary model's mode: it differs in the rows alone.  
#include "host_call.h"
#include "lsq_internal.h"
#include "nmrfit_amd_cov_im.h"

#include <cmath>

namespace nmrfit {
namespace {

constexpr int kMeatWaves = kLsqThreads / kLsqTile;

// the rows of the cross block's first band: the second takes the rest
inline int32_t cross_split(int32_t C) { return (C + 1) / 2; }
static_assert(kLsqThreads * kLsqAcc >= (kLsqMaxD + 1) * (kLsqMaxD + 2) / 2, "accumulators for a symmetric block of the largest D");
static_assert(kLsqThreads * kLsqAcc >= ((kLsqMaxD + 2) / 2) * (kLsqMaxD + 1), "accumulators for a band of the cross block");

__global__ __launch_bounds__(kLsqThreads) void lsq_meat_im_kernel(const LsqMeatImJob *__restrict__ jobs)
{
    extern __shared__ double T[];   // [kLsqTile][pitch]; a cross job: then Ta [kLsqTile][pitch_a]; then Q [kLsqTile]
    const LsqMeatImJob &q = jobs[blockIdx.y];
    if ((int)blockIdx.x >= q.nseg) return;   // (a launch is as wide as its longest grid needs)
    const int D = q.D, C = D + 1, pitch = C | 1;
    const bool cross = q.kind == kMeatImRI;
    const int row0 = q.row0, na = q.row1 - q.row0, pitch_a = cross ? (na | 1) : pitch;
    double *Ta = cross ? T + kLsqTile * pitch : T;
    double *Q = Ta + (cross ? kLsqTile * pitch_a : kLsqTile * pitch);
    const int64_t N = q.N;
    const int tid = threadIdx.x, jl = tid & (kLsqTile - 1), i0 = tid >> 6;
    const int nout = cross ? na * C : C * (C + 1) / 2;
    int pa[kLsqAcc], pb[kLsqAcc];
    double acc[kLsqAcc];
#pragma unroll
    for (int m = 0; m < kLsqAcc; ++m) {
        const int o = tid + m * kLsqThreads;
        pa[m] = pb[m] = 0;
        if (o < nout) {
            if (cross) {
                pa[m] = o / C;   // (the band's own column of Ta)
                pb[m] = o - pa[m] * C;
            } else {
                lsq_pair(o, C, &pa[m], &pb[m]);
            }
        }
        acc[m] = 0.0;
    }
    const int64_t tiles = (N + kLsqTile - 1) / kLsqTile;
    const int64_t t0 = (int64_t)blockIdx.x * q.seg_tiles;
    const int64_t t1 = (t0 + q.seg_tiles < tiles) ? t0 + q.seg_tiles : tiles;
    const double *__restrict__ Ra = q.Ra;
    const double *__restrict__ Rb = q.Rb;
    const double *__restrict__ c = q.c;
    for (int64_t t = t0; t < t1; ++t) {
        const int64_t j0 = t * kLsqTile;
        const int nj = (int)((N - j0 < kLsqTile) ? N - j0 : kLsqTile);
        const bool have = jl < nj;
        const double r0 = have ? Rb[j0 + jl] : 0.0;
        for (int i = i0; i < D; i += kMeatWaves) {
            const double ri = have ? Rb[(int64_t)(i + 1) * N + j0 + jl] : 0.0;
            T[jl * pitch + i] = (ri - r0) * c[i];
        }
        if (i0 == (D & (kMeatWaves - 1))) T[jl * pitch + D] = r0 * q.s;   // (the wave whose turn column D is)
        if (cross) {
            const double a0 = have ? Ra[j0 + jl] : 0.0;
            for (int i = row0 + i0; i < row0 + na; i += kMeatWaves) {
                if (i < D) {
                    const double ai = have ? Ra[(int64_t)(i + 1) * N + j0 + jl] : 0.0;
                    Ta[jl * pitch_a + (i - row0)] = (ai - a0) * c[i];
                } else {
                    Ta[jl * pitch_a + (i - row0)] = a0 * q.s;
                }
            }
        }
        if (i0 == kMeatWaves - 1) {
            double qj = 0.0;
            if (have) {
                const int64_t j = j0 + jl;
                double sn, cs;
                sincos(q.p0 + q.p1 * ((double)j / (double)N), &sn, &cs);
                const double ws = q.wt[grid_slot(j)] * q.s;
                if (q.kind == kMeatImRR)
                    qj = (ws * ws) * (cs * cs * q.var_u + sn * sn * q.var_v);
                else if (q.kind == kMeatImII)
                    qj = (ws * ws) * (sn * sn * q.var_u + cs * cs * q.var_v);
                else
                    qj = (ws * ws) * (cs * sn * q.var_u);   // (var_u holds sigma_u^2 - sigma_v^2)
            }
            Q[jl] = qj;
        }
        __syncthreads();
        for (int jj = 0; jj < nj; ++jj) {
            const double *rowa = Ta + jj * pitch_a;
            const double *rowb = T + jj * pitch;
            const double qq = Q[jj];
#pragma unroll
            for (int m = 0; m < kLsqAcc; ++m) acc[m] = __builtin_fma(qq * rowa[pa[m]], rowb[pb[m]], acc[m]);
        }
        __syncthreads();
    }
    double *__restrict__ out = q.partial + (int64_t)blockIdx.x * nout;
#pragma unroll
    for (int m = 0; m < kLsqAcc; ++m) {
        const int o = tid + m * kLsqThreads;
        if (o < nout) out[o] = acc[m];
    }
}

// the segments' sums one after the other, segment 0 first; a symmetric block comes back whole (both triangles from the
// same sum), a band of the cross block entry by entry
__global__ __launch_bounds__(kLsqThreads) void lsq_meat_im_reduce_kernel(const LsqMeatImJob *__restrict__ jobs)
{
    const LsqMeatImJob &q = jobs[blockIdx.x];
    const int C = q.D + 1;
    const bool cross = q.kind == kMeatImRI;
    const int nout = cross ? (q.row1 - q.row0) * C : C * (C + 1) / 2;
    for (int o = threadIdx.x; o < nout; o += kLsqThreads) {
        double sum = 0.0;
        for (int sgm = 0; sgm < q.nseg; ++sgm) sum += q.partial[(int64_t)sgm * nout + o];
        if (cross) {
            q.M[q.row0 * C + o] = sum;
        } else {
            int a, b;
            lsq_pair(o, C, &a, &b);
            q.M[a * C + b] = sum;
            q.M[b * C + a] = sum;
        }
    }
}

}  // namespace

int64_t lsq_meat_im_partials(int64_t N, int64_t D)
{
    int32_t nseg, seg_tiles;
    lsq_segments(N, &nseg, &seg_tiles);
    const int64_t C = D + 1;
    return nseg * (C * (C + 1) + C * C);   // two upper triangles and the whole cross block
}

void lsq_meat_im_jobs(LsqMeatImJob job[4], const double *R, const double *c, const double *wt, double s, double p0, double p1,
                      double sigma_u, double sigma_v, int64_t N, int32_t D, double *partial, double *M)
{
    const int32_t C = D + 1;
    const double *plane[2] = {R, R + (int64_t)C * N};
    const double var_u = sigma_u * sigma_u, var_v = sigma_v * sigma_v;
    for (int n = 0; n < 4; ++n) {
        LsqMeatImJob &j = job[n];
        j = LsqMeatImJob{};
        j.kind = n < 2 ? n : kMeatImRI;
        j.Ra = plane[n == 1 ? 1 : 0];
        j.Rb = plane[n == 0 ? 0 : 1];
        j.c = c;
        j.wt = wt;
        j.s = s;
        j.p0 = p0;
        j.p1 = p1;
        j.var_u = j.kind == kMeatImRI ? var_u - var_v : var_u;
        j.var_v = j.kind == kMeatImRI ? 0.0 : var_v;
        j.N = N;
        j.D = D;
        lsq_segments(N, &j.nseg, &j.seg_tiles);
        j.row0 = n == 3 ? cross_split(C) : 0;
        j.row1 = n == 2 ? cross_split(C) : C;
        j.partial = partial;
        j.M = M + (int64_t)j.kind * C * C;
        partial += j.nseg * lsq_meat_im_sums(j);
    }
}

int launch_lsq_meat_im(hipStream_t st, const LsqMeatImJob *d_jobs, int32_t njobs, int32_t Dmax)
{
    if (njobs <= 0) return NMRFIT_OK;
    if (Dmax > kLsqMaxD) {
        set_error("sandwich_im: D = 4 + 3 P above " + std::to_string(kLsqMaxD));
        return NMRFIT_E_UNSUPPORTED;
    }
    // the largest job of the launch: a band of the cross block, T and Ta, and the q row
    const int C = Dmax + 1;
    const size_t lds = (size_t)kLsqTile * (size_t)((C | 1) + (cross_split(C) | 1) + 1) * sizeof(double);
    hipLaunchKernelGGL(lsq_meat_im_kernel, dim3((unsigned)kLsqMaxSegments, (unsigned)njobs), dim3(kLsqThreads), lds, st, d_jobs);
    NMRFIT_HIP(hipGetLastError());
    hipLaunchKernelGGL(lsq_meat_im_reduce_kernel, dim3((unsigned)njobs), dim3(kLsqThreads), 0, st, d_jobs);
    NMRFIT_HIP(hipGetLastError());
    return NMRFIT_OK;
}

}  // namespace nmrfit

using namespace nmrfit;

#pragma GCC visibility push(default)   // the C-ABI: the only symbols the library exports (build.sh: -fvisibility=hidden)
extern "C" {

// A, g and rho are nmrfit_jacobian_im's own (ctx_eval.hip): that call leaves the two planes of D + 1 residual rows in the
// context's d_R and the factors behind the parameter rows in d_X, and the meat launch reads them there, on the same
// stream.  The records and sums of the meat are one Scratch block of this call.
int nmrfit_sandwich_im(nmrfit_ctx *ctx, int32_t P, int fit_im, const double *rows, const double *c, double s, double sigma_u,
                       double sigma_v, double *A_out, double *g_out, double *rho_out, double *M_out)
{
    int rc = bind(ctx);
    if (rc != NMRFIT_OK) return rc;
    if (!rows || !c) return refuse(NMRFIT_E_INVALID, "nmrfit_sandwich_im: null rows or c");
    if (fit_im != NMRFIT_FIT_IM_REFERENCE && fit_im != NMRFIT_FIT_IM_SUM)
        return refuse(NMRFIT_E_INVALID, "nmrfit_sandwich_im: fit_im must be 1 (reference fit_im=True) or 2 (all-peak imaginary model)");
    if ((rc = check_batch(1, P, rows, c)) != NMRFIT_OK) return rc;
    if ((rc = check_sigma("nmrfit_sandwich_im", sigma_u, sigma_v)) != NMRFIT_OK) return rc;
    const int64_t D = 4 + 3 * (int64_t)P, B = D + 1, C = D + 1, N = ctx->N;
    if (D > kLsqMaxD) return refuse(NMRFIT_E_UNSUPPORTED, "nmrfit_sandwich_im: D = 4 + 3 P <= " + std::to_string(kLsqMaxD));
    if (ctx->variant != NMRFIT_VARIANT_DEFAULT)
        return refuse(NMRFIT_E_UNSUPPORTED, "nmrfit_sandwich_im: the context's kernel variant must be DEFAULT");
    if (!A_out && !g_out && !rho_out && !M_out) return NMRFIT_OK;
    // (with M alone the call still runs the rows launch: rho is the cheapest thing to ask of it)
    double rho_own[2] = {0.0, 0.0};
    rc = nmrfit_jacobian_im(ctx, P, rows, c, s, fit_im, nullptr, nullptr, A_out, g_out,
                            rho_out ? rho_out : (A_out || g_out ? nullptr : rho_own));
    if (rc != NMRFIT_OK || !M_out) return rc;
    const int64_t kJobDoubles = (int64_t)(align256(4 * sizeof(LsqMeatImJob)) / sizeof(double));
    const int64_t n_partial = lsq_meat_im_partials(N, D), n_M = 3 * C * C;
    hipStream_t st = ctx->stream;
    Scratch mem;
    const auto enqueue_and_wait = [&]() -> int {
        double *d_mem = nullptr;
        NMRFIT_HIP(mem.alloc(&d_mem, (size_t)(kJobDoubles + n_partial + n_M)));
        double *d_M = d_mem + kJobDoubles + n_partial;
        LsqMeatImJob job[4];
        lsq_meat_im_jobs(job, ctx->d_R, ctx->d_X + B * D, ctx->d_wt, s, rows[0], rows[1], sigma_u, sigma_v, N, (int32_t)D,
                         d_mem + kJobDoubles, d_M);
        // (pageable host memory: the copy has left `job` when hipMemcpyAsync returns)
        NMRFIT_HIP(hipMemcpyAsync(d_mem, job, sizeof(job), hipMemcpyHostToDevice, st));
        const int launched = launch_lsq_meat_im(st, reinterpret_cast<const LsqMeatImJob *>(d_mem), 4, (int32_t)D);
        if (launched != NMRFIT_OK) return launched;
        NMRFIT_HIP(hipMemcpyAsync(M_out, d_M, (size_t)n_M * sizeof(double), hipMemcpyDeviceToHost, st));
        NMRFIT_HIP(hipStreamSynchronize(st));
        return NMRFIT_OK;
    };
    rc = enqueue_and_wait();
    if (rc != NMRFIT_OK) (void)hipStreamSynchronize(st);   // what was enqueued may still use the buffers `mem` frees
    return rc;
}

}  // extern "C"
#pragma GCC visibility pop

// ctx_eval.hip -- the evaluation calls on a context (ctx.hip): objective values and residual rows of parameter rows in
// host or device memory, the reconstruction of one fit, and the Jacobian of include/nmrfit_amd_lsq.h / _lsq_im.h.  Each
// enqueues on the context's stream and, in its host-pointer form, waits for it.  No exception leaves this file.
#include "host_call.h"
#include "lsq_internal.h"
#include "result_internal.h"

#include <cstring>
#include <vector>

using namespace nmrfit;

#pragma GCC visibility push(default)   // the C-ABI: the only symbols the library exports (build.sh: -fvisibility=hidden)
extern "C" {

int nmrfit_objective_batch_dev(nmrfit_ctx *ctx, int64_t S, int32_t P, const double *dX, double *df_out)
{
    int rc = bind(ctx);
    if (rc != NMRFIT_OK) return rc;
    rc = check_batch(S, P, dX, df_out);
    if (rc != NMRFIT_OK) return rc;
    return launch_objective(ctx, S, P, dX, df_out, nullptr);
}

int nmrfit_residual_batch_dev(nmrfit_ctx *ctx, int64_t B, int32_t P, const double *dX, double *dR_out, double *df_out)
{
    int rc = bind(ctx);
    if (rc != NMRFIT_OK) return rc;
    rc = check_batch(B, P, dX, dR_out);
    if (rc != NMRFIT_OK) return rc;
    if (B == 0) return NMRFIT_OK;
    if (!df_out) {
        rc = ensure(ctx, &ctx->d_f, &ctx->cap_f, B);
        if (rc != NMRFIT_OK) return rc;
        df_out = ctx->d_f;
    }
    return launch_objective(ctx, B, P, dX, df_out, dR_out);
}

int nmrfit_objective_batch(nmrfit_ctx *ctx, int64_t S, int32_t P, const double *X, int fit_im, double *f_out)
{
    int rc = bind(ctx);
    if (rc != NMRFIT_OK) return rc;
    if ((rc = check_fit_im(fit_im)) != NMRFIT_OK) return rc;
    rc = check_batch(S, P, X, f_out);
    if (rc != NMRFIT_OK) return rc;
    if (S == 0) return NMRFIT_OK;
    const int64_t D = 4 + 3 * (int64_t)P;
    if ((rc = ensure(ctx, &ctx->d_X, &ctx->cap_X, S * D)) != NMRFIT_OK) return rc;
    if ((rc = ensure(ctx, &ctx->d_f, &ctx->cap_f, S)) != NMRFIT_OK) return rc;
    const int saved = ctx->fit_im;
    ctx->fit_im = fit_im;
    // (Round 6, measured and rejected: the upload cut into slices through pinned memory, the kernel of a slice starting as
    // soon as its rows have landed -- 1.52 ms per C3 call against 1.34 ms for this plain form, resident launch 1.20: four
    // kernels each drain on their own, which costs more than the 0.1 ms of upload they hide;
    // profiles/r06/host_pointer_pipelined_ab.txt.)
    const int64_t x_bytes = S * D * (int64_t)sizeof(double);
    {
        hipError_t e = hipMemcpyAsync(ctx->d_X, X, (size_t)x_bytes, hipMemcpyHostToDevice, ctx->stream);
        if (e != hipSuccess) {
            ctx->fit_im = saved;
            return hip_fail(e, "hipMemcpyAsync(X)", __FILE__, __LINE__);
        }
    }
    rc = launch_objective(ctx, S, P, ctx->d_X, ctx->d_f, nullptr);
    ctx->fit_im = saved;
    if (rc != NMRFIT_OK) return rc;
    NMRFIT_HIP(hipMemcpyAsync(f_out, ctx->d_f, (size_t)S * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    NMRFIT_HIP(hipStreamSynchronize(ctx->stream));
    return NMRFIT_OK;
}

// The reconstruction of ONE fit through the kernel of result.hip: scratch device memory for the parameter vector, the
// optional output grid and the outputs, one launch, the copies back.  (A device batch does the same for all its fits in
// one launch from its resident state: nmrfit_batch_contributions, batch_data.hip.)
static int generate_one(nmrfit_ctx *ctx, int32_t P, const double *x, int64_t Nout, const double *w_out, double *real_out,
                        double *imag_out, double *fit_out, double *data_out, const char *who)
{
    int rc = bind(ctx);
    if (rc != NMRFIT_OK) return rc;
    if (!w_out) Nout = ctx->N;
    if (P < 0 || P > kMaxPeaks || !x || Nout < 0 || (P > 0 && Nout > 0 && (!real_out != !imag_out))) {
        set_error(std::string(who) + ": bad arguments");
        return NMRFIT_E_INVALID;
    }
    const int64_t N = ctx->N;
    const int64_t n_contrib = real_out ? (int64_t)P * Nout : 0;
    const int64_t n_fit = fit_out ? 4 * Nout : 0, n_data = data_out ? 2 * N : 0;
    const int64_t n_out = 2 * n_contrib + n_fit + n_data;
    if (n_out == 0) return NMRFIT_OK;
    const int64_t D = 4 + 3 * (int64_t)P;
    hipStream_t st = ctx->stream;   // (the context's own: synchronised here, never handed to the stream cache)
    Scratch mem;
    const auto enqueue_and_wait = [&]() -> int {
        double *d_in = nullptr, *d_out = nullptr;
        NMRFIT_HIP(mem.alloc(&d_in, (size_t)(D + (w_out ? Nout : 0))));
        NMRFIT_HIP(mem.alloc(&d_out, (size_t)n_out));
        NMRFIT_HIP(hipMemcpyAsync(d_in, x, (size_t)D * sizeof(double), hipMemcpyHostToDevice, st));
        if (w_out) NMRFIT_HIP(hipMemcpyAsync(d_in + D, w_out, (size_t)Nout * sizeof(double), hipMemcpyHostToDevice, st));
        ResultJob job{};
        job.wc = ctx->d_wc;
        job.w_plain = w_out ? d_in + D : nullptr;   // (centred in the kernel with the context's offset: it works on w - w0)
        job.x = d_in;
        job.u = ctx->d_u;
        job.v = ctx->d_v;
        job.w0 = ctx->w0;
        job.wspan = ctx->wspan;
        job.Nout = Nout;
        job.N = N;
        job.P = P;
        job.real = real_out ? d_out : nullptr;
        job.imag = real_out ? d_out + n_contrib : nullptr;
        job.fit = fit_out ? d_out + 2 * n_contrib : nullptr;
        job.data = data_out ? d_out + 2 * n_contrib + n_fit : nullptr;
        const int launched = launch_result_one(st, job);
        if (launched != NMRFIT_OK) return launched;
        if (n_contrib) {
            NMRFIT_HIP(hipMemcpyAsync(real_out, job.real, (size_t)n_contrib * sizeof(double), hipMemcpyDeviceToHost, st));
            NMRFIT_HIP(hipMemcpyAsync(imag_out, job.imag, (size_t)n_contrib * sizeof(double), hipMemcpyDeviceToHost, st));
        }
        if (n_fit) NMRFIT_HIP(hipMemcpyAsync(fit_out, job.fit, (size_t)n_fit * sizeof(double), hipMemcpyDeviceToHost, st));
        if (n_data) NMRFIT_HIP(hipMemcpyAsync(data_out, job.data, (size_t)n_data * sizeof(double), hipMemcpyDeviceToHost, st));
        NMRFIT_HIP(hipStreamSynchronize(st));
        return NMRFIT_OK;
    };
    rc = enqueue_and_wait();
    if (rc != NMRFIT_OK) (void)hipStreamSynchronize(st);   // what was enqueued may still use the buffers `mem` frees
    return rc;
}

int nmrfit_contributions(nmrfit_ctx *ctx, int32_t P, const double *x, int64_t Nout, const double *w_out,
                         double *real_out, double *imag_out)
{
    if (P > 0 && (w_out ? Nout > 0 : true) && (!real_out || !imag_out)) {
        set_error("nmrfit_contributions: bad arguments");
        return NMRFIT_E_INVALID;
    }
    return generate_one(ctx, P, x, Nout, w_out, real_out, imag_out, nullptr, nullptr, "nmrfit_contributions");
}

int nmrfit_generate_result(nmrfit_ctx *ctx, int32_t P, const double *x, int64_t Nout, const double *w_out,
                           double *real_out, double *imag_out, double *fit_out, double *data_out)
{
    return generate_one(ctx, P, x, Nout, w_out, real_out, imag_out, fit_out, data_out, "nmrfit_generate_result");
}

// The channel modes of the both-channels calls (include/nmrfit_amd_lsq_im.h)
static int check_rows_im(int fit_im, const char *who)
{
    if (fit_im != NMRFIT_FIT_IM_REFERENCE && fit_im != NMRFIT_FIT_IM_SUM)
        return refuse(NMRFIT_E_INVALID, std::string(who) + ": fit_im must be 1 (reference fit_im=True) or 2 (all-peak imaginary model)");
    return NMRFIT_OK;
}

// Residual rows of B parameter rows on nch channels: one plane [B][N] of R and f [B] on the real channel alone (fit_im 0);
// with nch = 2 the rows launch writes the imaginary rows of the mode fit_im into a second plane of the same buffer, and
// f is [B][2], the two RMSEs of every row.
static int ctx_residual_batch(nmrfit_ctx *ctx, const char *who, int nch, int fit_im, int64_t B, int32_t P, const double *X,
                              double *R_out, double *f_out)
{
    int rc = bind(ctx);
    if (rc != NMRFIT_OK) return rc;
    if (nch == 2 && (rc = check_rows_im(fit_im, who)) != NMRFIT_OK) return rc;
    rc = check_batch(B, P, X, R_out);
    if (rc != NMRFIT_OK) return rc;
    if (B == 0) return NMRFIT_OK;
    const int64_t D = 4 + 3 * (int64_t)P, N = ctx->N;
    if ((rc = ensure(ctx, &ctx->d_X, &ctx->cap_X, B * D)) != NMRFIT_OK) return rc;
    if ((rc = ensure(ctx, &ctx->d_f, &ctx->cap_f, nch * B)) != NMRFIT_OK) return rc;
    if ((rc = ensure(ctx, &ctx->d_R, &ctx->cap_R, nch * B * N)) != NMRFIT_OK) return rc;
    NMRFIT_HIP(hipMemcpyAsync(ctx->d_X, X, (size_t)(B * D) * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    if ((rc = launch_objective(ctx, B, P, ctx->d_X, ctx->d_f, ctx->d_R, nullptr, nullptr, fit_im)) != NMRFIT_OK) return rc;
    NMRFIT_HIP(hipMemcpyAsync(R_out, ctx->d_R, (size_t)(nch * B * N) * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    if (f_out)
        NMRFIT_HIP(hipMemcpyAsync(f_out, ctx->d_f, (size_t)(nch * B) * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    NMRFIT_HIP(hipStreamSynchronize(ctx->stream));
    return NMRFIT_OK;
}

int nmrfit_residual_batch(nmrfit_ctx *ctx, int64_t B, int32_t P, const double *X, double *R_out, double *f_out)
{
    return ctx_residual_batch(ctx, "nmrfit_residual_batch", 1, 0, B, P, X, R_out, f_out);
}

int nmrfit_residual_batch_im(nmrfit_ctx *ctx, int64_t B, int32_t P, const double *X, int fit_im, double *R_out, double *f2_out)
{
    return ctx_residual_batch(ctx, "nmrfit_residual_batch_im", 2, fit_im, B, P, X, R_out, f2_out);
}

// include/nmrfit_amd_lsq.h and nmrfit_amd_lsq_im.h: the D + 1 residual rows of a forward-difference Jacobian stay on the
// device; what comes back is J in scipy's layout, r, and / or the D x D normal equations, per channel.  One upload (rows, c,
// the kernels' records), the rows launch, the kernels of lsq.hip -- a channel is one job of theirs, on its plane of the
// rows -- and the copies back (J and r through the pinned staging buffers).  The workspace is [J, r, partial, A, g] per
// channel; every output has the channel as its leading index, f is the nch RMSEs of row 0.  (R stays in d_R and c behind the rows in d_X: nmrfit_sandwich, lsq_cov.hip, reads them there.)
static int ctx_jacobian(nmrfit_ctx *ctx, const char *who, int nch, int fit_im, int32_t P, const double *rows, const double *c,
                        double s, double *J_out, double *r_out, double *A_out, double *g_out, double *f_out)
{
    int rc = bind(ctx);
    if (rc != NMRFIT_OK) return rc;
    if (!rows || !c) return refuse(NMRFIT_E_INVALID, std::string(who) + ": null rows or c");
    if (nch == 2 && (rc = check_rows_im(fit_im, who)) != NMRFIT_OK) return rc;
    rc = check_batch(1, P, rows, c);
    if (rc != NMRFIT_OK) return rc;
    const int64_t D = 4 + 3 * (int64_t)P, B = D + 1, N = ctx->N;
    const bool sums = A_out || g_out;
    if (sums && D > kLsqMaxD)
        return refuse(NMRFIT_E_UNSUPPORTED, std::string(who) + ": A and g need D = 4 + 3 P <= " + std::to_string(kLsqMaxD));
    if (!J_out && !r_out && !sums && !f_out) return NMRFIT_OK;
    constexpr int64_t kJobDoubles = sizeof(LsqJob) / sizeof(double);
    static_assert(sizeof(LsqJob) % sizeof(double) == 0, "two jobs follow each other in a buffer of doubles");
    LsqJob job[2] = {};
    lsq_segments(N, &job[0].nseg, &job[0].seg_tiles);
    const int64_t n_partial = sums ? job[0].nseg * lsq_sums(D) : 0;
    const int64_t n_J = J_out ? N * D : 0, n_r = r_out ? N : 0, n_Ag = sums ? D * D + D : 0;
    const int64_t n_ch = n_J + n_r + n_partial + n_Ag;   // one channel's share of the workspace
    const int64_t n_up = B * D + D + nch * kJobDoubles;
    if ((rc = ensure(ctx, &ctx->d_X, &ctx->cap_X, n_up)) != NMRFIT_OK) return rc;
    if ((rc = ensure(ctx, &ctx->d_f, &ctx->cap_f, nch * B)) != NMRFIT_OK) return rc;
    if ((rc = ensure(ctx, &ctx->d_R, &ctx->cap_R, nch * B * N)) != NMRFIT_OK) return rc;
    if ((rc = ensure(ctx, &ctx->d_lsq, &ctx->cap_lsq, nch * n_ch + 1)) != NMRFIT_OK) return rc;
    double *d_c = ctx->d_X + B * D, *d_job = d_c + D;
    double *d_J[2], *d_r[2], *d_A[2], *d_g[2];
    for (int ch = 0; ch < nch; ++ch) {
        d_J[ch] = ctx->d_lsq + ch * n_ch;
        d_r[ch] = d_J[ch] + n_J;
        double *d_partial = d_r[ch] + n_r;
        d_A[ch] = d_partial + n_partial;
        d_g[ch] = d_A[ch] + (sums ? D * D : 0);
        LsqJob &q = job[ch];
        q.R = ctx->d_R + ch * B * N;   // the channel's plane of the rows
        q.c = d_c;
        q.s = s;
        q.N = N;
        q.D = (int32_t)D;
        q.nseg = job[0].nseg;
        q.seg_tiles = job[0].seg_tiles;
        q.J = J_out ? d_J[ch] : nullptr;
        q.r = r_out ? d_r[ch] : nullptr;
        q.partial = sums ? d_partial : nullptr;
        q.A = sums ? d_A[ch] : nullptr;
        q.g = sums ? d_g[ch] : nullptr;
    }
    hipStream_t st = ctx->stream;
    std::vector<double> up((size_t)n_up);
    memcpy(up.data(), rows, (size_t)(B * D) * sizeof(double));
    memcpy(up.data() + B * D, c, (size_t)D * sizeof(double));
    memcpy(up.data() + B * D + D, job, (size_t)nch * sizeof(LsqJob));
    // (pageable host memory: the copy has left `up` when hipMemcpyAsync returns)
    NMRFIT_HIP(hipMemcpyAsync(ctx->d_X, up.data(), up.size() * sizeof(double), hipMemcpyHostToDevice, st));
    if ((rc = launch_objective(ctx, B, P, ctx->d_X, ctx->d_f, ctx->d_R, nullptr, nullptr, fit_im)) != NMRFIT_OK) return rc;
    if (J_out || r_out || sums) {
        if (D <= kLsqMaxD) {
            rc = launch_lsq(st, reinterpret_cast<const LsqJob *>(d_job), nch, (int32_t)D, sums);
        } else {
            for (int ch = 0; ch < nch && rc == NMRFIT_OK; ++ch) rc = launch_lsq_plain(st, job[ch]);
        }
        if (rc != NMRFIT_OK) return rc;
    }
    for (int ch = 0; ch < nch; ++ch) {
        if (A_out) NMRFIT_HIP(hipMemcpyAsync(A_out + ch * D * D, d_A[ch], (size_t)(D * D) * sizeof(double), hipMemcpyDeviceToHost, st));
        if (g_out) NMRFIT_HIP(hipMemcpyAsync(g_out + ch * D, d_g[ch], (size_t)D * sizeof(double), hipMemcpyDeviceToHost, st));
    }
    if (f_out) NMRFIT_HIP(hipMemcpyAsync(f_out, ctx->d_f, (size_t)nch * sizeof(double), hipMemcpyDeviceToHost, st));   // row 0's
    for (int ch = 0; ch < nch; ++ch) {
        if (r_out && (rc = staged_d2h(ctx->device, st, r_out + ch * N, d_r[ch], (size_t)N * sizeof(double))) != NMRFIT_OK) return rc;
        if (J_out && (rc = staged_d2h(ctx->device, st, J_out + ch * N * D, d_J[ch], (size_t)(N * D) * sizeof(double))) != NMRFIT_OK) return rc;
    }
    NMRFIT_HIP(hipStreamSynchronize(st));
    return NMRFIT_OK;
}

// the real channel: whatever kernel variant the context is set to
int nmrfit_jacobian(nmrfit_ctx *ctx, int32_t P, const double *rows, const double *c, double s, double *J_out, double *r_out,
                    double *A_out, double *g_out, double *f_out)
{
    return ctx_jacobian(ctx, "nmrfit_jacobian", 1, 0, P, rows, c, s, J_out, r_out, A_out, g_out, f_out);
}

// both channels: the rows launch takes the DEFAULT kernel alone (launch_objective refuses another)
int nmrfit_jacobian_im(nmrfit_ctx *ctx, int32_t P, const double *rows, const double *c, double s, int fit_im, double *J_out,
                       double *r_out, double *A_out, double *g_out, double *f2_out)
{
    return ctx_jacobian(ctx, "nmrfit_jacobian_im", 2, fit_im, P, rows, c, s, J_out, r_out, A_out, g_out, f2_out);
}

}  // extern "C"
#pragma GCC visibility pop

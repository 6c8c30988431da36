// ctx.hip -- the context object of include/nmrfit_amd.h: one spectrum's grid arrays on a device, a stream and the
// grow-on-demand workspace of the host-pointer calls (ctx_eval.hip) -- its life-cycle and settings, and the helpers that
// go with a context: device memory, HIP-event timers, in-run profiling.  No exception leaves this file.
#include "host_call.h"
#include "nmrfit_amd_diag.h"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <new>

namespace nmrfit {

int ensure(nmrfit_ctx *ctx, double **buf, int64_t *cap, int64_t need)
{
    if (need <= *cap) return NMRFIT_OK;
    // the old buffer may still be in use by work enqueued on the stream
    NMRFIT_HIP(hipStreamSynchronize(ctx->stream));
    if (*buf) NMRFIT_HIP(hipFree(*buf));
    *buf = nullptr;
    *cap = 0;
    int64_t n = need + need / 4 + 64;
    NMRFIT_HIP(device_alloc((void **)buf, (size_t)n * sizeof(double)));
    *cap = n;
    return NMRFIT_OK;
}

// What the kernels need to know about a grid besides its values: the centring offset, the span, and -- for the Gaussian
// recurrence -- whether it is uniformly spaced (np.linspace grids, ascending or descending) and how exactly.
void analyse_grid(const double *w, int64_t N, double *w0_out, double *wspan_out, double *lane_step_out, double *grid_dev_out)
{
    const double w0 = w[N / 2];
    double wspan = 0.0, lane_step = 0.0, grid_dev = 0.0;
    for (int64_t j = 0; j < N; ++j) wspan = std::fmax(wspan, std::fabs(w[j] - w0));
    // Measured on the centred values the kernel sees: deviation of every point from the straight line through the ends.
    if (N >= 2 * kChunk) {
        const double first = w[0] - w0, step = ((w[N - 1] - w0) - first) / (double)(N - 1);
        double dev = 0.0;
        for (int64_t j = 0; j < N; ++j) dev = std::fmax(dev, std::fabs((w[j] - w0) - (first + (double)j * step)));
        if (step != 0.0 && dev <= 1.0e-6 * std::fabs(step)) {   // NaN fails the test
            lane_step = step * kWave;
            grid_dev = 2.0 * dev;
        }
    }
    *w0_out = w0;
    *wspan_out = wspan;
    *lane_step_out = lane_step;
    *grid_dev_out = grid_dev;
}

// the kernel variants this library holds: every one in the A/B build, the selectable four in the product
// (3, 4 and 5 were A/B forms since retired: the numbers stay unused)
static bool variant_known(int variant)
{
    return variant == NMRFIT_VARIANT_DEFAULT || variant == NMRFIT_VARIANT_BASELINE || variant == NMRFIT_VARIANT_NOSKIP ||
           variant == NMRFIT_VARIANT_FARFIELD || variant == NMRFIT_VARIANT_NOREC || variant == NMRFIT_VARIANT_FARFIELD32;
}
static bool variant_built(int variant)
{
#ifdef NMRFIT_AB_BUILD
    return variant_known(variant);
#else
    return variant == NMRFIT_VARIANT_DEFAULT || variant == NMRFIT_VARIANT_FARFIELD || variant == NMRFIT_VARIANT_NOREC ||
           variant == NMRFIT_VARIANT_FARFIELD32;
#endif
}

}  // namespace nmrfit

using namespace nmrfit;

#pragma GCC visibility push(default)   // the C-ABI: the only symbols the library exports (build.sh: -fvisibility=hidden)
extern "C" {

int nmrfit_ctx_create(int device, int64_t N, const double *w, const double *u, const double *v,
                      const double *weights, nmrfit_ctx **out)
{
    if (!out) {
        set_error("null out pointer");
        return NMRFIT_E_INVALID;
    }
    *out = nullptr;
    if (N <= 0 || !w || !u || !v || !weights) {
        set_error("nmrfit_ctx_create: N must be > 0 and w, u, v, weights non-null");
        return NMRFIT_E_INVALID;
    }
    DeviceInfo prop;
    int rc = use_device(device, &prop);
    if (rc != NMRFIT_OK) return rc;
    nmrfit_ctx *ctx = new (std::nothrow) nmrfit_ctx();
    if (!ctx) {
        set_error("out of host memory");
        return NMRFIT_E_INVALID;
    }
    ctx->device = device;
    ctx->compute_units = prop.cus;
    ctx->N = N;
    ctx->n_chunks = block_plan(N).n_chunks;
    if (const char *tw = getenv("NMRFIT_TARGET_WAVES")) ctx->target_waves = atoll(tw);   // tuning knob
    if (getenv("NMRFIT_NO_WIDE_WORKGROUPS")) ctx->wide_workgroups = false;               // A/B knob
    if (const char *pw = getenv("NMRFIT_PAIR_WAVES")) ctx->pair_waves = atoi(pw) != 0 ? 1 : 0;   // A/B knob
    // test knob: run a whole test suite with another kernel variant as every context's default
    if (const char *dv = getenv("NMRFIT_DEFAULT_VARIANT")) {
        const int vnum = atoi(dv);
        if (variant_built(vnum)) ctx->variant = vnum;
    }
    analyse_grid(w, N, &ctx->w0, &ctx->wspan, &ctx->lane_step, &ctx->grid_dev);
    const size_t bytes = (size_t)N * sizeof(double);
    const size_t padded = (size_t)ctx->n_chunks * kChunk * sizeof(double);   // whole chunks, grid_slot order
    NMRFIT_HIP_OR(take_stream(device, &ctx->own_stream), nmrfit_ctx_destroy(ctx));
    ctx->stream = ctx->own_stream;
    NMRFIT_HIP_OR(hipEventCreate(&ctx->ev0), nmrfit_ctx_destroy(ctx));
    NMRFIT_HIP_OR(hipEventCreate(&ctx->ev1), nmrfit_ctx_destroy(ctx));
    // ONE allocation for the four padded grid arrays, the chunk table and the landing buffer (which first holds the raw w)
    Carver c;
    const size_t o_wc = c.take(padded), o_u = c.take(padded), o_v = c.take(padded), o_wt = c.take(padded);
    const size_t o_chunk = c.take((size_t)ctx->n_chunks * sizeof(double2)), o_stage = c.take(bytes);
    NMRFIT_HIP_OR(device_alloc((void **)&ctx->d_block, c.total), nmrfit_ctx_destroy(ctx));
    // (the four grid arrays: their padding is zeros, weight 0)
    NMRFIT_HIP_OR(hipMemsetAsync(ctx->d_block, 0, o_chunk, ctx->stream), nmrfit_ctx_destroy(ctx));
    unsigned char *base = reinterpret_cast<unsigned char *>(ctx->d_block);
    ctx->d_wc = reinterpret_cast<double *>(base + o_wc);
    ctx->d_u = reinterpret_cast<double *>(base + o_u);
    ctx->d_v = reinterpret_cast<double *>(base + o_v);
    ctx->d_wt = reinterpret_cast<double *>(base + o_wt);
    ctx->d_chunk = reinterpret_cast<double2 *>(base + o_chunk);
    ctx->d_stage = reinterpret_cast<double *>(base + o_stage);
    NMRFIT_HIP_OR(hipMemcpyAsync(ctx->d_stage, w, bytes, hipMemcpyHostToDevice, ctx->stream), nmrfit_ctx_destroy(ctx));
    rc = prepare_grid(ctx, ctx->d_stage);
    // u, v, weights: land in plain order, then into the pair-interleaved order the kernels read (nmrfit_internal.h,
    // grid_slot); stream order lets the one landing buffer serve all three
    const double *host_arrays[] = {u, v, weights};
    double *dev_arrays[] = {ctx->d_u, ctx->d_v, ctx->d_wt};
    for (int a = 0; a < 3 && rc == NMRFIT_OK; ++a) {
        NMRFIT_HIP_OR(hipMemcpyAsync(ctx->d_stage, host_arrays[a], bytes, hipMemcpyHostToDevice, ctx->stream),
                      nmrfit_ctx_destroy(ctx));
        rc = scatter_grid(ctx, ctx->d_stage, dev_arrays[a]);
    }
    if (rc != NMRFIT_OK) {
        nmrfit_ctx_destroy(ctx);
        return rc;
    }
    NMRFIT_HIP_OR(hipStreamSynchronize(ctx->stream), nmrfit_ctx_destroy(ctx));
    *out = ctx;
    return NMRFIT_OK;
}

int nmrfit_ctx_destroy(nmrfit_ctx *ctx)
{
    if (!ctx) return NMRFIT_OK;
    (void)hipSetDevice(ctx->device);
    if (ctx->own_stream) {
        (void)hipStreamSynchronize(ctx->stream);
        if (ctx->stream != ctx->own_stream) (void)hipStreamSynchronize(ctx->own_stream);
    }
    void *bufs[] = {ctx->d_block /* wc, u, v, weights, chunk table, landing buffer */, ctx->d_X, ctx->d_f, ctx->d_partial, ctx->d_R, ctx->d_lsq};
    for (void *b : bufs)
        if (b) (void)hipFree(b);
    if (ctx->ev0) (void)hipEventDestroy(ctx->ev0);
    if (ctx->ev1) (void)hipEventDestroy(ctx->ev1);
    (void)nmrfit_prof_enable(ctx, 0);
    if (ctx->own_stream) give_stream(ctx->device, ctx->own_stream);   // (synchronised above)
    delete ctx;
    return NMRFIT_OK;
}

int nmrfit_ctx_set_weights(nmrfit_ctx *ctx, const double *weights)
{
    int rc = bind(ctx);
    if (rc != NMRFIT_OK) return rc;
    if (!weights) {
        set_error("null weights");
        return NMRFIT_E_INVALID;
    }
    NMRFIT_HIP(hipMemcpyAsync(ctx->d_stage, weights, (size_t)ctx->N * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    rc = scatter_grid(ctx, ctx->d_stage, ctx->d_wt);
    if (rc != NMRFIT_OK) return rc;
    NMRFIT_HIP(hipStreamSynchronize(ctx->stream));
    return NMRFIT_OK;
}

int nmrfit_ctx_synchronize(nmrfit_ctx *ctx)
{
    int rc = bind(ctx);
    if (rc != NMRFIT_OK) return rc;
    NMRFIT_HIP(hipStreamSynchronize(ctx->stream));
    return NMRFIT_OK;
}

int nmrfit_ctx_set_stream(nmrfit_ctx *ctx, void *hip_stream)
{
    int rc = bind(ctx);
    if (rc != NMRFIT_OK) return rc;
    NMRFIT_HIP(hipStreamSynchronize(ctx->stream));   // drain work queued on the old stream
    ctx->stream = hip_stream ? (hipStream_t)hip_stream : ctx->own_stream;
    return NMRFIT_OK;
}

int nmrfit_ctx_set_variant(nmrfit_ctx *ctx, int variant)
{
    if (!ctx || !variant_known(variant)) {
        set_error("bad context or variant");
        return NMRFIT_E_INVALID;
    }
    if (!variant_built(variant))
        return refuse(NMRFIT_E_UNSUPPORTED,
                      "this kernel variant is an A/B form: it exists in libnmrfit_amd_ab.so (nmrfit_amd/csrc/build.sh --ab) only");
    ctx->variant = variant;
    return NMRFIT_OK;
}

int nmrfit_ctx_n(const nmrfit_ctx *ctx, int64_t *N)
{
    if (!ctx || !N) {
        set_error("null argument");
        return NMRFIT_E_INVALID;
    }
    *N = ctx->N;
    return NMRFIT_OK;
}

int nmrfit_ctx_set_fit_im(nmrfit_ctx *ctx, int fit_im)
{
    const int rc = check_fit_im(ctx ? fit_im : -1);   // (a missing context is refused in the same words)
    if (rc != NMRFIT_OK) return rc;
    ctx->fit_im = fit_im;
    return NMRFIT_OK;
}

int nmrfit_dev_alloc(nmrfit_ctx *ctx, int64_t bytes, void **dptr)
{
    int rc = bind(ctx);
    if (rc != NMRFIT_OK) return rc;
    if (!dptr || bytes < 0) {
        set_error("bad arguments to nmrfit_dev_alloc");
        return NMRFIT_E_INVALID;
    }
    *dptr = nullptr;
    if (bytes == 0) return NMRFIT_OK;
    NMRFIT_HIP(device_alloc(dptr, (size_t)bytes));
    return NMRFIT_OK;
}

int nmrfit_dev_free(nmrfit_ctx *ctx, void *dptr)
{
    int rc = bind(ctx);
    if (rc != NMRFIT_OK) return rc;
    if (!dptr) return NMRFIT_OK;
    NMRFIT_HIP(hipStreamSynchronize(ctx->stream));
    NMRFIT_HIP(hipFree(dptr));
    return NMRFIT_OK;
}

static int ctx_memcpy(nmrfit_ctx *ctx, const char *who, void *dst, const void *src, int64_t bytes, hipMemcpyKind kind)
{
    int rc = bind(ctx);
    if (rc != NMRFIT_OK) return rc;
    if (bytes < 0 || (bytes > 0 && (!dst || !src))) return refuse(NMRFIT_E_INVALID, std::string("bad arguments to ") + who);
    if (bytes == 0) return NMRFIT_OK;
    NMRFIT_HIP(hipMemcpyAsync(dst, src, (size_t)bytes, kind, ctx->stream));
    NMRFIT_HIP(hipStreamSynchronize(ctx->stream));
    return NMRFIT_OK;
}

int nmrfit_memcpy_h2d(nmrfit_ctx *ctx, void *dst_dev, const void *src_host, int64_t bytes)
{
    return ctx_memcpy(ctx, "nmrfit_memcpy_h2d", dst_dev, src_host, bytes, hipMemcpyHostToDevice);
}

int nmrfit_memcpy_d2h(nmrfit_ctx *ctx, void *dst_host, const void *src_dev, int64_t bytes)
{
    return ctx_memcpy(ctx, "nmrfit_memcpy_d2h", dst_host, src_dev, bytes, hipMemcpyDeviceToHost);
}

int nmrfit_timer_begin(nmrfit_ctx *ctx)
{
    int rc = bind(ctx);
    if (rc != NMRFIT_OK) return rc;
    NMRFIT_HIP(hipEventRecord(ctx->ev0, ctx->stream));
    return NMRFIT_OK;
}

int nmrfit_timer_end(nmrfit_ctx *ctx, double *elapsed_ms)
{
    int rc = bind(ctx);
    if (rc != NMRFIT_OK) return rc;
    if (!elapsed_ms) {
        set_error("null elapsed_ms");
        return NMRFIT_E_INVALID;
    }
    NMRFIT_HIP(hipEventRecord(ctx->ev1, ctx->stream));
    NMRFIT_HIP(hipEventSynchronize(ctx->ev1));
    float ms = 0.f;
    NMRFIT_HIP(hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1));
    *elapsed_ms = (double)ms;
    return NMRFIT_OK;
}

int nmrfit_prof_enable(nmrfit_ctx *ctx, int64_t capacity)
{
    int rc = bind(ctx);
    if (rc != NMRFIT_OK) return rc;
    if (capacity < 0 || capacity > (1 << 20)) {
        set_error("nmrfit_prof_enable: capacity must be 0..2^20");
        return NMRFIT_E_INVALID;
    }
    NMRFIT_HIP(hipStreamSynchronize(ctx->stream));
    for (auto *vec : {&ctx->prof_k0, &ctx->prof_k1, &ctx->prof_marks}) {
        for (hipEvent_t e : *vec) (void)hipEventDestroy(e);
        vec->clear();
    }
    ctx->prof_cap = 0;
    ctx->prof_nk = ctx->prof_nm = 0;
    if (capacity == 0) {
        if (ctx->d_clk) (void)hipFree(ctx->d_clk);
        ctx->d_clk = nullptr;
        return NMRFIT_OK;
    }
    if (!ctx->d_clk) {
#ifdef NMRFIT_DIAG_STAMPS   // diagnostic builds: room for 16 phase stamps of up to 1024 workgroups behind the clock ticks
        constexpr size_t kClkWords = 4 + 16 * 1024;
#else
        constexpr size_t kClkWords = 4;
#endif
        NMRFIT_HIP(device_alloc((void **)&ctx->d_clk, kClkWords * sizeof(unsigned long long)));
        NMRFIT_HIP(hipMemsetAsync(ctx->d_clk, 0, kClkWords * sizeof(unsigned long long), ctx->stream));
    }
    for (int64_t i = 0; i < capacity; ++i) {
        hipEvent_t a = nullptr, b = nullptr, c = nullptr;
        NMRFIT_HIP(hipEventCreate(&a));
        ctx->prof_k0.push_back(a);
        NMRFIT_HIP(hipEventCreate(&b));
        ctx->prof_k1.push_back(b);
        NMRFIT_HIP(hipEventCreate(&c));
        ctx->prof_marks.push_back(c);
    }
    // one more mark than steps: n steps are bracketed by n + 1 marks
    hipEvent_t last = nullptr;
    NMRFIT_HIP(hipEventCreate(&last));
    ctx->prof_marks.push_back(last);
    ctx->prof_cap = capacity;
    return NMRFIT_OK;
}

int nmrfit_prof_mark(nmrfit_ctx *ctx)
{
    int rc = bind(ctx);
    if (rc != NMRFIT_OK) return rc;
    if (ctx->prof_cap == 0) {
        set_error("nmrfit_prof_mark before nmrfit_prof_enable");
        return NMRFIT_E_STATE;
    }
    if (ctx->prof_nm > ctx->prof_cap) return NMRFIT_OK;   // full: later marks are dropped
    NMRFIT_HIP(hipEventRecord(ctx->prof_marks[(size_t)ctx->prof_nm], ctx->stream));
    ++ctx->prof_nm;
    return NMRFIT_OK;
}

int nmrfit_prof_read(nmrfit_ctx *ctx, double *kernel_ms, int64_t kernel_cap, int64_t *n_kernel, double *step_ms,
                     int64_t step_cap, int64_t *n_step, double *clock_mhz)
{
    int rc = bind(ctx);
    if (rc != NMRFIT_OK) return rc;
    if (kernel_cap < 0 || step_cap < 0 || (kernel_cap > 0 && !kernel_ms) || (step_cap > 0 && !step_ms)) {
        set_error("nmrfit_prof_read: bad arguments");
        return NMRFIT_E_INVALID;
    }
    NMRFIT_HIP(hipStreamSynchronize(ctx->stream));
    const int64_t nk = std::min<int64_t>(ctx->prof_nk, kernel_cap);
    for (int64_t i = 0; i < nk; ++i) {
        float ms = 0.f;
        NMRFIT_HIP(hipEventElapsedTime(&ms, ctx->prof_k0[(size_t)i], ctx->prof_k1[(size_t)i]));
        kernel_ms[i] = (double)ms;
    }
    const int64_t ns = std::min<int64_t>(std::max<int64_t>(ctx->prof_nm - 1, 0), step_cap);
    for (int64_t i = 0; i < ns; ++i) {
        float ms = 0.f;
        NMRFIT_HIP(hipEventElapsedTime(&ms, ctx->prof_marks[(size_t)i], ctx->prof_marks[(size_t)i + 1]));
        step_ms[i] = (double)ms;
    }
    if (n_kernel) *n_kernel = nk;
    if (n_step) *n_step = ns;
    if (clock_mhz) {
        *clock_mhz = 0.0;
        if (ctx->d_clk && ctx->prof_nk > 0) {
            unsigned long long t[4] = {0, 0, 0, 0};
            NMRFIT_HIP(hipMemcpy(t, ctx->d_clk, sizeof t, hipMemcpyDeviceToHost));
            if (t[3] > t[1] && t[2] > t[0]) *clock_mhz = 100.0 * (double)(t[2] - t[0]) / (double)(t[3] - t[1]);
        }
    }
    ctx->prof_nk = ctx->prof_nm = 0;   // reading rewinds
    return NMRFIT_OK;
}

int nmrfit_last_launch(const nmrfit_ctx *ctx, int64_t *waves, int32_t *segments, int64_t *segment_len)
{
    if (!ctx) {
        set_error("null context");
        return NMRFIT_E_INVALID;
    }
    if (waves) *waves = ctx->last.waves;
    if (segments) *segments = ctx->last.nseg;
    if (segment_len) *segment_len = ctx->last.seg_len;
    return NMRFIT_OK;
}

int nmrfit_last_launch_workgroup(const nmrfit_ctx *ctx, int32_t *waves_per_workgroup)
{
    if (!ctx) {
        set_error("null context");
        return NMRFIT_E_INVALID;
    }
    if (waves_per_workgroup) *waves_per_workgroup = ctx->last.waves_per_workgroup;
    return NMRFIT_OK;
}

#ifdef NMRFIT_DIAG_STAMPS
// diagnostic builds only (not in the header): the phase stamps of the last profiled launch, [workgroup][16]
int nmrfit_diag_read_stamps(nmrfit_ctx *ctx, unsigned long long *out, int64_t workgroups)
{
    if (!ctx || !ctx->d_clk || workgroups > 1024) return NMRFIT_E_INVALID;
    NMRFIT_HIP(hipStreamSynchronize(ctx->stream));
    NMRFIT_HIP(hipMemcpy(out, ctx->d_clk + 4, (size_t)workgroups * 16 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    return NMRFIT_OK;
}
#endif

}  // extern "C"
#pragma GCC visibility pop

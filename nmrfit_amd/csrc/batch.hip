// batch.hip -- device-batched fits: K independent nmrfit fits advanced together, ONE kernel launch per swarm generation
// for all of them (the nmrfit_batch_* entry points of include/nmrfit_amd.h).
//
// The reference's users call `nmrfit.fit` once per spectrum (nmrfit/core.py:64, README.md:64-66), each with a
// 204-particle swarm (nmrfit/utils.py:177).  A lone swarm of that size occupies a fraction of an MI355X and its
// generation is one wave's critical path (11.7 us for ~0.9 us of throughput-bound work); host threads driving one
// context each saturate at ~95 fits/s.  Here the K spectra are prepared into ONE device allocation, the K swarms live
// next to them, and a generation of every swarm is one launch of the objective kernel whose workgroups find their fit's
// record (BatchFit) from blockIdx (objective_batch.hip).  Each fit keeps its own (g, fg), stop flags and random stream
// (Philox keyed by its seed), runs exactly the operations a lone `nmrfit_amd.fit` runs in the same order, and stops by
// its own pyswarm rule: the K results are bit-identical to K lone fits.
//
// State machine (the deferred fold of pso.hip, for K swarms in lock step): after generation 0 every launch moves, evaluates
// and personal-bests every particle and leaves its generation to be folded by the NEXT launch's prologue; x / v and
// (p, fp) ping-pong every launch, the (g, fg | flags) blocks whenever a launch folded.  The kernel reads which buffer is
// which from one of 8 + 1 descriptor tables built once at creation (phase of x / p, phase of the state block, fold
// pending or not; + plain evaluation), so a generation costs the host one launch and no copies.
//
// This unit: the batch's own four kernels, the launch geometries of a part, the generation state machine and its
// entry points (step, run, status, best, geometry, synchronize, get_state).  Creation is batch_create.hip, least squares
// batch_lsq.hip, reconstruction / noise / spectra batch_data.hip; what they share is batch_part.h.
#include "batch_part.h"
#include "nmrfit_amd_diag.h"

#include <algorithm>
#include <cstdlib>
#include <string>
#include <vector>

namespace nmrfit {
namespace {

#pragma clang fp contract(off)

struct PrepareArgs {
    int64_t plane;           // doubles per uploaded array (the sum of the fits' lengths)
    const double *raw;       // [4][plane]: w, u, v, weights as uploaded, fit after fit
    const BatchFit *fits;    // any table: wc, u, v, wt, chunk, w0, N, raw_off
};

// centred grid + scatter of the four arrays into the pair-interleaved order the kernels read (nmrfit_internal.h,
// grid_slot), for every fit of the batch at once (blockIdx.y = the fit); the padding up to whole chunks was zeroed before
__global__ void batch_prepare_kernel(PrepareArgs a)
{
    const BatchFit &f = a.fits[blockIdx.y];
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= f.N) return;
    const int64_t idx = f.raw_off + j;
    const int64_t slot = grid_slot(j);
    const_cast<double *>(f.wc)[slot] = a.raw[idx] - f.w0;
    const_cast<double *>(f.u)[slot] = a.raw[a.plane + idx];
    const_cast<double *>(f.v)[slot] = a.raw[2 * a.plane + idx];
    const_cast<double *>(f.wt)[slot] = a.raw[3 * a.plane + idx];
}

// per-chunk (min, max) of every fit's centred grid: one wave per (fit, chunk)
__global__ void batch_chunk_minmax_kernel(PrepareArgs a)
{
    const BatchFit &f = a.fits[blockIdx.y];
    const int64_t c = (int64_t)blockIdx.x * (blockDim.x / kWave) + (threadIdx.x >> 6);
    if (c * kChunk < f.N) chunk_minmax_wave(f.wc, f.N, c, threadIdx.x & (kWave - 1), const_cast<double2 *>(f.chunk));
}

// generation 0 of every swarm: x ~ U(lb, ub), v ~ U(-|ub - lb|, |ub - lb|), p = 0, fp = +inf (pso.hip, pso_init_kernel)
__global__ void batch_init_kernel(const BatchFit *__restrict__ fits, int64_t Dmax)
{
    const BatchFit &f = fits[blockIdx.y];
    const int64_t S = f.S;
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= S * Dmax) return;
    const int64_t i = r / Dmax;
    const int d = (int)(r - i * Dmax);
    const int64_t D = 4 + 3 * (int64_t)f.P;
    if (d >= D) return;
    const PsoFused &u = f.upd;
    double r0, r1;
    uniform2(u.seed, 0u, (uint32_t)d, (uint64_t)i, &r0, &r1);
    const double lo = u.lb[d], hi = u.ub[d];
    const double vhigh = fabs(hi - lo), vlow = -vhigh;
    const int64_t e = i * D + d;
    const_cast<double *>(u.x_in)[e] = lo + r0 * (hi - lo);
    const_cast<double *>(u.v_in)[e] = vlow + r1 * (vhigh - vlow);
    double *p = const_cast<double *>(u.p);
    p[e] = 0.0;
    if (d == 0) p[S * D + i] = INFINITY;
    if (r == 0) {
        const_cast<long long *>(u.flags)[0] = 0;
        const_cast<long long *>(u.flags)[1] = 0;
    }
}

enum { kBatchPbest = 1, kBatchArgmin = 2, kBatchApply = 4 };

// One workgroup per fit: what follows an objective launch that did not finish the generation itself -- personal bests
// (generation 0), argmin over fp -> candidate record, fold with pyswarm's rule -- and the fit's line of the summary
// the host reads (generations, stop code, fg, best value, best position).  Same device bodies as pso_tail_kernel.
__global__ __launch_bounds__(1024) void batch_tail_kernel(const BatchFit *__restrict__ fits, int phases, int is_init,
                                                          double *__restrict__ summary, double *__restrict__ bestx,
                                                          const int64_t *__restrict__ boff)
{
    const BatchFit &f = fits[blockIdx.x];
    const PsoFused &u = f.upd;
    const int64_t D = 4 + 3 * (int64_t)f.P, S = f.S;
    long long *flags = const_cast<long long *>(u.flags);
    double *best = const_cast<double *>(u.best);
    double *p = const_cast<double *>(u.p), *fp = p + S * D;
    __shared__ double s_val[16];
    __shared__ long long s_idx[16];
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6, nw = blockDim.x / kWave;
    if (flags[1] == 0) {   // (after a stop nothing moves: pso_tail_kernel returns at once)
        if (phases & kBatchPbest) {
            for (int64_t i = wave; i < S; i += nw) pbest_particle(i, lane, D, u.x_in, f.fx, p, fp);
            __syncthreads();
        }
        if (phases & kBatchArgmin) {
            argmin_block(S, D, fp, p, u.x_in, u.cand, s_val, s_idx);
            __syncthreads();
        }
        if (phases & kBatchApply) {
            if (wave == 0) apply_wave(lane, D, 1, is_init, u.minstep, u.minfunc, u.cand, flags, best);
            __syncthreads();
        }
    }
    if (threadIdx.x == 0) {
        double *s = summary + 4 * (int64_t)blockIdx.x;
        s[0] = (double)flags[0];
        s[1] = (double)flags[1];
        s[2] = best[0];
        s[3] = best[1];
    }
    for (int64_t d = threadIdx.x; d < D; d += blockDim.x) bestx[boff[blockIdx.x] + d] = best[2 + D + d];
}

int launch_generation(const BatchLaunch &g) { return g.fit_im ? launch_objective_batch_im(g) : launch_objective_batch(g); }

const BatchFit *table(const BatchPart *b, int t) { return b->d_tables + (size_t)t * (size_t)b->K; }

int launch_tail(BatchPart *b, int phases, int is_init)
{
    // the table of the CURRENT phases: x_in / p are the buffers the last launch wrote, best / flags the current block
    const BatchFit *t = table(b, b->xp + 2 * b->b);
    hipLaunchKernelGGL(batch_tail_kernel, dim3((unsigned)b->K), dim3(1024), 0, b->stream, t, phases, is_init,
                       b->d_summary, b->d_bestx, reinterpret_cast<const int64_t *>(b->d_bestx + b->Dsum));
    NMRFIT_HIP(hipGetLastError());
    return NMRFIT_OK;
}

}  // namespace

// ---- the two launch geometries of a part (objective.hip's launch_objective picks among the same forms for a lone swarm)

// the row copies a workgroup keeps in LDS behind the kernel's records: three rows of ONE particle (workgroup = particle),
// or per wave three rows and two doubles (wave = particle)
static size_t row_copy_bytes(bool wave_swarm, int32_t Pmax)
{
    const size_t Dmax = 4 + 3 * (size_t)Pmax;
    return (wave_swarm ? (size_t)kWavesPerBlock * (3 * Dmax + 2) : 3 * Dmax) * sizeof(double);
}

void plan_geometry(BatchPart *b)
{
    // (ragged batches: the wave = particle form takes every fit's grid from its record; the launch record then carries
    // the longest grid's figures, which that kernel does not read)
    const int64_t N = b->N ? b->N : b->Nmax;
    const BlockPlan bp = block_plan(N);
    const int64_t n_blocks = bp.n_blocks, blk_len = bp.blk_len;
    for (int m = 0; m < 2; ++m) {
        BatchLaunch &g = b->geom[m];
        g = BatchLaunch{};
        g.stream = b->stream;
        g.K = b->K;
        g.S = b->Smax;
        g.N = N;
        g.blk_chunks = bp.blk_chunks;
        g.n_blocks = (int)n_blocks;
        g.variant = b->variant;
        g.fit_im = b->fit_im;
        b->geom_ok[m] = false;
        int slices, rows;
        if (m == 0) {
            // workgroup = particle: eight segments (an eight-wave workgroup) when the grid cuts into exactly eight, else
            // four; the deferred fold's argmin covers kDeferredPerLane x 64 entries per wave (pso_update.h)
            int wpb = 0;
            int64_t seg_len = 0;
            for (int w : {kWideWaves, kWavesPerBlock}) {
                if (b->fit_im != NMRFIT_FIT_IM_OFF) continue;   // (the imaginary channel: wave = particle only)
                if (b->N == 0 || b->S == 0) continue;           // (fits of different lengths or swarm sizes: wave = particle only)
                if (n_blocks < w) continue;
                const int64_t sl = ((n_blocks + w - 1) / w) * blk_len;
                if ((N + sl - 1) / sl != w) continue;
                if (b->S > (int64_t)kDeferredPerLane * kWave * w) continue;
                wpb = w;
                seg_len = sl;
                break;
            }
            if (!wpb) continue;
            g.wpb = wpb;
            g.nseg = wpb;
            g.seg_len = seg_len;
            g.seg_blocks = (int)(seg_len / blk_len);
            g.wave_swarm = false;
            g.blocks_per_fit = b->S;
            slices = 1;
            rows = 3;
        } else {
            // wave = particle: one segment, four particles per workgroup (the last workgroup of a fit padded with idle waves,
            // so that a workgroup never spans two fits)
            g.wpb = kWavesPerBlock;
            g.nseg = 1;
            g.seg_len = n_blocks * blk_len;
            g.seg_blocks = (int)n_blocks;
            g.wave_swarm = true;
            g.blocks_per_fit = (b->Smax + kWavesPerBlock - 1) / kWavesPerBlock;
            slices = kWavesPerBlock;
            rows = 14;   // >= 4 x (3 D + 2) doubles for every D >= 4
        }
        int v = b->variant;
        unsigned aux = 0;
        size_t lds = objective_lds(b->variant, b->Pmax, false, b->fit_im, &v, &aux, g.wpb, slices, rows);
        if (v != b->variant) continue;   // (would run another kernel than a lone fit: not bit-identical)
        lds = (lds + 15) & ~(size_t)15;   // the row copies come last (their offset, xrow_offset below, travels in the
        lds += row_copy_bytes(g.wave_swarm, b->Pmax);   // descriptor tables: PsoFused::xrow_off, re-stamped when the geometry changes)
        if (!lds_fits(lds, kObjectiveStaticLds)) continue;
        g.lds = lds;
        g.aux_off = aux;
        b->geom_ok[m] = true;
    }
    // The geometry a new part starts in: the wave form for many particles (one prologue per particle instead of one per
    // workgroup of idle waves).  Measured on 204 x 4096 x 6 fits (profiles/r05/batch_fits_small_k.txt): the workgroup
    // form costs ~9 us per fit and generation whatever K (two fits: 20.1 us), the wave form 25 us per generation up to a
    // wave per SIMD and ~9 us per further wave per SIMD (three fits: 25.4, eight: 32.1) -- they cross between two and
    // three fits.  Longer grids have longer waves: there the wave form waits until every SIMD has one.
    // NMRFIT_BATCH_WAVE_MIN overrides.
    b->mode = b->geom_ok[0] ? 0 : 1;
    int64_t wave_min = (b->n_chunks <= 16) ? 512 : 1024;
    if (const char *e = getenv("NMRFIT_BATCH_WAVE_MIN")) wave_min = atoll(e);
    if (b->geom_ok[1] && b->Ssum >= wave_min) b->mode = 1;
}

unsigned xrow_offset(const BatchPart *b, int m)
{
    const BatchLaunch &g = b->geom[m];
    return (unsigned)(g.lds - row_copy_bytes(g.wave_swarm, b->Pmax));
}

// creation's two launches over the uploaded planes (d_raw: [4][sum of the fits' lengths]): the scatter, the chunk tables
int launch_prepare(BatchPart *b, const double *d_raw)
{
    PrepareArgs a{};
    a.plane = b->noff[(size_t)b->K];
    a.raw = d_raw;
    a.fits = b->d_tables;
    hipLaunchKernelGGL(batch_prepare_kernel, dim3((unsigned)((b->Nmax + 255) / 256), (unsigned)b->K), dim3(256), 0, b->stream, a);
    NMRFIT_HIP(hipGetLastError());
    hipLaunchKernelGGL(batch_chunk_minmax_kernel, dim3((unsigned)((b->n_chunks + 3) / 4), (unsigned)b->K), dim3(kWave * 4), 0, b->stream, a);
    NMRFIT_HIP(hipGetLastError());
    return NMRFIT_OK;
}

// ---- what the entry points of every unit begin with (batch_part.h) ----

int bind_batch(const BatchPart *b)
{
    if (!b) return refuse(NMRFIT_E_INVALID, "null batch handle");
    NMRFIT_HIP(hipSetDevice(b->device));
    return NMRFIT_OK;
}

int bind_started(BatchPart *b, const char *who)
{
    const int rc = bind_batch(b);
    if (rc != NMRFIT_OK) return rc;
    if (!b->initialized) return refuse(NMRFIT_E_STATE, std::string(who) + " before the first generation");
    return NMRFIT_OK;
}

// fold the generation whose personal bests are still waiting, in a launch of its own (pso.hip, flush_fold)
int flush_fold(BatchPart *b)
{
    if (!b->fold_pending) return NMRFIT_OK;
    const int rc = launch_tail(b, kBatchArgmin | kBatchApply, 0);
    if (rc == NMRFIT_OK) b->fold_pending = false;
    return rc;
}

int check_batch_handle(const nmrfit_batch *b)
{
    if (!b || b->parts.empty()) return refuse(NMRFIT_E_INVALID, "null batch handle");
    NMRFIT_HIP(hipSetDevice(b->device));
    return NMRFIT_OK;
}

int part_of(const nmrfit_batch *b, int32_t k)
{
    int p = 0;
    while (p + 1 < (int)b->parts.size() && k >= b->first[(size_t)p + 1]) ++p;
    return p;
}

int check_idle(const nmrfit_batch *b, const char *who)
{
    for (const BatchPart *q : b->parts)
        if (q->d_result) return refuse(NMRFIT_E_STATE, std::string(who) + ": a reconstruction of this batch is still in flight");
    return NMRFIT_OK;
}

}  // namespace nmrfit

using namespace nmrfit;

// generation 0: positions, velocities, evaluation, personal bests, (g, fg) <- the best of them
static int batch_init(BatchPart *b)
{
    b->xp = b->b = 0;
    b->fold_pending = false;
    const int64_t Dmax = 4 + 3 * (int64_t)b->Pmax;
    const int64_t n = b->Smax * Dmax;
    hipLaunchKernelGGL(batch_init_kernel, dim3((unsigned)((n + 255) / 256), (unsigned)b->K), dim3(256), 0, b->stream, table(b, 0), Dmax);
    NMRFIT_HIP(hipGetLastError());
    BatchLaunch g = b->geom[b->mode];
    g.fits = table(b, 8);
    int rc = launch_generation(g);
    if (rc != NMRFIT_OK) return rc;
    if ((rc = launch_tail(b, kBatchPbest | kBatchArgmin | kBatchApply, 1)) != NMRFIT_OK) return rc;
    b->initialized = true;
    return NMRFIT_OK;
}

// one generation of every swarm that has not stopped: ONE launch
static int batch_generation(BatchPart *b)
{
    BatchLaunch g = b->geom[b->mode];
    g.fits = table(b, b->xp + 2 * b->b + (b->fold_pending ? 4 : 0));
    const int rc = launch_generation(g);
    if (rc != NMRFIT_OK) return rc;
    b->xp ^= 1;                          // x / v and (p, fp): the buffers the launch has just written
    if (b->fold_pending) b->b ^= 1;      // it folded the generation before: particle 0 wrote the other state block
    b->fold_pending = true;              // its own generation waits for the next launch (or flush_fold)
    ++b->launches;
    return NMRFIT_OK;
}

static int part_step(BatchPart *b)
{
    int rc = bind_batch(b);
    if (rc != NMRFIT_OK) return rc;
    if (!b->initialized) return batch_init(b);
    return batch_generation(b);
}

static int read_summary(BatchPart *b, std::vector<double> &s)
{
    int rc = flush_fold(b);
    if (rc != NMRFIT_OK) return rc;
    s.resize((size_t)b->K * 4);
    NMRFIT_HIP(hipMemcpyAsync(s.data(), b->d_summary, s.size() * sizeof(double), hipMemcpyDeviceToHost, b->stream));
    NMRFIT_HIP(hipStreamSynchronize(b->stream));
    return NMRFIT_OK;
}

static int part_status(BatchPart *b, int64_t *iteration, int32_t *stop_code, double *fg)
{
    int rc = bind_started(b, "nmrfit_batch_status");
    if (rc != NMRFIT_OK) return rc;
    std::vector<double> s;
    if ((rc = read_summary(b, s)) != NMRFIT_OK) return rc;
    for (int32_t k = 0; k < b->K; ++k) {
        if (iteration) iteration[k] = (int64_t)s[(size_t)k * 4];
        if (stop_code) stop_code[k] = (int32_t)s[(size_t)k * 4 + 1];
        if (fg) fg[k] = s[(size_t)k * 4 + 2];
    }
    return NMRFIT_OK;
}

static int part_best(BatchPart *b, double *x_best, double *f_best)
{
    int rc = bind_started(b, "nmrfit_batch_best");
    if (rc != NMRFIT_OK) return rc;
    std::vector<double> s;
    if ((rc = read_summary(b, s)) != NMRFIT_OK) return rc;
    if (f_best)
        for (int32_t k = 0; k < b->K; ++k) f_best[k] = s[(size_t)k * 4 + 3];
    if (x_best) {
        NMRFIT_HIP(hipMemcpyAsync(x_best, b->d_bestx, (size_t)b->Dsum * sizeof(double), hipMemcpyDeviceToHost, b->stream));
        NMRFIT_HIP(hipStreamSynchronize(b->stream));
    }
    return NMRFIT_OK;
}


static bool part_allows_geometry(const BatchPart *b, int mode)
{
    return mode >= 0 && mode <= 1 && b->geom_ok[mode];
}

static int refuse_geometry()
{
    set_error("nmrfit_batch_set_geometry: 0 (workgroup = particle) or 1 (wave = particle), where the shape allows it");
    return NMRFIT_E_UNSUPPORTED;
}

static int part_set_geometry(BatchPart *b, int mode)
{
    int rc = bind_batch(b);
    if (rc != NMRFIT_OK) return rc;
    if (!part_allows_geometry(b, mode)) return refuse_geometry();
    if (mode == b->mode) return NMRFIT_OK;
    if ((rc = flush_fold(b)) != NMRFIT_OK) return rc;
    NMRFIT_HIP(hipStreamSynchronize(b->stream));
    // the row copies sit elsewhere in LDS: re-stamp the offset in the eight fused tables
    std::vector<BatchFit> tabs((size_t)8 * (size_t)b->K);
    NMRFIT_HIP(hipMemcpy(tabs.data(), b->d_tables, tabs.size() * sizeof(BatchFit), hipMemcpyDeviceToHost));
    for (BatchFit &f : tabs) f.upd.xrow_off = xrow_offset(b, mode);
    NMRFIT_HIP(hipMemcpy(b->d_tables, tabs.data(), tabs.size() * sizeof(BatchFit), hipMemcpyHostToDevice));
    b->mode = mode;
    return NMRFIT_OK;
}

static int part_geometry(const BatchPart *b, int32_t *mode, int32_t *waves_per_workgroup, int32_t *segments, int64_t *workgroups)
{
    if (!b) return refuse(NMRFIT_E_INVALID, "null batch handle");
    const BatchLaunch &g = b->geom[b->mode];
    if (mode) *mode = b->mode;
    if (waves_per_workgroup) *waves_per_workgroup = g.wpb;
    if (segments) *segments = g.nseg;
    if (workgroups) *workgroups = g.blocks_per_fit * b->K;
    return NMRFIT_OK;
}

static int part_synchronize(BatchPart *b)
{
    int rc = bind_batch(b);
    if (rc != NMRFIT_OK) return rc;
    NMRFIT_HIP(hipStreamSynchronize(b->stream));
    return NMRFIT_OK;
}

// swarm state of fit k (any pointer may be NULL): x, v, p are S x D_k; fx, fp are S
static int part_get_state(BatchPart *b, int32_t k, double *x, double *v, double *p, double *fx, double *fp)
{
    int rc = bind_batch(b);
    if (rc != NMRFIT_OK) return rc;
    if (k < 0 || k >= b->K) return refuse(NMRFIT_E_INVALID, "nmrfit_batch_get_state: fit index out of range");
    if (!b->initialized) return refuse(NMRFIT_E_STATE, "nmrfit_batch_get_state before the first generation");
    if ((rc = flush_fold(b)) != NMRFIT_OK) return rc;
    BatchFit f;
    NMRFIT_HIP(hipMemcpy(&f, table(b, b->xp + 2 * b->b) + k, sizeof f, hipMemcpyDeviceToHost));
    const int64_t S = b->Sk[(size_t)k];
    const size_t sd = (size_t)(S * b->D[(size_t)k]) * sizeof(double), s1 = (size_t)S * sizeof(double);
    hipStream_t st = b->stream;
    if (x) NMRFIT_HIP(hipMemcpyAsync(x, f.upd.x_in, sd, hipMemcpyDeviceToHost, st));
    if (v) NMRFIT_HIP(hipMemcpyAsync(v, f.upd.v_in, sd, hipMemcpyDeviceToHost, st));
    if (p) NMRFIT_HIP(hipMemcpyAsync(p, f.upd.p, sd, hipMemcpyDeviceToHost, st));
    if (fx) NMRFIT_HIP(hipMemcpyAsync(fx, f.fx, s1, hipMemcpyDeviceToHost, st));
    if (fp) NMRFIT_HIP(hipMemcpyAsync(fp, f.upd.p + S * b->D[(size_t)k], s1, hipMemcpyDeviceToHost, st));
    NMRFIT_HIP(hipStreamSynchronize(st));
    return NMRFIT_OK;
}

#pragma GCC visibility push(default)   // the C-ABI: the only symbols the library exports (build.sh: -fvisibility=hidden)
extern "C" {

int nmrfit_batch_step(nmrfit_batch *b)
{
    int rc = check_batch_handle(b);
    for (size_t p = 0; rc == NMRFIT_OK && p < b->parts.size(); ++p) rc = part_step(b->parts[p]);
    return rc;
}

int nmrfit_batch_run(nmrfit_batch *b, int64_t maxiter, int32_t check_every)
{
    int rc = check_batch_handle(b);
    if (rc != NMRFIT_OK) return rc;
    if (maxiter < 0 || check_every < 1)
        return refuse(NMRFIT_E_INVALID, "nmrfit_batch_run: maxiter must be >= 0 and check_every >= 1");
    for (BatchPart *p : b->parts)
        if (!p->initialized && (rc = batch_init(p)) != NMRFIT_OK) return rc;
    // every fit runs the generations a lone nmrfit_pso_run would: a stopped swarm's waves return at once, so the others'
    // generations do not touch it; a part leaves the loop when every one of its swarms has stopped (polled every
    // check_every).  The parts' launches are interleaved on their own streams.
    std::vector<char> done(b->parts.size(), 0);
    std::vector<double> s;
    for (int64_t it = 1; it <= maxiter; ++it) {
        bool any = false;
        for (size_t p = 0; p < b->parts.size(); ++p) {
            if (done[p]) continue;
            any = true;
            if ((rc = batch_generation(b->parts[p])) != NMRFIT_OK) return rc;
        }
        if (!any) break;
        if (it % check_every == 0 || it == maxiter) {
            for (size_t p = 0; p < b->parts.size(); ++p) {
                if (done[p]) continue;
                if ((rc = read_summary(b->parts[p], s)) != NMRFIT_OK) return rc;
                bool all = true;
                for (int32_t k = 0; k < b->parts[p]->K; ++k) all = all && s[(size_t)k * 4 + 1] != 0.0;
                done[p] = all ? 1 : 0;
            }
        }
    }
    return NMRFIT_OK;
}

int nmrfit_batch_status(nmrfit_batch *b, int64_t *iteration, int32_t *stop_code, double *fg)
{
    int rc = check_batch_handle(b);
    for (size_t p = 0; rc == NMRFIT_OK && p < b->parts.size(); ++p) {
        const int32_t f0 = b->first[p];
        rc = part_status(b->parts[p], iteration ? iteration + f0 : nullptr, stop_code ? stop_code + f0 : nullptr,
                         fg ? fg + f0 : nullptr);
    }
    return rc;
}

int nmrfit_batch_best(nmrfit_batch *b, double *x_best, double *f_best)
{
    int rc = check_batch_handle(b);
    for (size_t p = 0; rc == NMRFIT_OK && p < b->parts.size(); ++p) {
        const int32_t f0 = b->first[p];
        rc = part_best(b->parts[p], x_best ? x_best + b->boff[(size_t)f0] : nullptr, f_best ? f_best + f0 : nullptr);
    }
    return rc;
}

/* ---- diagnostics (include/nmrfit_amd_diag.h) ---- */

int nmrfit_batch_set_geometry(nmrfit_batch *b, int mode)
{
    int rc = check_batch_handle(b);
    if (rc != NMRFIT_OK) return rc;
    // all or nothing: a form that one part's shapes do not allow is refused before any part has changed
    for (const BatchPart *q : b->parts)
        if (!part_allows_geometry(q, mode)) return refuse_geometry();
    for (size_t p = 0; rc == NMRFIT_OK && p < b->parts.size(); ++p) rc = part_set_geometry(b->parts[p], mode);
    return rc;
}

int nmrfit_batch_geometry(const nmrfit_batch *b, int32_t *mode, int32_t *waves_per_workgroup, int32_t *segments, int64_t *workgroups)
{
    if (!b || b->parts.empty()) return refuse(NMRFIT_E_INVALID, "null batch handle");
    int64_t total = 0;
    for (size_t p = 0; p < b->parts.size(); ++p) {   // (mode, waves and segments of the first part; workgroups of all)
        int64_t n = 0;
        const int rc = part_geometry(b->parts[p], p == 0 ? mode : nullptr, p == 0 ? waves_per_workgroup : nullptr,
                                     p == 0 ? segments : nullptr, &n);
        if (rc != NMRFIT_OK) return rc;
        total += n;
    }
    if (workgroups) *workgroups = total;
    return NMRFIT_OK;
}

int nmrfit_batch_synchronize(nmrfit_batch *b)
{
    int rc = check_batch_handle(b);
    for (size_t p = 0; rc == NMRFIT_OK && p < b->parts.size(); ++p) rc = part_synchronize(b->parts[p]);
    return rc;
}

int nmrfit_batch_get_state(nmrfit_batch *b, int32_t k, double *x, double *v, double *p, double *fx, double *fp)
{
    int rc = check_batch_handle(b);
    if (rc != NMRFIT_OK) return rc;
    if (k < 0 || k >= b->K) return refuse(NMRFIT_E_INVALID, "nmrfit_batch_get_state: fit index out of range");
    const int q = part_of(b, k);
    return part_get_state(b->parts[(size_t)q], k - b->first[(size_t)q], x, v, p, fx, fp);
}

}  // extern "C"
#pragma GCC visibility pop

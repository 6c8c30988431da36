// batch_create.hip -- creation and destruction of a device batch (nmrfit_batch_create*, nmrfit_batch_destroy): a part's
// fits are checked and described on the host, its launch geometry planned (batch.hip), its ONE device allocation laid out
// once -- the same record carves the allocation and forms the pointers of the descriptor tables -- and the spectra
// uploaded and prepared on the part's stream; the batch divides its fits over one or two parts.
#include "batch_part.h"
#include "nmrfit_amd_prep.h"
#include "weights_internal.h"

#include <algorithm>
#include <new>
#include <string>
#include <vector>

namespace nmrfit {
namespace {

// ---- one part of a batch: a set of fits advanced by one launch per generation on one stream ----------------
// part_create: check the arguments, describe the fits on the host, plan the geometry, lay the one allocation out, build
// the descriptor tables from the layout, then upload and prepare the spectra.

const char kCreateArgs[] = "nmrfit_batch_create: K, N, swarmsize must be > 0 and every array non-null";

// what part_create refuses before it touches the device
int check_part_args(int32_t K, const int64_t *Nk, const double *w, const double *u, const double *v, const double *weights,
                    const int32_t *R, const int32_t *P, const double *lower, const double *upper, const int64_t *swarm,
                    const nmrfit_pso_params *params, int variant, int fit_im)
{
    if (K <= 0 || !Nk || !swarm || !w || !u || !v || (!weights && !R) || !P || !lower || !upper || !params)
        return refuse(NMRFIT_E_INVALID, kCreateArgs);
    for (int32_t k = 0; k < K; ++k)
        if (Nk[k] <= 0 || swarm[k] <= 0 || swarm[k] > 0x7fffffffLL / 8)
            return refuse(NMRFIT_E_INVALID,
                          "nmrfit_batch_create: every grid length and swarm size must be > 0 (and a swarm below 2^28 particles)");
    if (variant != NMRFIT_VARIANT_DEFAULT && variant != NMRFIT_VARIANT_FARFIELD)
        return refuse(NMRFIT_E_UNSUPPORTED, "nmrfit_batch_create: device-batched fits run the DEFAULT and FARFIELD kernels");
    if (fit_im < 0 || fit_im > NMRFIT_FIT_IM_SUM)
        return refuse(NMRFIT_E_INVALID, "fit_im must be 0 (real part), 1 (reference fit_im=True) or 2 (all-peak imaginary model)");
    if (K > 65535) return refuse(NMRFIT_E_INVALID, "nmrfit_batch_create: more than 65535 fits in one part");
    return NMRFIT_OK;
}

// the host-side description of the part's fits: lengths, swarm sizes, peak counts, and their offsets in the caller's arrays
int describe_fits(BatchPart *b, const int64_t *Nk, const int64_t *swarm, const int32_t *P, const double *lower, const double *upper)
{
    const int32_t K = b->K;
    b->Nk.assign(Nk, Nk + K);
    b->noff.resize((size_t)K + 1);
    b->noff[0] = 0;
    b->N = Nk[0];
    for (int32_t k = 0; k < K; ++k) {
        b->noff[(size_t)k + 1] = b->noff[(size_t)k] + Nk[k];
        b->Nmax = std::max(b->Nmax, Nk[k]);
        if (Nk[k] != Nk[0]) b->N = 0;   // ragged
    }
    b->Sk.assign(swarm, swarm + K);
    b->S = swarm[0];
    for (int32_t k = 0; k < K; ++k) {
        b->Smax = std::max(b->Smax, swarm[k]);
        b->Ssum += swarm[k];
        if (swarm[k] != swarm[0]) b->S = 0;   // swarms of different sizes
    }
    b->n_chunks = block_plan(b->Nmax).n_chunks;
    b->P.assign(P, P + K);
    b->D.resize((size_t)K);
    b->boff.resize((size_t)K);
    for (int32_t k = 0; k < K; ++k) {
        if (P[k] < 0 || 4 + 3 * (int64_t)P[k] > kFusedMaxD)
            return refuse(NMRFIT_E_INVALID, "nmrfit_batch_create: peak counts must be 0 <= P and 4 + 3 P <= " + std::to_string(kFusedMaxD));
        b->D[(size_t)k] = 4 + 3 * (int64_t)P[k];
        b->boff[(size_t)k] = b->Dsum;
        b->Dsum += b->D[(size_t)k];
        b->Pmax = std::max(b->Pmax, P[k]);
        b->Psum += P[k];
    }
    for (int64_t d = 0; d < b->Dsum; ++d)
        if (!(upper[d] > lower[d]))   // pyswarm: assert np.all(ub > lb)
            return refuse(NMRFIT_E_INVALID, "All upper-bound values must be greater than lower-bound values");
    return NMRFIT_OK;
}

// Where a fit's arrays lie in the part's one allocation: the byte offset of each piece and, for those that come in several
// copies, the aligned size of one.  Computed once (lay_out): the allocation is carved and the descriptor tables' pointers
// are formed from the same numbers.
struct FitLayout {
    size_t grid, grid_bytes;     // wc, u, v, wt: four padded arrays (whole chunks, grid_slot order)
    size_t chunk;                // the chunk table
    size_t xv, xv_bytes;         // x, v and the buffers they ping-pong with, x', v': four arrays [S x D]
    size_t p, p_bytes;           // (p [S x D], fp [S]) twice
    size_t fx, cand;             // fx [S]; the candidate record [D + 1]
    size_t state, state_bytes;   // the state block twice (host_call.h, swarm_state_bytes)
};
// ... and the part's own pieces behind them: the K boxes, concatenated like the caller's arrays (two uploads for the whole
// part: they were 2 K small ones, ~8 us each); the summary, the best rows (+ their offsets), the descriptor tables, the
// landing buffer of the upload; the region tables of a weights plane built here (weights.hip)
struct PartLayout {
    std::vector<FitLayout> fit;
    size_t lb, ub;
    size_t zeroed;               // bytes from the start that creation zeroes: the grids' padding (weight 0), the state blocks
    size_t summary, bestx, tables, raw;
    size_t wspecs, rspec, edges, level, pairs;
    size_t total;
};

PartLayout lay_out(const BatchPart *b, size_t n_wspecs, size_t n_regions)
{
    const size_t K = (size_t)b->K, Dsum = (size_t)b->Dsum, Nsum = (size_t)b->noff[K];
    PartLayout L;
    L.fit.resize(K);
    Carver c;
    for (size_t k = 0; k < K; ++k) {
        FitLayout &f = L.fit[k];
        const size_t D = (size_t)b->D[k], S = (size_t)b->Sk[k], n_chunks = (size_t)block_plan(b->Nk[k]).n_chunks;
        f.grid_bytes = align256(n_chunks * kChunk * sizeof(double));
        f.xv_bytes = align256(S * D * sizeof(double));
        f.p_bytes = align256((S * D + S) * sizeof(double));
        f.state_bytes = swarm_state_bytes((int64_t)D);
        f.grid = c.take(4 * f.grid_bytes);
        f.chunk = c.take(n_chunks * sizeof(double2));
        f.xv = c.take(4 * f.xv_bytes);
        f.p = c.take(2 * f.p_bytes);
        f.fx = c.take(S * sizeof(double));
        f.cand = c.take((D + 1) * sizeof(double));
        f.state = c.take(2 * f.state_bytes);
    }
    L.lb = c.take(Dsum * sizeof(double));
    L.ub = c.take(Dsum * sizeof(double));
    L.zeroed = c.total;
    L.summary = c.take(K * 4 * sizeof(double));
    L.bestx = c.take(Dsum * sizeof(double) + K * sizeof(int64_t));
    L.tables = c.take(9 * K * sizeof(BatchFit));
    L.raw = c.take(4 * Nsum * sizeof(double));
    L.wspecs = c.take(n_wspecs * sizeof(WeightSpec));
    L.rspec = c.take(n_regions * sizeof(int32_t));
    L.edges = c.take(2 * n_regions * sizeof(double));
    L.level = c.take(n_regions * sizeof(double));
    L.pairs = c.take(2 * n_regions * sizeof(int64_t));
    L.total = c.total;
    return L;
}

// the nine descriptor tables (host copy, uploaded once): every fit's pointers from its layout, its grid's constants, its
// swarm's constants; the fused tables carry the offset of the row copies in the part's geometry (b->mode)
std::vector<BatchFit> build_tables(const BatchPart *b, const PartLayout &L, unsigned char *base, const double *w,
                                   const nmrfit_pso_params *params)
{
    const size_t K = (size_t)b->K;
    std::vector<BatchFit> tabs(9 * K);
    auto at = [&](size_t offset) { return reinterpret_cast<double *>(base + offset); };
    for (size_t k = 0; k < K; ++k) {
        const FitLayout &m = L.fit[k];
        const size_t D = (size_t)b->D[k];
        double *const x[2] = {at(m.xv), at(m.xv + 2 * m.xv_bytes)}, *const vel[2] = {at(m.xv + m.xv_bytes), at(m.xv + 3 * m.xv_bytes)};
        double *const p[2] = {at(m.p), at(m.p + m.p_bytes)}, *const best[2] = {at(m.state), at(m.state + m.state_bytes)};
        BatchFit f{};
        f.wc = at(m.grid);
        f.u = at(m.grid + m.grid_bytes);
        f.v = at(m.grid + 2 * m.grid_bytes);
        f.wt = at(m.grid + 3 * m.grid_bytes);
        f.chunk = reinterpret_cast<double2 *>(base + m.chunk);
        double grid_dev = 0.0;
        const int64_t N = b->Nk[k];
        analyse_grid(w + b->noff[k], N, &f.w0, &f.wspan, &f.lane_step, &grid_dev);
        f.rec_devk = grid_dev * 11.0e10;   // (as launch_variant passes it: objective_kernel.h)
        const BlockPlan bp = block_plan(N);   // the fit's own block structure, one segment
        f.N = N;
        f.blk_chunks = bp.blk_chunks;
        f.n_blocks = (int32_t)bp.n_blocks;
        f.seg_len = bp.n_blocks * bp.blk_len;
        f.raw_off = b->noff[k];
        f.S = b->Sk[k];
        f.fx = at(m.fx);
        f.P = b->P[k];
        const nmrfit_pso_params &prm = params[k];
        for (int t = 0; t < 9; ++t) {
            BatchFit e = f;
            PsoFused &q = e.upd;
            if (t == 8) {
                e.X = x[0];   // plain evaluation of generation 0's positions
                // (what batch_init_kernel and the generation-0 tail need travels in table 0)
            } else {
                const int xp = t & 1, bb = (t >> 1) & 1, pending = (t >> 2) & 1;
                q.x_in = x[xp];
                q.v_in = vel[xp];
                q.x_out = x[xp ^ 1];
                q.v_out = vel[xp ^ 1];
                q.p = p[xp];
                q.pflip = (int)(p[xp ^ 1] - p[xp]);
                q.best = best[bb];
                q.flags = reinterpret_cast<const long long *>(q.best + 2 + 2 * D);
                q.flip = (int)(best[bb ^ 1] - best[bb]);
                q.lb = at(L.lb) + b->boff[k];
                q.ub = at(L.ub) + b->boff[k];
                q.seed = prm.seed;
                q.offset = 0;
                q.omega = prm.omega;
                q.phip = prm.phip;
                q.phig = prm.phig;
                q.minstep = prm.minstep;
                q.minfunc = prm.minfunc;
                q.cand = at(m.cand);
                q.pbest = 1u;
                q.tail = 1u;
                q.pending = (unsigned)pending;
                q.xrow_off = xrow_offset(b, b->mode);
            }
            tabs[(size_t)t * K + k] = e;
        }
    }
    return tabs;
}

// The device work of creation behind the allocation and its zeroes, all of it on the part's stream and waited for once at
// the end: the tables, the spectra -- four uploads (or three, and the weights plane built from the regions: two launches), one scatter kernel, one
// chunk-table kernel -- and the boxes.  On failure the caller destroys the part.
int upload_and_prepare(BatchPart *b, const PartLayout &L, const std::vector<BatchFit> &tabs, const double *w, const double *u,
                       const double *v, const double *weights, const std::vector<WeightSpec> &wspecs,
                       const std::vector<int32_t> &region_spec, const double *edges, const double *level, const double *lower,
                       const double *upper)
{
    const int32_t K = b->K;
    const size_t Nsum = (size_t)b->noff[(size_t)K], n_regions = region_spec.size();
    hipStream_t st = b->stream;
    unsigned char *base = reinterpret_cast<unsigned char *>(b->d_block);
    b->d_summary = reinterpret_cast<double *>(base + L.summary);
    b->d_bestx = reinterpret_cast<double *>(base + L.bestx);
    b->d_tables = reinterpret_cast<BatchFit *>(base + L.tables);
    double *d_raw = reinterpret_cast<double *>(base + L.raw);
    b->d_w_plain = d_raw;   // (the w plane stays as uploaded: the region edges of the residual statistics are found on it)
    NMRFIT_HIP(hipMemcpyAsync(b->d_tables, tabs.data(), tabs.size() * sizeof(BatchFit), hipMemcpyHostToDevice, st));
    NMRFIT_HIP(hipMemcpyAsync(b->d_bestx + b->Dsum, b->boff.data(), (size_t)K * sizeof(int64_t), hipMemcpyHostToDevice, st));
    const size_t plane = Nsum * sizeof(double);
    const double *host_arrays[] = {w, u, v, weights};
    for (int a = 0; a < (weights ? 4 : 3); ++a)
        NMRFIT_HIP(hipMemcpyAsync(d_raw + (size_t)a * Nsum, host_arrays[a], plane, hipMemcpyHostToDevice, st));
    if (!weights) {
        NMRFIT_HIP(hipMemcpyAsync(base + L.wspecs, wspecs.data(), wspecs.size() * sizeof(WeightSpec), hipMemcpyHostToDevice, st));
        if (n_regions) {
            NMRFIT_HIP(hipMemcpyAsync(base + L.rspec, region_spec.data(), n_regions * sizeof(int32_t), hipMemcpyHostToDevice, st));
            NMRFIT_HIP(hipMemcpyAsync(base + L.edges, edges, 2 * n_regions * sizeof(double), hipMemcpyHostToDevice, st));
            NMRFIT_HIP(hipMemcpyAsync(base + L.level, level, n_regions * sizeof(double), hipMemcpyHostToDevice, st));
        }
        const int rc = launch_weights(st, K, reinterpret_cast<const WeightSpec *>(base + L.wspecs),
                                      reinterpret_cast<const int32_t *>(base + L.rspec), (int64_t)n_regions, b->Nmax, d_raw,
                                      reinterpret_cast<const double *>(base + L.edges), reinterpret_cast<const double *>(base + L.level),
                                      reinterpret_cast<int64_t *>(base + L.pairs), d_raw + 3 * Nsum);
        if (rc != NMRFIT_OK) return rc;
    }
    NMRFIT_HIP(hipMemcpyAsync(base + L.lb, lower, (size_t)b->Dsum * sizeof(double), hipMemcpyHostToDevice, st));
    NMRFIT_HIP(hipMemcpyAsync(base + L.ub, upper, (size_t)b->Dsum * sizeof(double), hipMemcpyHostToDevice, st));
    const int rc = launch_prepare(b, d_raw);
    if (rc != NMRFIT_OK) return rc;
    NMRFIT_HIP(hipStreamSynchronize(st));   // (the caller's host vectors go out of scope)
    return NMRFIT_OK;
}

int part_destroy(BatchPart *b)
{
    if (!b) return NMRFIT_OK;
    (void)hipSetDevice(b->device);
    if (b->stream) (void)hipStreamSynchronize(b->stream);
    if (b->d_result) (void)hipFree(b->d_result);
    if (b->d_quality) (void)hipFree(b->d_quality);
    if (b->d_block) (void)hipFree(b->d_block);
    if (b->stream) give_stream(b->device, b->stream);
    delete b;
    return NMRFIT_OK;
}

// (w, u, v, weights: the part's fits one after the other, fit k's Nk[k] points at offset sum_{i<k} Nk[i].  `weights`
// null: the weights plane is built on the device from the part's regions -- R[k] of them per fit, their bounds and
// levels concatenated in edges and level, already checked (check_weight_regions) -- by the two launches of weights.hip)
int part_create(int device, int32_t K, const int64_t *Nk, const double *w, const double *u, const double *v,
                const double *weights, const int32_t *R, const double *edges, const double *level, const int32_t *P,
                const double *lower, const double *upper, const int64_t *swarm, const nmrfit_pso_params *params,
                int variant, int fit_im, BatchPart **out)
{
    if (!out) return refuse(NMRFIT_E_INVALID, "null out pointer");
    *out = nullptr;
    int rc = check_part_args(K, Nk, w, u, v, weights, R, P, lower, upper, swarm, params, variant, fit_im);
    if (rc != NMRFIT_OK) return rc;
    DeviceInfo prop;
    if ((rc = use_device(device, &prop)) != NMRFIT_OK) return rc;
    BatchPart *b = new (std::nothrow) BatchPart();
    if (!b) return refuse(NMRFIT_E_INVALID, "out of host memory");
    b->device = device;
    b->compute_units = prop.cus;
    b->K = K;
    b->variant = variant;
    b->fit_im = fit_im;
    if ((rc = describe_fits(b, Nk, swarm, P, lower, upper)) != NMRFIT_OK) {
        delete b;
        return rc;
    }
    NMRFIT_HIP_OR(take_stream(device, &b->stream), part_destroy(b));
    plan_geometry(b);
    if (!b->geom_ok[0] && !b->geom_ok[1]) {
        const bool ragged = b->N == 0 && b->fit_im == NMRFIT_FIT_IM_OFF;
        part_destroy(b);
        return refuse(NMRFIT_E_UNSUPPORTED,
                      ragged ? "nmrfit_batch_create: fits of different grid lengths run in the wave = particle geometry, and these peak "
                               "counts leave its LDS records no room"
                             : "nmrfit_batch_create: too many peaks for the kernel's LDS records in a batched launch");
    }
    std::vector<WeightSpec> wspecs;
    std::vector<int32_t> region_spec;
    if (!weights) weights_layout(K, Nk, R, &wspecs, &region_spec);
    const PartLayout L = lay_out(b, wspecs.size(), region_spec.size());
    NMRFIT_HIP_OR(device_alloc(&b->d_block, L.total), part_destroy(b));
    unsigned char *base = reinterpret_cast<unsigned char *>(b->d_block);
    NMRFIT_HIP_OR(hipMemsetAsync(base, 0, L.zeroed, b->stream), part_destroy(b));
    const std::vector<BatchFit> tabs = build_tables(b, L, base, w, params);
    b->h_fits.assign(tabs.begin(), tabs.begin() + K);
    if ((rc = upload_and_prepare(b, L, tabs, w, u, v, weights, wspecs, region_spec, edges, level, lower, upper)) != NMRFIT_OK) {
        part_destroy(b);
        return rc;
    }
    *out = b;
    return NMRFIT_OK;
}

}  // namespace
}  // namespace nmrfit

using namespace nmrfit;

// nmrfit_batch_create_ragged (weights given) and nmrfit_batch_create_regions (weights null; R, edges, level: checked)
static int batch_create(int device, int32_t K, const int64_t *N, const double *w, const double *u, const double *v,
                        const double *weights, const int32_t *R, const double *edges, const double *level, const int32_t *P,
                        const double *lower, const double *upper, const int64_t *swarmsize, const nmrfit_pso_params *params,
                        int variant, int fit_im, nmrfit_batch **out)
{
    if (!out) return refuse(NMRFIT_E_INVALID, "null out pointer");
    *out = nullptr;
    if (K <= 0 || !N || !swarmsize || !w || !u || !v || (!weights && !R) || !P || !lower || !upper || !params)
        return refuse(NMRFIT_E_INVALID, kCreateArgs);
    nmrfit_batch *b = new (std::nothrow) nmrfit_batch();
    if (!b) return refuse(NMRFIT_E_INVALID, "out of host memory");
    b->K = K;
    b->device = device;
    b->boff.resize((size_t)K + 1);
    b->noff.resize((size_t)K + 1);
    b->prow.resize((size_t)K + 1);
    b->boff[0] = b->noff[0] = b->prow[0] = 0;
    for (int32_t k = 0; k < K; ++k) {
        b->boff[(size_t)k + 1] = b->boff[(size_t)k] + 4 + 3 * (int64_t)std::max(P[k], 0);
        b->noff[(size_t)k + 1] = b->noff[(size_t)k] + std::max<int64_t>(N[k], 0);
        b->prow[(size_t)k + 1] = b->prow[(size_t)k] + std::max(P[k], 0);
    }
    int nparts = (K >= 6) ? 2 : 1;
    if (const char *e = getenv("NMRFIT_BATCH_STREAMS")) nparts = std::max(1, std::min(atoi(e), (int)std::min<int32_t>(K, 8)));
    for (int p = 0; p <= nparts; ++p) b->first.push_back((int32_t)((int64_t)K * p / nparts));
    int64_t r0 = 0;   // regions before the part (the region tables are offset per part, as the planes are)
    for (int p = 0; p < nparts; ++p) {
        const int32_t f0 = b->first[(size_t)p], f1 = b->first[(size_t)p + 1];
        const int64_t n0 = b->noff[(size_t)f0];
        BatchPart *part = nullptr;
        const int rc = part_create(device, f1 - f0, N + f0, w + n0, u + n0, v + n0, weights ? weights + n0 : nullptr,
                                   R ? R + f0 : nullptr, edges ? edges + 2 * r0 : nullptr, level ? level + r0 : nullptr, P + f0,
                                   lower + b->boff[(size_t)f0], upper + b->boff[(size_t)f0], swarmsize + f0, params + f0, variant,
                                   fit_im, &part);
        if (rc != NMRFIT_OK) {
            nmrfit_batch_destroy(b);
            return rc;
        }
        b->parts.push_back(part);
        for (int32_t k = f0; R && k < f1; ++k) r0 += R[k];
    }
    *out = b;
    return NMRFIT_OK;
}

#pragma GCC visibility push(default)   // the C-ABI: the only symbols the library exports (build.sh: -fvisibility=hidden)
extern "C" {

int nmrfit_batch_create_ragged(int device, int32_t K, const int64_t *N, const double *w, const double *u, const double *v,
                               const double *weights, const int32_t *P, const double *lower, const double *upper,
                               const int64_t *swarmsize, const nmrfit_pso_params *params, int variant, int fit_im, nmrfit_batch **out)
{
    if (out && !weights) {   // (reported as batch_create reports the other null arrays)
        *out = nullptr;
        set_error(kCreateArgs);
        return NMRFIT_E_INVALID;
    }
    return batch_create(device, K, N, w, u, v, weights, nullptr, nullptr, nullptr, P, lower, upper, swarmsize, params, variant,
                        fit_im, out);
}

int nmrfit_batch_create_regions(int device, int32_t K, const int64_t *N, const double *w, const double *u, const double *v,
                                const int32_t *R, const double *edges, const double *level, const int32_t *P,
                                const double *lower, const double *upper, const int64_t *swarmsize,
                                const nmrfit_pso_params *params, int variant, int fit_im, nmrfit_batch **out)
{
    const char *who = "nmrfit_batch_create_regions";
    if (!out) return refuse(NMRFIT_E_INVALID, "null out pointer");
    *out = nullptr;
    if (!w || !u || !v || !P || !lower || !upper || !swarmsize || !params)
        return refuse(NMRFIT_E_INVALID, std::string(who) + ": null pointer");
    int64_t n_points = 0, n_regions = 0;
    const int rc = check_weight_regions(who, K, N, R, edges, level, &n_points, &n_regions);
    if (rc != NMRFIT_OK) return rc;
    return batch_create(device, K, N, w, u, v, nullptr, R, edges, level, P, lower, upper, swarmsize, params, variant, fit_im, out);
}

int nmrfit_batch_create(int device, int32_t K, int64_t N, const double *w, const double *u, const double *v,
                        const double *weights, const int32_t *P, const double *lower, const double *upper,
                        int64_t swarmsize, const nmrfit_pso_params *params, int variant, int fit_im, nmrfit_batch **out)
{
    if (K <= 0 || N <= 0 || swarmsize <= 0) {
        if (out) *out = nullptr;
        set_error(kCreateArgs);
        return NMRFIT_E_INVALID;
    }
    const std::vector<int64_t> lengths((size_t)K, N), swarms((size_t)K, swarmsize);
    return nmrfit_batch_create_ragged(device, K, lengths.data(), w, u, v, weights, P, lower, upper, swarms.data(), params, variant,
                                      fit_im, out);
}

int nmrfit_batch_destroy(nmrfit_batch *b)
{
    if (!b) return NMRFIT_OK;
    for (BatchPart *p : b->parts) (void)part_destroy(p);
    delete b;
    return NMRFIT_OK;
}

}  // extern "C"
#pragma GCC visibility pop

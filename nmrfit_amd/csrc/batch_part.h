// batch_part.h -- what the host-side units of the device-batched fits share: one part of a batch (a set of fits advanced
// by one launch per generation on one stream), the batch (its fits divided over one or two parts), and the few steps that
// every unit's entry points begin with.  batch_create.hip makes and destroys them, batch.hip runs the generations;
// batch_lsq.hip (least squares) and batch_data.hip (reconstruction, noise, spectra) work on their resident arrays.
#pragma once
#include "batch_internal.h"
#include "host_call.h"

#include <vector>

struct BatchPart {
    int device = -1;
    int compute_units = 0;
    hipStream_t stream = nullptr;
    int32_t K = 0;
    int64_t N = 0;                       // the fits' common grid length, or 0 when they differ (ragged: wave = particle form only)
    int64_t S = 0, n_chunks = 0;         // particles per fit, or 0 when the swarms differ in size (wave = particle form only); chunks of the LONGEST grid
    std::vector<int64_t> Sk;             // per fit: swarm size
    int64_t Smax = 0, Ssum = 0;
    std::vector<int64_t> Nk, noff;       // per fit: grid length; offset of its first point in the concatenated arrays (+ total)
    int64_t Nmax = 0;
    int variant = NMRFIT_VARIANT_DEFAULT;
    int fit_im = NMRFIT_FIT_IM_OFF;
    int32_t Pmax = 0;
    std::vector<int32_t> P;
    std::vector<int64_t> D, boff;        // per fit: 4 + 3P, offset of its bounds / best row in the concatenated arrays
    int64_t Dsum = 0;
    void *d_block = nullptr;             // the one allocation behind everything below
    nmrfit::BatchFit *d_tables = nullptr;   // [9][K]: t = xp + 2 b + 4 pending (fused generations), 8 = plain evaluation
    double *d_summary = nullptr;         // [K][4]: generations, stop code, fg, best_f   (written by batch_tail_kernel)
    double *d_bestx = nullptr;           // [Dsum]: best_x rows, concatenated
    const double *d_w_plain = nullptr;   // [sum of the fits' lengths]: the uploaded grids, plain order, NOT centred (the upload's landing buffer)
    std::vector<nmrfit::BatchFit> h_fits;   // host copy of table 0: every fit's array pointers and grid constants
    int64_t Psum = 0;
    // scratch of a reconstruction call in flight (nmrfit_batch_contributions): device block, and what goes where on the host
    void *d_result = nullptr;
    struct ResultCopy {
        void *host;
        const void *dev;
        size_t bytes;
    };
    std::vector<ResultCopy> result_copies;
    // the buffers of nmrfit_batch_quality_stats (job table, region tables, the tiles' sums, the rows): grown on demand
    void *d_quality = nullptr;
    size_t cap_quality = 0;
    // launch geometry: [0] workgroup = particle, [1] wave = particle
    nmrfit::BatchLaunch geom[2];
    bool geom_ok[2] = {false, false};
    int mode = 0;                        // 0 workgroup form, 1 wave form (chosen at creation; nmrfit_batch_set_geometry)
    // phases
    int xp = 0, b = 0;
    bool fold_pending = false;
    bool initialized = false;
    bool noised = false;                 // nmrfit_batch_add_noise has perturbed the resident u, v (allowed once)
    int64_t launches = 0;
};

// A generation of a part is a few lock-step rounds of short waves: its last round drains with the SIMDs
// half empty, its first starts with every wave in the latency-bound prologue.  Two parts on two streams fill each
// other's gaps -- the launches of one generation of part A and part B are independent -- for 5-11 % more fits per
// second (K = 40: 216 -> 241, K = 200: 238 -> 251; profiles/r05/batch_two_streams.txt; K = 6 ... 12: +3-8 %).  From 6
// fits on (each part then still has the particles for the wave = particle geometry); NMRFIT_BATCH_STREAMS=1 turns it
// off (A/B knob).
struct nmrfit_batch {
    std::vector<BatchPart *> parts;
    std::vector<int32_t> first;      // first fit of each part (+ K at the end)
    std::vector<int64_t> boff;       // offset of each fit's row in the concatenated bounds / best arrays (+ total)
    std::vector<int64_t> noff;       // offset of each fit's first grid point in the concatenated spectra (+ total)
    std::vector<int64_t> prow;       // peaks before each fit (+ total)
    int32_t K = 0;
    int device = -1;
};

namespace nmrfit {

// ---- batch.hip ----
// the part's two launch geometries (geom, geom_ok) and the one it starts in (mode), from its fits' shapes
void plan_geometry(BatchPart *b);
unsigned xrow_offset(const BatchPart *b, int m);           // where geometry m keeps the row copies in LDS (PsoFused::xrow_off)
int launch_prepare(BatchPart *b, const double *d_raw);     // creation: scatter the uploaded planes, build the chunk tables
int bind_batch(const BatchPart *b);                        // the part's device becomes the calling thread's
int bind_started(BatchPart *b, const char *who);           // ... and NMRFIT_E_STATE before the part's first generation
int flush_fold(BatchPart *b);                              // fold the generation that still waits, in a launch of its own
int check_batch_handle(const nmrfit_batch *b);             // non-null, and its device the calling thread's
int part_of(const nmrfit_batch *b, int32_t k);             // the part that holds fit k
// NMRFIT_E_STATE while a reconstruction of the batch is in flight (a part's d_result)
int check_idle(const nmrfit_batch *b, const char *who);

}  // namespace nmrfit

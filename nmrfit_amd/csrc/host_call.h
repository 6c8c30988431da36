// host_call.h -- what the host side of an entry point is built from besides nmrfit_internal.h's use_device and
// NMRFIT_HIP (host_call.hip): the argument checks of the calls on a context, the device buffers and the stream of one
// call, the layout of an object's one allocation, and the HIP call of a create function.  Host code only.
#pragma once
#include "nmrfit_internal.h"

#include <algorithm>
#include <vector>

#include "poison_knob.h"

namespace nmrfit {

// The one home of device allocation: every hipMalloc of the library is this call (host_call.hip).  With the diagnostic
// NMRFIT_POISON_ALLOC=<byte> (poison_knob.h) the new block is filled with that byte, and the fill is
// complete on return -- so that no result can lean on what a fresh block happens to hold (the audit table).
hipError_t device_alloc(void **p, size_t bytes);

// A HIP call while an object is half built: on failure the error is recorded with the call's own file and line,
// `cleanup` (the object's destroy call) runs, and the enclosing function returns the code.
#define NMRFIT_HIP_OR(call, cleanup)                                                  \
    do {                                                                              \
        hipError_t _e = (call);                                                       \
        if (_e != hipSuccess) {                                                       \
            int _rc = ::nmrfit::hip_fail(_e, #call, __FILE__, __LINE__);              \
            cleanup;                                                                  \
            return _rc;                                                               \
        }                                                                             \
    } while (0)

// a refusal: the message recorded, the code returned
inline int refuse(int code, const std::string &msg)
{
    set_error(msg);
    return code;
}

// What the entry points on a context (ctx.hip, ctx_eval.hip) begin with: the context is there, and its device is the
// calling thread's current one
inline int bind(const nmrfit_ctx *ctx)
{
    if (!ctx) return refuse(NMRFIT_E_INVALID, "null context");
    NMRFIT_HIP(hipSetDevice(ctx->device));
    return NMRFIT_OK;
}

// S parameter rows of P peaks at X, results at `out`
inline int check_batch(int64_t S, int32_t P, const void *X, const void *out)
{
    if (S < 0 || P < 0) return refuse(NMRFIT_E_INVALID, "negative batch size or peak count");
    if (P > kMaxPeaks)
        return refuse(NMRFIT_E_INVALID, "P exceeds the supported maximum of " + std::to_string(kMaxPeaks) +
                                            " peaks (per-peak records of a workgroup live in a CU's 160 KiB of LDS)");
    if (S > 0 && (!X || !out)) return refuse(NMRFIT_E_INVALID, "null parameter/output pointer");
    return NMRFIT_OK;
}

inline int check_fit_im(int fit_im)
{
    if (fit_im < 0 || fit_im > NMRFIT_FIT_IM_SUM)
        return refuse(NMRFIT_E_INVALID, "fit_im must be 0 (real part), 1 (reference fit_im=True) or 2 (all-peak imaginary model)");
    return NMRFIT_OK;
}

inline size_t align256(size_t bytes) { return (bytes + 255) & ~(size_t)255; }

// one allocation cut into 256-byte aligned pieces: take() returns a piece's byte offset, total is what to allocate
struct Carver {
    size_t total = 0;
    size_t take(size_t bytes)
    {
        const size_t at = total;
        total += align256(bytes);
        return at;
    }
};

// One copy of a swarm's state block -- (fg, best_f, g[D], best_x[D] | generations, stop code), the two flags right behind
// the doubles -- as a lone swarm (pso.hip) and a fit of a batch (batch_create.hip) hold it, twice each: the deferred fold of a
// fused launch reads one copy and writes the other (PsoFused::flip).
inline size_t swarm_state_bytes(int64_t D) { return align256((size_t)(2 + 2 * D) * sizeof(double) + 2 * sizeof(long long)); }

// device buffers of one call, freed on every path
struct Scratch {
    std::vector<void *> ptrs;
    ~Scratch()
    {
        for (void *p : ptrs) (void)hipFree(p);
    }
    template <typename T>
    hipError_t alloc(T **p, size_t n)
    {
        void *q = nullptr;
        hipError_t e = device_alloc(&q, std::max<size_t>(n, 1) * sizeof(T));
        if (e == hipSuccess) ptrs.push_back(q);
        *p = (T *)q;
        return e;
    }
};

// the stream of one call: a recycled one (take_stream), synchronised and handed back on every path
struct StreamLease {
    int device;
    hipStream_t s = nullptr;
    explicit StreamLease(int d) : device(d) {}
    hipError_t take() { return take_stream(device, &s); }
    ~StreamLease()
    {
        if (s) {
            (void)hipStreamSynchronize(s);
            give_stream(device, s);
        }
    }
};

}  // namespace nmrfit

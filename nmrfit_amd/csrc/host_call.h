// host_call.h -- what the host side of an entry point is built from besides nmrfit_internal.h's use_device and
// NMRFIT_HIP: the device buffers and the stream of one call, the layout of an object's one allocation, and the HIP call
// of a create function.  Host code only.
#pragma once
#include "nmrfit_internal.h"

#include <algorithm>
#include <vector>

namespace nmrfit {

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
        hipError_t e = hipMalloc(&q, std::max<size_t>(n, 1) * sizeof(T));
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

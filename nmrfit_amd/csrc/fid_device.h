// fid_device.h -- what the kernels of fid.hip, fid_cond.hip and fid_any.hip share: the complex value and its once-rounded
// arithmetic, and how a workgroup of a flat launch finds its work item, its spectrum and its place in a trace.  Device code.
#pragma once
#include <hip/hip_runtime.h>

namespace nmrfit {

#pragma clang fp contract(off)   // (every product and sum of the definition is rounded once)

struct Cx {
    double re, im;
};
__device__ __forceinline__ Cx cmul(Cx a, Cx w) { return Cx{a.re * w.re - a.im * w.im, a.re * w.im + a.im * w.re}; }
__device__ __forceinline__ Cx cadd(Cx a, Cx b) { return Cx{a.re + b.re, a.im + b.im}; }
__device__ __forceinline__ Cx csub(Cx a, Cx b) { return Cx{a.re - b.re, a.im - b.im}; }

// the spectrum of an item: the largest k < K with pref[k] <= item (a spectrum without items has pref[k] == pref[k + 1])
__device__ __forceinline__ int find_job(const long long *__restrict__ pref, int K, long long item)
{
    int lo = 0, hi = K;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (pref[mid] <= item) lo = mid;
        else hi = mid;
    }
    return lo;
}

// What every kernel of a flat launch opens with: this workgroup's item (blockIdx.y * gridDim.x + blockIdx.x) as the
// spectrum k it belongs to and its number within the spectrum, local() (read from the table where the kernel asks for
// it).  False past the end: the whole workgroup leaves.
struct ItemAt {
    const long long *__restrict__ pref;
    long long item;
    int k;
    __device__ __forceinline__ long long local() const { return item - pref[k]; }
};
__device__ __forceinline__ bool item_at(const long long *__restrict__ pref, int K, ItemAt *at)
{
    const long long total = pref[K], item = (long long)blockIdx.y * gridDim.x + blockIdx.x;
    if (item >= total) return false;
    *at = ItemAt{pref, item, find_job(pref, K, item)};
    return true;
}

constexpr int kFidChunk = 1024;   // points of a trace per work item of an element-wise stage

// the item's trace and first point: a trace of `len` points is ceil(len / 1024) items
__device__ __forceinline__ void item_place(long long local, int len, long long *t, int *from)
{
    const int chunks = (len + kFidChunk - 1) / kFidChunk;
    *t = local / chunks;
    *from = (int)(local - *t * chunks) * kFidChunk;
}

}  // namespace nmrfit

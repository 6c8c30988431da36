// fid_device.h -- what the kernels of fid.hip and fid_cond.hip share: the complex value and its once-rounded
// arithmetic, and how a workgroup of a flat launch finds its work item and its spectrum.  Device code.
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

// the work item of this workgroup, or -1 past the end (the whole workgroup leaves)
__device__ __forceinline__ long long work_item(long long total)
{
    const long long item = (long long)blockIdx.y * gridDim.x + blockIdx.x;
    return item < total ? item : -1;
}

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

}  // namespace nmrfit

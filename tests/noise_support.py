"""
Shared by tests/test_noise_cpu.py and tests/test_gpu_noise.py: the high-precision truth of the noise deviates
(include/nmrfit_amd_noise.h) and the error unit both tiers measure in.

The Philox words are integers and exact in numpy (nmrfit_amd.pso.philox4x32_10); from them a = ((ua >> 11) + 1) 2^-53 and
b = (ub >> 11) 2^-53 are exact doubles and t = 6.283185307179586 * b is, by the definition, the ROUNDED fp64 product.
Everything after that -- log, sqrt, cos, sin, the two products -- is evaluated by mpmath at 200 bits.  The unit of error
is e = 2^-52 max(1, r) with r = sqrt(-2 log a): an ulp of a deviate of size r (|z| <= r), never below an ulp of 1.
"""
import functools

import mpmath
import numpy as np

from nmrfit_amd import noise, pso

TRUTH_SEED, TRUTH_N = 7, 2000


@functools.lru_cache(maxsize=None)
def truth(seed=TRUTH_SEED, N=TRUTH_N):
    """(z_u, z_v, e): the deviates of points 0 .. N-1 rounded from 200-bit values, and the error unit per point.  The
    arrays are shared between tests: read-only."""
    j = np.arange(N, dtype=np.uint64)
    o0, o1, o2, o3 = pso.philox4x32_10(j & np.uint64(0xFFFFFFFF), j >> np.uint64(32), np.full(N, noise.NOISE_TAG, dtype=np.uint64),
                                       np.zeros(N, dtype=np.uint64), seed & 0xFFFFFFFF, seed >> 32)
    ua = [(int(hi) << 32) | int(lo) for hi, lo in zip(o1, o0)]
    ub = [(int(hi) << 32) | int(lo) for hi, lo in zip(o3, o2)]
    zu, zv, e = np.empty(N), np.empty(N), np.empty(N)
    with mpmath.workprec(200):
        for i in range(N):
            a = mpmath.mpf((ua[i] >> 11) + 1) / 2 ** 53
            b = float(ub[i] >> 11) * 2.0 ** -53                 # exact: 53 bits times a power of two
            t = mpmath.mpf(6.283185307179586 * b)               # the rounded fp64 product is the argument
            r = mpmath.sqrt(-2 * mpmath.log(a))
            zu[i], zv[i] = float(r * mpmath.cos(t)), float(r * mpmath.sin(t))
            e[i] = 2.0 ** -52 * max(1.0, float(r))
    for x in (zu, zv, e):
        x.setflags(write=False)
    return zu, zv, e


def worst_error(zu, zv, seed=TRUTH_SEED):
    """max over both channels of |z - truth| / e."""
    tu, tv, e = truth(seed, len(zu))
    return float(max(np.max(np.abs(zu - tu) / e), np.max(np.abs(zv - tv) / e)))

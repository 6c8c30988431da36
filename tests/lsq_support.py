"""
Shared by tests/test_lsq_batch_cpu.py and tests/test_gpu_lsq_batch.py: exactly summed normal equations and the bound a
floating-point sum of them must keep, the cases of the lock-step polish, and scipy's TRF driven by given residual rows.
"""
import math

import numpy as np

from nmrfit_amd import lsq, synth

U = 2.0 ** -53

# What the final objective of lsq.lm_polish may differ by, relatively, from scipy TRF's on the same smooth function from
# the same start: ten times the largest gap measured over polish_cases() on the CPU with the C restatement of the
# residual as the provider of both (tools/lsq_timing.py --cpu; profiles/lsq_timing.txt: 6.73e-13), capped at 1e-6 --
# beyond the cap a difference is another minimum, not another stopping rule.
MEASURED_GAP = 6.73e-13
FINAL_F_BAR = min(10.0 * MEASURED_GAP, 1e-6)


def _split(a):
    c = 134217729.0 * a
    hi = c - (c - a)
    return hi, a - hi


def two_product(a, b):
    """p + e == a * b exactly (Dekker / Veltkamp; no overflow or underflow for the magnitudes of a Jacobian)."""
    p = a * b
    ah, al = _split(a)
    bh, bl = _split(b)
    e = ((ah * bh - p) + ah * bl + al * bh) + al * bl
    return p, e


def exact_normal_equations(J, r):
    """A = J^T J, g = J^T r with every entry the EXACT sum of the exact products, rounded once (math.fsum over the
    error-free split of every product), and for the bound a LOWER estimate of every entry's sum of absolute exact
    products: numpy's sum of the rounded ones is at most (1 + u)^(N + 1) above it, so that sum times
    (1 - 2 (N + 1) u) lies below -- the bound made of it is a hair tighter than the one stated, never wider."""
    N, D = J.shape
    cols = np.ascontiguousarray(J.T)
    A = np.empty((D, D))
    absA = np.empty((D, D))
    g = np.empty(D)
    absg = np.empty(D)
    low = 1.0 - 2.0 * (N + 1) * U
    for i in range(D):
        others = np.vstack((cols[i:], r[None, :]))            # columns i .. D - 1, then r
        p, e = two_product(cols[i][None, :], others)
        totals = [math.fsum(row) for row in np.concatenate((p, e), axis=1).tolist()]
        mags = np.abs(p).sum(axis=1) * low
        A[i, i:] = A[i:, i] = totals[:-1]
        absA[i, i:] = absA[i:, i] = mags[:-1]
        g[i], absg[i] = totals[-1], mags[-1]
    return A, g, absA, absg


def sum_bound(N, mags):
    """|computed - exact| for a sum of N products in ANY order, with or without FMA: the products round once each (or not
    at all), the N - 1 additions once each -- (1 + u)^N - 1 <= 1.01 N u for N u < 0.01 -- and one more u for the rounding
    of the exact value itself: 1.01 (N + 1) 2^-53 sum_j |J_ji J_jk|."""
    return 1.01 * (N + 1) * U * mags


def spectrum_tuple(sp):
    return sp["w"], sp["u"], sp["v"], sp["weights"]


def perturbed_start(sp, seed, spread=0.02):
    """The generating parameters moved by up to ``spread`` of the box, inside it: where a swarm leaves a fit."""
    rng = np.random.default_rng(seed)
    lo, hi = np.asarray(sp["lower"], float), np.asarray(sp["upper"], float)
    x = np.asarray(sp["x_true"], float) + spread * (hi - lo) * rng.uniform(-1.0, 1.0, lo.size)
    return np.clip(x, lo, hi)


def polish_cases():
    """physical=True spectra, P = 1, 2, 3, N = 1024, and a start near the optimum."""
    out = []
    for P in (1, 2, 3):
        sp = synth.make_spectrum(1024, P, seed=40 + P, physical=True)
        out.append((sp, perturbed_start(sp, 50 + P)))
    return out


# scipy's default tolerances (1e-8 on the change of the COST, 0.5 f^2) stop TRF short of the minimum wherever the valley
# is flat -- on the one-peak case 1.4e-6 relative above the value it reaches itself with tighter ones, which is also
# lm_polish's to 1e-12.  Two solvers can only be compared at the minimum if both go there: TRF runs with lm_polish's
# own ftol in all three of its tests, here and in lsq.polish on the GPU.
TRF_TOL = dict(ftol=1e-12, xtol=1e-12, gtol=1e-12)


def trf_on_rows(residual, x0, lower, upper):
    """scipy's TRF on fun(x) = R[0] s and the forward-difference Jacobian of lsq.forward_rows, both from
    ``residual(rows) -> (R, f)``: what lsq.least_squares does with a device context.  Returns (x, f)."""
    from scipy.optimize import least_squares
    lower, upper = np.asarray(lower, float), np.asarray(upper, float)

    def fun(x):
        R, _ = residual(np.asarray(x, float)[None, :])
        return R[0] / np.sqrt(R.shape[1])

    def jac(x):
        rows, h = lsq.forward_rows(x, lower, upper)
        R, _ = residual(rows)
        s = 1.0 / np.sqrt(R.shape[1])
        return lsq.normal_equations_host(R, s / h, s)[2]

    res = least_squares(fun, np.clip(x0, lower, upper), jac=jac, bounds=(lower, upper), method="trf",
                        x_scale=np.maximum(upper - lower, 1e-12), **TRF_TOL)
    _, f = residual(res.x[None, :])
    return res.x, float(f[0])

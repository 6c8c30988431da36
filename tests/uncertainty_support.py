"""
Shared by tests/test_uncertainty_cpu.py and tests/test_gpu_uncertainty.py: the sandwich covariance of a fit
(nmrfit_amd/uncertainty.py, csrc/lsq_cov.hip) against the linear response of tests/calibration_support.py.

``Truth.cov``, ``Truth.sigma_x`` and ``Truth.af_sigma`` there are what the feature must return, computed by central
differences (and, on the noisy base, the full Hessian).  ``mirror`` is the feature's own statement on the CPU:
``uncertainty.sandwich_host`` + ``uncertainty.covariance`` on the forward-difference Jacobian the device forms
(``lsq.forward_rows``), with the oracle's residual in the kernel's place.
"""
import functools

import numpy as np

from nmrfit_amd import lsq, uncertainty

from . import calibration_support as cs

EXACT_CASES = ("n512_p2", "n512_p2_unit", "n1024_p3_v2", "n1024_p3_unit", "user_n512_p2", "user_n1024_p3_v2")
NOISY_CASES = ("end_to_end",)
DEVICE_CASES = ("n512_p2", "n1024_p3_v2", "user_n1024_p3_v2", "end_to_end")

# -- the bars ----------------------------------------------------------------------------------------------------------
# The largest deviation of the mirror from the truth over the cases of a class, measured on the CPU
# (tests/test_uncertainty_cpu.py::test_mirror_against_the_truth re-measures and prints them):
#   std : max_i |params_std_i / sigma_x_i - 1|
#   af  : |area_fraction_std / af_sigma - 1|
#   cov : max_ab |cov_ab - Truth.cov_ab| / (sigma_x_a sigma_x_b)
# exact base: the forward step's truncation; noisy base: the truth takes the full Hessian, so this is the size of the
# Gauss-Newton remainder sum_j r_j grad^2 r_j.  The bar of a class is calibration_support.twice_rounded_up(measured), on
# the CPU and on the device alike.
MEASURED = {"exact": dict(std=4.56e-6, af=8.04e-7, cov=2.22e-5), "noisy": dict(std=1.75e-3, af=2.07e-4, cov=3.49e-3)}
# fault -> (the case that shows it, the deviation of the standard errors measured there)
FAULTS = {"variance": ("n512_p2", 1.0), "swapped": ("n1024_p3_v2", 0.94), "no_weights": ("n512_p2", 0.44),
          "ramp": ("n1024_p3_v2", 5.9e-5)}


def klass(name):
    return "noisy" if name in NOISY_CASES else "exact"


def bars(name):
    return {k: cs.twice_rounded_up(v) for k, v in MEASURED[klass(name)].items()}


# -- the mirror ----------------------------------------------------------------------------------------------------------
def forward_jacobian(c, x):
    """(J [N x D], r [N]) of the weighted residual at x as the device forms them: the rows and realised steps of
    ``lsq.forward_rows`` in the case's box, J[:, i] = (R[i + 1] - R[0]) * (1 / h_i)."""
    rows, h = lsq.forward_rows(x, np.asarray(c.lower, float), np.asarray(c.upper, float))
    R = np.array([cs.residual(c, row) for row in rows])
    return np.ascontiguousarray(((R[1:] - R[0]) / h[:, None]).T), R[0]


@functools.lru_cache(maxsize=None)
def jacobian_at_truth(name):
    t = cs.truth(name)
    J, r = forward_jacobian(t.case, t.x0)
    J.setflags(write=False)
    r.setflags(write=False)
    return J, r


def mirror(name, fault=None):
    """The ``FitUncertainty`` of case ``name`` at ``Truth.x0`` from the CPU mirror -- or with one fault injected into
    the meat: sigma applied as a variance, sigma_u and sigma_v swapped, the weights left out of q_j, the phase ramp
    j / (N - 1) instead of j / N."""
    t = cs.truth(name)
    c = t.case
    J, r = jacobian_at_truth(name)
    su, sv, weights, xq = c.sigma_u, c.sigma_v, c.weights, t.x0.copy()
    if fault == "variance":
        su, sv = su * su, sv * sv
    elif fault == "swapped":
        su, sv = sv, su
    elif fault == "no_weights":
        weights = np.ones(c.N)
    elif fault == "ramp":
        xq[1] = xq[1] * c.N / (c.N - 1.0)
    elif fault is not None:
        raise ValueError(fault)
    M = uncertainty.sandwich_host(J, weights, xq, su, sv)
    return uncertainty.covariance(J.T @ J, M, J.T @ r, t.x0, c.lower, c.upper, sigma=(su, sv))


def deviations(name, fu):
    """dict(std, af, cov) of a FitUncertainty from the truth of case ``name`` (see MEASURED)."""
    t = cs.truth(name)
    return dict(std=float(np.max(np.abs(fu.params_std / t.sigma_x - 1.0))),
                af=float(abs(fu.area_fraction_std / t.af_sigma - 1.0)),
                cov=float(np.max(np.abs(fu.cov - t.cov) / np.outer(t.sigma_x, t.sigma_x))))


# -- the same bits everywhere ----------------------------------------------------------------------------------------------
# Three fits of different N and P whose residual rows, (D + 1) N doubles, are 120640, 163840 and 156000: any two exceed the
# smallest workspace budget (NMRFIT_LSQ_WORKSPACE_MB=1: 131072 doubles), so under it every fit is a group of its own.
# 4160 = 65 tiles (two tiles per segment, a last segment of one), 8192 = two tiles per segment exactly, 6000 ends in a
# ragged tile of 48 points.
BITS_SHAPES = ((4160, 8), (8192, 5), (6000, 7))
BITS_KEYS = ("A", "M", "g", "f")


def bits_problems():
    from nmrfit_amd import synth
    from .lsq_support import perturbed_start
    sps = [synth.make_spectrum(N, P, seed=70 + k, physical=True) for k, (N, P) in enumerate(BITS_SHAPES)]
    X = [perturbed_start(sp, 80 + k) for k, sp in enumerate(sps)]
    sig = [(1e-3 * float(np.max(np.abs(sp["u"]))), 2e-3 * float(np.max(np.abs(sp["u"])))) for sp in sps]
    return sps, X, sig


def batch_sandwich(sps, X, sig, order):
    """(A, M, g, f) of every problem from ONE FitBatch.sandwich call on a batch that holds them in ``order``."""
    from nmrfit_amd.batch import FitBatch
    with FitBatch([(sps[k]["w"], sps[k]["u"], sps[k]["v"], sps[k]["weights"]) for k in order], [sps[k]["lower"] for k in order],
                  [sps[k]["upper"] for k in order], swarmsize=8, seeds=list(range(len(order)))) as fb:
        got = fb.sandwich([X[k] for k in order], [sig[k][0] for k in order], [sig[k][1] for k in order])
    out = [None] * len(sps)
    for place, k in enumerate(order):
        out[k] = got[place]
    return out


def lone_sandwich(sp, x, sig):
    from nmrfit_amd.equations import Evaluator
    with Evaluator(sp["w"], sp["u"], sp["v"], sp["weights"]) as ev:
        return lsq.ResidualModel(ev, sp["lower"], sp["upper"]).sandwich(x, sig[0], sig[1])


def device_record():
    """What one process gets for bits_problems(): every fit on a lone context and in a batch, as one dict of arrays."""
    sps, X, sig = bits_problems()
    rec = {}
    batch = batch_sandwich(sps, X, sig, (0, 1, 2))
    for k, (sp, x, sg) in enumerate(zip(sps, X, sig)):
        for name, a, b in zip(BITS_KEYS, lone_sandwich(sp, x, sg), batch[k]):
            rec["lone.%d.%s" % (k, name)] = np.asarray(a)
            rec["batch.%d.%s" % (k, name)] = np.asarray(b)
    return rec


def main(out):
    """``python -m tests.uncertainty_support OUT.npz``: device_record() of this process (a child of
    tests/test_gpu_uncertainty.py, started with its own NMRFIT_POISON_ALLOC)."""
    np.savez(out, **device_record())


# -- the device's meat against numpy ---------------------------------------------------------------------------------------
# What |M_dev - M_numpy| may be per entry, with numpy's M = (q J)^T J made from the device's OWN J (bit for bit the host
# expression) and numpy's q.  Every term q_j J_ja J_jb of an entry is the same real number on both sides up to
#   * the roundings of one term: the quotient j / N, the product with p1, the sum with p0 (those three move phi and are
#     counted below), then sin, cos (1 ulp each on either side), their squares, the two products with the variances,
#     their sum, weights * s, its square, the product with omega, q * J_ja, and the FMA's one rounding: about 16 eps of the
#     term in all, both sides together;
#   * phi's own rounding, eps (|p0| + |p1|) at most on each side (|p1 j / N| <= |p1|), which reaches omega through
#     d omega / d phi = (sigma_v^2 - sigma_u^2) sin 2 phi: relative to omega >= min sigma^2 that is
#     2 (|p0| + |p1|) max sigma^2 / min sigma^2 eps;
# and the two sides add the N terms in different orders: each side's sum is within N eps sum_j |term_j| of the exact one
# (the classic bound for any order of recursive summation, FMA or not), 2 N eps together.
def meat_bound(J, q, x, sigma_u, sigma_v):
    """[D x D]: eps * sum_j |q_j J_ja J_jb| * (2 N + 16 + 2 (|p0| + |p1|) max sigma^2 / min sigma^2)."""
    N = J.shape[0]
    eps = np.finfo(np.float64).eps
    s2 = (sigma_u * sigma_u, sigma_v * sigma_v)
    factor = 2.0 * N + 16.0 + 2.0 * (abs(x[0]) + abs(x[1])) * max(s2) / min(s2)
    return eps * factor * ((q[:, None] * np.abs(J)).T @ np.abs(J))


if __name__ == "__main__":
    import sys
    main(sys.argv[1])

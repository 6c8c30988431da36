"""
Shared by tests/test_lsq_analytic_cpu.py and tests/test_gpu_lsq_analytic.py: the hostile particles at which the analytic
Jacobian (include/nmrfit_amd_lsq_analytic.h) is held to tests/jac_truth.py, the comparison of one point's D + 1 entries
with their truth, and the measured bar of the lock-step polish over analytic normal equations.
"""
import math

import numpy as np

from nmrfit_amd import lsq
from tests import hp_truth as hp
from tests import jac_truth as jt
from tests import lsq_support as S

# What the final objective of lsq.lm_polish over lsq.analytic_provider may differ by, relatively, from the same loop over
# lsq.rows_provider (forward differences) on the same host residual from the same start: ten times the largest gap
# measured over lsq_support.polish_cases() (tools/lsq_analytic_timing.py --cpu; profiles/lsq_analytic_timing.txt: 4.25e-14),
# capped at 1e-6 -- lsq_support.FINAL_F_BAR's rule: beyond the cap a difference is another minimum, not another Jacobian.
MEASURED_GAP = 4.25e-14
FINAL_F_BAR = min(10.0 * MEASURED_GAP, 1e-6)

T_PROBES = (0.0, 1.0, -1.0, math.sqrt(1.0 / (2.0 * math.log(2.0))), -math.sqrt(3.0), 1.0e4)
R_PROBES = (0.0, 1.0, -0.2, 1.3)
GRIDS = (("uniform", 1101), ("uniform", 8781), ("uniform", 1), ("uniform", 63), ("uniform", 64), ("uniform", 65))
PEAKS = (0, 1, 2, 5, 24)


def grid_probes(N):
    """Both sides of every tile boundary that matters: the first and last point, the first tile's end, the ragged last
    tile's start, the last segment's first point (segments of whole tiles: csrc/lsq_internal.h lsq_segments)."""
    tiles = (N + 63) // 64
    per = (tiles + 63) // 64
    nseg = (tiles + per - 1) // per
    js = {0, N - 1, 63, 64, (tiles - 1) * 64 - 1, (tiles - 1) * 64, (nseg - 1) * per * 64, N // 2}
    return sorted(j for j in js if 0 <= j < N)


def _spread(w):
    """A length in which widths and offsets are measured: the grid's span, or 1 for a grid of one point."""
    span = float(w.max() - w.min())
    return span if span > 0 else 1.0


def fillers(w, P, rng):
    span = _spread(w)
    lo = float(w.min())
    return [[rng.uniform(0.003, 0.05) * span * rng.choice([1.0, 1.0, -1.0]), lo + rng.uniform(0.0, 1.0) * span,
             rng.uniform(0.3, 1.5)] for _ in range(P)]


def particles(w, j, P, seed=0):
    """X [S x (4 + 3P)] around probe j: peak 0 placed so that the probe sees t = 0, |t| = 1, t^2 = 1/(2 ln2), t^2 = 3
    and |t| = 1e4 (the Gaussian has underflowed), then r = 0, 1, -0.2, 1.3, a = 0, a < 0, a negative width and a width
    just above the kernels' floor; the other peaks are fillers, some of negative width.  P = 0: the phase rows alone."""
    rng = np.random.default_rng(7919 * P + j + seed)
    w0, wspan = jt.frame(w)
    span = _spread(w)
    wj = float(w[j])
    if P == 0:
        return np.array([[0.5, 900.0, 0.37, 1e-3], [-2.0, 0.3, 1.3, -2e-3]])
    rest = fillers(w, P - 1, rng)

    def row(p0, p1, r, yoff, peak0):
        return np.concatenate([[p0, p1, r, yoff], peak0, np.ravel(rest)])
    X = []
    width = 0.013 * span
    for i, t in enumerate(T_PROBES):
        wd = width if abs(t) < 100 else 2.0 * 0.05 * span / abs(t)
        X.append(row(0.3 + i, -0.7 * i, 0.4, 1e-3, [wd, wj - t * wd / 2.0, 1.1]))
    for r in R_PROBES:
        X.append(row(0.1, 40.0, r, -2e-3, [width, wj - 0.3 * width, 0.9]))
    X.append(row(0.2, 1.0, 0.6, 1e-3, [width, wj + 0.2 * width, 0.0]))             # a = 0
    X.append(row(0.2, 1.0, 0.6, 1e-3, [width, wj + 0.2 * width, -0.8]))            # a < 0
    X.append(row(-1.2, 3.0, 0.3, 0.0, [-width, wj - 0.4 * width, 1.0]))            # a negative width
    loc = wj + 3.0 * span / max(w.size, 2)
    floor = 2.0 * (wspan + abs(loc - w0)) / hp.T_CAP
    X.append(row(0.0, 0.0, 0.5, 1e-3, [floor * 1.001 if floor > 0 else 1e-300, loc, 1e-12]))     # just above the floor
    X = np.stack(X)
    for x in X:
        for k in range(P):
            assert not hp.capped(float(x[4 + 3 * k]), float(x[5 + 3 * k]), w0, wspan)
    return X


def check_entries(worst, J_row, r_val, t, where):
    """The D entries of J and r at one point against their truth; returns the worst ratio of the point."""
    worst_q = 0.0
    for i, got in enumerate(J_row):
        worst_q = max(worst_q, worst["J"].check(float(got), float(t["J"][i]), float(t["tol_J"][i]), where + (jt.column_name(i),)))
    worst_q = max(worst_q, worst["r"].check(float(r_val), float(t["r"]), float(t["tol_r"]), where + ("r",)))
    return worst_q


# ---- the lock-step polish on the host -----------------------------------------------------------------------------------

def host_jacobian(sp):
    return lambda x: lsq.jacobian_host(x, *S.spectrum_tuple(sp))


def host_rows(sp):
    """(R, f) of parameter rows from the same numpy statement: what the rows launch returns, on the host."""
    w, u, v, wt = S.spectrum_tuple(sp)
    root_n = np.sqrt(w.size)

    def residual(rows):
        R = np.stack([lsq.jacobian_host(x, w, u, v, wt)[1] for x in np.atleast_2d(rows)]) * root_n
        return R, np.sqrt((R * R).sum(axis=1) / w.size)
    return residual


def polish_gap(case):
    """The relative gap of the final objective between lm_polish over analytic_provider and over rows_provider on one case
    of lsq_support.polish_cases(), both at 100 D launches: (gap, f_analytic, f_rows, start)."""
    sp, x0 = case
    lo, hi = [sp["lower"]], [sp["upper"]]
    budget = 100 * len(x0)
    Xa, fa, ia = lsq.lm_polish(lsq.analytic_provider([host_jacobian(sp)]), [x0], lo, hi, max_launches=budget)
    Xr, fr, ir = lsq.lm_polish(lsq.rows_provider([host_rows(sp)], lo, hi), [x0], lo, hi, max_launches=budget)
    return abs(fa[0] - fr[0]) / fr[0], float(fa[0]), float(fr[0]), ia["history"][0][0]


# ---- the poison driver ----------------------------------------------------------------------------------------------------

def poison_driver(out):
    """What tests/test_gpu_lsq_analytic.py runs in a fresh process per value of NMRFIT_POISON_ALLOC (the knob is read once
    per process): every output of a context call and of a ragged batch call on the analytic path -- the workspace of both
    comes from the library's one allocation helper -- into ``out``.  Host arrays start as NaN (poison_support.nan_outputs):
    a copy that came up short shows."""
    from nmrfit_amd.batch import FitBatch
    from nmrfit_amd.equations import Evaluator
    from tests import poison_support as PS
    from tests import rows_support as RS
    arrays = {}
    fits = []
    for k, (N, P) in enumerate(((1101, 5), (65, 0), (8781, 24), (700, 2), (1101, 5), (64, 1))):
        w, u, v = RS.make_grid("uniform", N, seed=80 + k)
        j = (2 * N) // 3
        wt, _ = RS.hostile_weights(N, [j], seed=90 + k)
        x = particles(w, j, P)[k % 2].copy()
        d = 0.01 * np.abs(x) + 1e-6
        fits.append(((w, u, v, wt), x, x - d, x + d))
    with PS.nan_outputs():
        for k, (spec, x, _, _) in enumerate(fits[:3]):
            with Evaluator(*spec) as ev:
                got = ev.jacobian_analytic(x, J=True, r=True, normal=True)
                for name in ("J", "r", "A", "g"):
                    arrays["ctx%d.%s" % (k, name)] = got[name]
                arrays["ctx%d.f" % k] = np.array(got["f"])
        with FitBatch([f[0] for f in fits], [f[2] for f in fits], [f[3] for f in fits], swarmsize=8,
                      seeds=list(range(1, len(fits) + 1))) as fb:
            for k, (Ab, gb, fk) in enumerate(fb.normal_equations([f[1] for f in fits], jac="analytic")):
                arrays["batch%d.A" % k], arrays["batch%d.g" % k], arrays["batch%d.f" % k] = Ab, gb, np.array(fk)
    np.savez(out, **arrays)


if __name__ == "__main__":
    import sys
    poison_driver(sys.argv[1])

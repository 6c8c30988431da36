"""
Shared by tests/test_gpu_rows_pointwise.py and tests/test_hp_truth_cpu.py: the cases at which the residual ROWS
(R[b, j] = weights[j] (data - model), both channels) are held to the pointwise truth of tests/hp_truth.py.

Nothing here builds a particle: the particles are those of tests/test_gpu_pointwise.py (peaks at the kernels' switches
around a probe point) and tests/test_gpu_pointwise_forms.py (one class of the two per-particle form switches around a
chunk), imported as they are.  What is added is what rows need: weights that are not ones, the choice of probes that
keeps a test inside its budget of truth (about 5000 peak-points a test id at ~0.8 ms each), a cache of the truths --
one hp.point serves the real row and the imaginary rows of both modes, of every kernel variant -- and the comparison of
one point of one row with its truth.

The bound is always the PLAIN one (hp.point without ``rec``): no launch that writes rows takes the Gaussian recurrence.
"""
import numpy as np

from tests import hp_truth as hp
from tests.test_gpu_pointwise import make_grid, particles, probe_points     # noqa: F401 (make_grid: for the tests)
from tests.test_gpu_pointwise_forms import (CLASSES, GRIDS, P_ROW, assert_class, assert_placements, chunk_kinds,     # noqa: F401
                                            class_particles, counts_of, probes_of)

SWITCH_KINDS = ("uniform", "descending", "nonuniform", "unsorted")
SWITCH_P = (1, 8, 9, 32, 33)              # at every probe
SWITCH_P_LARGE = (65, 130)                # at every fourth probe (as the objective's test does)
CLASS_GRIDS = ("uniform1101", "uniform8781")
X_NO_PEAK = np.array([[0.5, 900.0, 0.37, 1e-3]])     # the P = 0 row: the rotated data alone


def hostile_weights(N, probes, seed):
    """uniform(0.5, 2) with five exact zeros away from the probes and one negative value AT a probe: a row read with the
    wrong weight, a weight of the wrong index or |weight| is then seen where the truth is compared.  Returns
    (weights, indices of the zeros)."""
    rng = np.random.default_rng(seed)
    wt = rng.uniform(0.5, 2.0, N)
    probes = sorted(set(int(j) for j in probes))
    free = np.setdiff1d(np.arange(N), probes)
    zeros = np.sort(rng.choice(free, size=min(5, free.size), replace=False)) if free.size else np.zeros(0, dtype=int)
    wt[zeros] = 0.0
    neg = probes[len(probes) // 2]
    wt[neg] = -wt[neg]
    return wt, zeros


def switch_probes(N):
    """probe_points(N) thinned to the truth budget: the in-chunk positions 0, 1, 63, 64, 511 and the second chunk's
    first point, the last point, both sides of the ragged tail's start, and every other of the remaining block
    boundaries (both sides of each kept)."""
    js = probe_points(N)
    keep = {0, 1, 63, 64, 511, 512, N - 1}
    if N % hp.CHUNK:
        keep.update((N - N % hp.CHUNK - 1, N - N % hp.CHUNK))
    rest = [j for j in js if j not in keep]
    keep.update(j for i, j in enumerate(rest) if (i // 2) % 2 == 0)
    return sorted(j for j in keep if 0 <= j < N)


def switch_stacks(w, n, j):
    """{P: X} of the n-th probe j: particles() at the peak counts of the issue."""
    Xs = particles(w, j, with_large=(n % 4 == 0))
    assert set(Xs) == set(SWITCH_P + (SWITCH_P_LARGE if n % 4 == 0 else ()))
    return Xs


_TRUTH = {}


def truth(key, x, w, u, v, j):
    """hp.point(x, w, u, v, j) -- plain bound, both channels -- computed once per key (grid, probe, P, row)."""
    if key not in _TRUTH:
        t = hp.point(x, w, u, v, j)
        for name in ("dV", "dI1", "dI2", "tol_V", "tol_I1", "tol_I2"):
            assert np.isfinite(t[name]), (key, name, t[name])
        _TRUTH[key] = t
    return _TRUTH[key]


CHANNELS = {"re": ("dV", "tol_V"), "im1": ("dI1", "tol_I1"), "im2": ("dI2", "tol_I2")}


def check_point(worst, got, t, channel, wj, where):
    """One point of one row against weights[j] times the truth, within |weights[j]| times the plain bound."""
    val, tol = CHANNELS[channel]
    return worst.check(got, wj * t[val], abs(wj) * t[tol], where)


# ---- the form classes -------------------------------------------------------------------------------------------------

def class_probes(N, cls):
    """[(chunk kind, chunk, [(row, j)])] of a class test: one probe of every row (the lane varying with the row) in the
    full chunk that is first in its phase block, in one that is second (where blocks have two chunks), and in the ragged
    tail; and the two probes -- a full chunk's row that moves with the class, and the grid's last point -- that also take
    the peak counts of 64 and more."""
    out = []
    for kind, c in chunk_kinds(N).items():
        rows = {}
        for q, j in probes_of(N, c):
            rows.setdefault(q, []).append(j)
        out.append((kind, c, [(q, js[q % len(js)]) for q, js in sorted(rows.items())]))
    ci = list(CLASSES).index(cls)
    first = dict((k, p) for k, _, p in out)["first"]
    large = {first[(3 * ci + 2) % len(first)][1], N - 1}
    assert N - 1 in {j for _, _, p in out for _, j in p}
    return out, large


def class_stacks(w, c, cls, frame):
    """{P: X} of one class around chunk c, every particle asserted to be in its class and every Gaussian where its
    placement says, a priori (the conditions of tests/test_gpu_pointwise_forms.py, unchanged)."""
    stacks, seen = {}, set()
    for P in counts_of(cls):
        X, places = class_particles(w, c, cls, P, with_places=True)
        for x, pl in zip(X, places):
            assert_class(x, w, cls, frame)
            assert_placements(x, pl, w, c)
        seen.update(p_ for pl in places for p_ in pl)
        stacks[P] = X
    assert seen == set(range(5))
    return stacks


def class_grid(grid):
    return make_grid(*GRIDS[grid])

"""
CPU tier: every reference the GPU tier of the unit law leans on (tests/test_gpu_units.py) keeps the law ALONE, bit for
bit, under changes of units by powers of two (tests/units_support.py) -- the numpy and C oracles, the host swarm, the
host normal equations, the noise and quality mirrors, the weights, and the high-precision truth with its bound.  The
check that a reference is covariant is made here, not on the device: a device kernel that then breaks the law is wrong
by itself, or has a reason that its source shows.

Also one test per precondition helper of units_support.
"""
import math
import types

import numpy as np
import pytest

from nmrfit_amd import lsq, noise, quality, synth, utils
from oracle import c_oracle
from oracle import nmrfit_oracle as onp
from tests import hp_truth as hp
from tests import units_support as us
from tests.swarm_support import HostSwarm

POW2 = (us.E1, us.E2, us.E3, us.Exact("odd", 2.0 ** -9, 2.0 ** 33))


@pytest.fixture(scope="module")
def spec():
    sp = synth.make_spectrum(700, 9, seed=3, physical=True)
    sp["X"] = synth.make_swarm(sp["lower"], sp["upper"], 16, seed=4, x_true=sp["x_true"])
    return sp


def _in(sys_, sp):
    w, u, v, wt = sys_.spectrum(sp["w"], sp["u"], sp["v"], sp["weights"])
    return w, u, v, wt, sys_.params(sp["X"])


@pytest.mark.parametrize("sys_", POW2 + (us.DESC,), ids=lambda s: s.name)
@pytest.mark.parametrize("which", ["numpy", "c"])
def test_oracles_keep_the_law(spec, sys_, which):
    o = onp if which == "numpy" else c_oracle
    w, u, v, wt, X = _in(sys_, spec)
    assert us.in_range(w, u, v, X)
    f0 = o.objective_batch(spec["X"], spec["w"], spec["u"], spec["v"], spec["weights"])
    f1 = o.objective_batch(X, w, u, v, wt)
    R0 = o.residual_batch(spec["X"], spec["w"], spec["u"], spec["v"], spec["weights"])
    R1 = o.residual_batch(X, w, u, v, wt)
    if which == "c":
        R0, R1 = R0[0], R1[0]
    assert np.array_equal(f1, sys_.c * f0)
    assert np.array_equal(R1, sys_.c * R0)


@pytest.mark.parametrize("what", ["epsilon", "threshold", "float"])
def test_the_law_sees_a_constant_with_units(spec, what):
    """The instrument is sharp: an evaluation with ONE constant that has units -- an absolute epsilon of 1e-13 on a
    width, an absolute threshold of 0.05 on an area's line amplitude below which a line is dropped, a location rounded
    to float32 after an absolute offset -- breaks the exact law under E1 or E2, though each is far below every
    tolerance of the parity tests (1e-9 relative on f)."""
    def f(sys_):
        w, u, v, wt, X = _in(sys_, spec)
        X = X.copy()
        if what == "epsilon":
            X[:, 4::3] += 1e-13
        elif what == "threshold":
            al = X[:, 6::3] * X[:, 2:3] * (2.0 / X[:, 4::3]) / math.pi
            X[:, 6::3] = np.where(al > 0.05, X[:, 6::3], 0.0)
        else:
            X[:, 5::3] = (X[:, 5::3] + 1.0).astype(np.float32).astype(np.float64) - 1.0
        return onp.objective_batch(X, w, u, v, wt)
    f0 = f(us.IDENTITY)
    seen = [not np.array_equal(f(s), s.c * f0) for s in (us.E1, us.E2)]
    assert any(seen), what
    if what == "epsilon":
        assert np.max(np.abs(f(us.E1) / f0 - 1.0)) < 1e-9


def test_oracle_weights_power_of_two(spec):
    f0 = onp.objective_batch(spec["X"], spec["w"], spec["u"], spec["v"], spec["weights"])
    for k in (-20, 3, 40):
        f = onp.objective_batch(spec["X"], spec["w"], spec["u"], spec["v"], spec["weights"] * 2.0 ** k)
        assert np.array_equal(f, f0 * 2.0 ** k)


def _host_run(sp, sys_, minfunc, gens=12, S=48):
    w, u, v, wt = sys_.spectrum(sp["w"], sp["u"], sp["v"], sp["weights"])
    lo, up = sys_.box(sp["lower"], sp["upper"])
    hs = HostSwarm(lambda X: onp.objective_batch(X, w, u, v, wt), lo, up, S, seed=5, minstep=-1.0,
                   minfunc=minfunc * sys_.c)
    hs.init()
    hs.apply_global([hs.candidate()])
    for _ in range(gens):
        hs.step_local()
        hs.apply_global([hs.candidate()])
    return hs


@pytest.mark.parametrize("minfunc", [0.25, -1.0], ids=["stops", "runs"])
def test_host_swarm_keeps_the_law(spec, minfunc):
    """minstep = -1: the step norm adds squares of coordinates of unlike units (pyswarm's own rule), so it is no part of
    the law; minfunc is an intensity and scales by c."""
    a = _host_run(spec, us.IDENTITY, minfunc)
    assert (a.stop == 1) == (minfunc > 0)
    for sys_ in (us.E1, us.E2, us.E3):
        b = _host_run(spec, sys_, minfunc)
        s = sys_.pscale(a.D)
        for name in ("x", "v", "p", "g", "best_x"):
            assert np.array_equal(getattr(b, name), getattr(a, name) * s), (sys_, name)
        assert np.array_equal(b.fp, a.fp * sys_.c) and np.array_equal(b.fx, a.fx * sys_.c)
        assert (b.fg, b.best_f, b.stop, b.iteration) == (a.fg * sys_.c, a.best_f * sys_.c, a.stop, a.iteration)


def test_host_swarm_draws_are_not_covariant_under_negation(spec):
    """Why no swarm is compared across the descending twin: a box swaps its ends under a negative column scale."""
    lo, up = us.DESC.box(spec["lower"], spec["upper"])
    assert np.all(up > lo)
    a = HostSwarm(lambda X: np.zeros(len(X)), spec["lower"], spec["upper"], 8, seed=5)
    b = HostSwarm(lambda X: np.zeros(len(X)), lo, up, 8, seed=5)
    a.init()
    b.init()
    assert not np.array_equal(b.x, a.x * us.DESC.pscale(a.D))


@pytest.mark.parametrize("sys_", POW2 + (us.DESC,), ids=lambda s: s.name)
def test_normal_equations_host_keep_the_law(spec, sys_):
    x = spec["x_true"]
    rows, h = lsq.forward_rows(x, spec["lower"], spec["upper"])
    s = 1.0 / math.sqrt(spec["w"].size)
    R = onp.residual_batch(rows, spec["w"], spec["u"], spec["v"], spec["weights"])
    A, g, J, r = lsq.normal_equations_host(R, s / h, s)
    w, u, v, wt = sys_.spectrum(spec["w"], spec["u"], spec["v"], spec["weights"])
    R2 = onp.residual_batch(sys_.params(rows), w, u, v, wt)
    A2, g2, J2, r2 = lsq.normal_equations_host(R2, sys_.lsq_factors(s / h), s)
    sc = sys_.pscale(x.size)
    assert np.array_equal(r2, r * sys_.c) and np.array_equal(J2, J * (sys_.c / sc))
    Au, gu = sys_.un_normal(A2, g2)
    assert np.array_equal(Au, A) and np.array_equal(gu, g)


def test_replicas_host_keep_the_law(spec):
    u0, v0 = noise.replicas_host(spec["u"], spec["v"], 0.01, 0.02, 77)
    for sys_ in POW2:
        u1, v1 = noise.replicas_host(sys_.inten(spec["u"]), sys_.inten(spec["v"]), sys_.sigma(0.01), sys_.sigma(0.02), 77)
        assert np.array_equal(u1, sys_.c * u0) and np.array_equal(v1, sys_.c * v0)


def _regions(sp):
    loc, wd = sp["x_true"][5::3], sp["x_true"][4::3]
    return [(float(l - 2 * d), float(l + 2 * d)) for l, d in zip(loc[:4], wd[:4])]


@pytest.mark.parametrize("sys_", POW2 + (us.DESC,), ids=lambda s: s.name)
def test_residual_stats_host_keep_the_law(spec, sys_):
    x = spec["X"][1]
    reg = _regions(spec)
    Vfit = sum(onp.voigt(spec["w"], x[2], x[3], *x[4 + 3 * k:7 + 3 * k]) for k in range(9))
    dV, _ = onp.ps2(spec["u"], spec["v"], x[0], x[1])
    rows = quality.residual_stats_host(Vfit, dV, spec["w"], reg)
    w, u, v = sys_.spectrum(spec["w"], spec["u"], spec["v"])
    x2 = sys_.params(x)
    Vfit2 = sum(onp.voigt(w, x2[2], x2[3], *x2[4 + 3 * k:7 + 3 * k]) for k in range(9))
    dV2, _ = onp.ps2(u, v, x2[0], x2[1])
    assert np.array_equal(Vfit2, sys_.c * Vfit) and np.array_equal(dV2, sys_.c * dV)
    rows2 = quality.residual_stats_host(Vfit2, dV2, w, sys_.regions(reg))
    assert np.array_equal(sys_.un_quality(rows2), rows)
    assert np.array_equal(rows2[:, 7], rows[:, 7]) and np.array_equal(rows2[:, 0], rows[:, 0])


@pytest.mark.parametrize("sys_", POW2 + (us.DESC,), ids=lambda s: s.name)
def test_compute_weights_bit_identical(spec, sys_):
    """The levels are ratios of heights, the regions nearest points: the weights do not change at all."""
    def peaks(ax, c):
        return [types.SimpleNamespace(bounds=(lo * ax, hi * ax), height=pk.height * c / abs(ax))
                for pk, (lo, hi) in zip(spec["peaks"], [(p.loc - 2 * p.width, p.loc + 3 * p.width) for p in spec["peaks"]])]
    a = utils.compute_weights(spec["w"], peaks(1.0, 1.0))
    b = utils.compute_weights(sys_.grid(spec["w"]), peaks(sys_.ax, sys_.c))
    assert a.min() < a.max()
    assert np.array_equal(a, b)
    assert np.array_equal(onp.compute_weights(sys_.grid(spec["w"]), peaks(sys_.ax, sys_.c)), a)


@pytest.mark.parametrize("sys_", POW2 + (us.DESC,), ids=lambda s: s.name)
def test_truth_and_bound_keep_the_law(spec, sys_):
    """hp_truth.point and objective_probe: the value AND the tolerance scale by c, to the last bit."""
    w, u, v, _, X = _in(sys_, spec)
    for x, x2, j in ((spec["X"][0], X[0], 0), (spec["X"][3], X[3], 351), (spec["X"][7], X[7], 699)):
        t0 = hp.point(x, spec["w"], spec["u"], spec["v"], j)
        t1 = hp.point(x2, w, u, v, j)
        for key in ("V", "I", "Vf", "If1", "If2", "dV", "dI1", "dI2", "tol_V", "tol_I1", "tol_I2", "tol_Vf", "tol_If"):
            assert t1[key] == t0[key] * sys_.c, (sys_, j, key, t1[key], t0[key] * sys_.c)
        for key in ("real", "imag", "tol_real", "tol_imag"):
            assert np.array_equal(t1[key], t0[key] * sys_.c), (sys_, j, key)
        for mode in (False, True, "sum"):
            a, b = hp.objective_probe(t0, mode), hp.objective_probe(t1, mode)
            assert b == (a[0] * sys_.c, a[1] * sys_.c)


# ---- the precondition helpers -----------------------------------------------------------------------------------------

def test_same_forms_sees_the_flip(spec):
    """A 9-peak synth particle takes the pair form in the suite's units and under E1 and E2 (c = 4^14 lowers the sums of
    eight exponents by 224: still inside the budget of 250), and loses it under E3 (c = 4^-12 raises them by 192)."""
    X = spec["X"][:4]
    base, (ehi, elo) = us.forms(X, spec["w"])
    assert all(f for f, _ in base) and ehi < hp.EXP_BUDGET and elo > -hp.EXP_BUDGET
    for sys_ in (us.E1, us.E2, us.DESC):
        ok, f1, f2 = us.same_forms(X, spec["w"], sys_.params(X), sys_.grid(spec["w"]))
        assert ok.all(), (sys_, f1, f2)
    ok, f1, f2 = us.same_forms(X, spec["w"], us.E3.params(X), us.E3.grid(spec["w"]))
    assert not ok.any() and not any(f for f, _ in f2)
    _, (ehi3, _) = us.forms(us.E3.params(X), us.E3.grid(spec["w"]))
    assert ehi3 == ehi + 8 * 24


def test_in_range_sees_a_value_that_leaves(spec):
    w, u, v, X = spec["w"], spec["u"], spec["v"], spec["X"]
    assert us.in_range(w, u, v, X)
    assert not us.in_range(w, u * 2.0 ** 460, v, X)           # the square of an intensity
    bad = X.copy()
    bad[0, 6] = 2.0 ** -905
    assert not us.in_range(w, u, v, bad)                      # an area below the range
    bad = X.copy()
    bad[0, 4] = 2.0 ** 899
    assert not us.in_range(w, u, v, bad)                      # a 2/width, of a width and an area that are in range
    bad = X.copy()
    bad[0, 4] = 1e-30                                         # a width below the floor is the floor's: in range
    assert us.in_range(w, u, v, bad)


def test_exact_systems_are_what_the_law_needs():
    for s in us.EXACT:
        assert us.is_pow2(s.ax) and us.is_pow2(s.c) and s.even
    assert not us.Exact("odd", 1.0, 2.0 ** 33).even
    assert not us.is_pow2(3.7e8) and not us.is_pow2(0.0)
    x = np.arange(1.0, 14.0)
    for s in us.EXACT:
        assert np.array_equal(s.un_params(s.params(x)), x)
        lo, up = s.box(x, x + 1.0)
        assert np.all(up > lo)
    assert (us.E2.ax, us.E2.c, us.E3.ax, us.E3.c, us.DESC.ax) == (2.0 ** 14, 2.0 ** 28, 2.0 ** -10, 2.0 ** -24, -128.0)


def test_physical_systems_map_the_axis():
    s = np.linspace(0.0, 1.0, 11)
    assert np.allclose(us.P1.grid(3.0 + s), 185.0 - 25.0 * s, rtol=1e-15)
    assert np.allclose(us.P2.grid(3.0 + s), 2.5e4 + 2.4e4 * s, rtol=1e-15)
    assert np.allclose(us.P3.grid(3.0 + s), 1e-3 * (3.0 + s), rtol=1e-15)
    x = np.array([0.1, 0.2, 0.5, 0.01, 0.02, 3.5, 2.0])
    y = us.P1.params(x)
    assert np.allclose(y, [0.1, 0.2, 0.5, 3.7e6, 0.5, 172.5, 2.0 * 25 * 3.7e8])

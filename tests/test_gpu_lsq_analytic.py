"""
GPU tier of the analytic Jacobian (include/nmrfit_amd_lsq_analytic.h, csrc/lsq_analytic.hip).

    pointwise     J and r of nmrfit_jacobian_analytic at hostile particles against tests/jac_truth.py, err/tol <= 1 at every
                  probe: six grids (N = 1101: a ragged last tile, one tile per segment; N = 8781: three tiles per segment, 46
                  segments, a ragged last segment; N = 1, 63, 64, 65), P = 0, 1, 2, 5, 24, hostile weights
    refusals      a width of zero, a capped width, NaN, P = 25, a null x; the context then returns the bits it returned before
    sums          A and g against the exactly summed products of the RETURNED J and r, f against the exactly summed squares
                  of the returned r, A symmetric bit for bit
    one order     the same bits on two calls, on a lone context and in a batch ragged in N and P at either end of it, with
                  every fit a group of its own, and under the poison knob
    better        the analytic J inside its bound where the forward-difference J's error is printed in the same units
    polish        FitBatch.polish(jac="analytic") and fit_many(polish_jac="analytic")

Each test prints its worst err/tol ratios (recorded in profiles/lsq_analytic_pointwise.txt).
"""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from nmrfit_amd import _cabi, lsq, synth
from nmrfit_amd.equations import Evaluator
from tests import hp_truth as hp
from tests import jac_truth as jt
from tests import lsq_analytic_support as A
from tests import lsq_support as S
from tests import rows_support as RS

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    assert _cabi.device_count() >= 1


def worsts(name):
    return {"J": hp.Worst(name + "/J"), "r": hp.Worst(name + "/r")}


def plan(N, P):
    """(probes, particle stride) of one (grid, P): every probe and particle for P <= 2, every other probe for P = 5, two
    probes and every other particle for P = 24 -- the budget of truth, about 1500 peak-points a test id."""
    js = A.grid_probes(N)
    if P <= 2:
        return js, 1
    if P == 5:
        return js[::2] + ([js[-1]] if (len(js) - 1) % 2 else []), 1
    return sorted({js[len(js) // 2], js[-1]}), 2


@pytest.mark.parametrize("kind,N", A.GRIDS)
def test_pointwise(kind, N):
    w, u, v = RS.make_grid(kind, N, seed=N)
    probes = A.grid_probes(N)
    wt, zeros = RS.hostile_weights(N, probes, seed=N + 1)
    assert sum(wt[j] < 0 for j in probes) == 1
    worst = worsts("analytic/%s%d" % (kind, N))
    with Evaluator(w, u, v, wt) as ev:
        for P in A.PEAKS:
            js, stride = plan(N, P)
            for j in js:
                for n, x in list(enumerate(A.particles(w, j, P)))[::stride]:
                    out = ev.jacobian_analytic(x, J=True, r=True)
                    J, r = out["J"], out["r"]
                    assert J.shape == (N, x.size) and r.shape == (N,)
                    assert np.isfinite(J).all() and np.isfinite(r).all(), (N, P, j, n)
                    assert not J[zeros].any() and not r[zeros].any(), (N, P, j, n)      # a weight of zero: a row of zeros, exactly
                    if P and n == 5:       # |t| = 1e4: the Gaussian has underflowed, the peak's Lorentzian is all there is
                        assert r[j] != 0.0 and J[j, 6] != 0.0
                    A.check_entries(worst, J[j], r[j], jt.point(x, w, u, v, wt, j), (N, P, j, n))
    fails = worst["J"].report() + worst["r"].report()
    assert not fails, fails[:5]


def _case(N, P, seed, particle=0):
    """A spectrum with hostile weights, a point of the hostile particles and a box round it."""
    w, u, v = RS.make_grid("uniform", N, seed=seed)
    j = min(N - 1, (2 * N) // 3)
    wt, _ = RS.hostile_weights(N, [j], seed=seed + 1)
    x = A.particles(w, j, P)[particle].copy()
    d = 0.01 * np.abs(x) + 1e-6
    return dict(spec=(w, u, v, wt), x=x, lower=x - d, upper=x + d, j=j)


def test_refusals():
    c = _case(1101, 2, seed=3)
    w, u, v, wt = c["spec"]
    w0, wspan = hp.grid_frame(w)
    L = _cabi.lib()
    with Evaluator(w, u, v, wt) as ev:
        before = ev.jacobian_analytic(c["x"], J=True, r=True, normal=True)

        def refused(x, code, what):
            with pytest.raises(_cabi.NmrfitError) as ei:
                ev.jacobian_analytic(x, J=True, normal=True)
            assert ei.value.code == code, (what, ei.value)
            return str(ei.value)
        x = c["x"].copy()
        x[7] = 0.0
        assert "peak 1" in refused(x, _cabi.E_INVALID, "width 0")
        x = c["x"].copy()
        x[4] = 1.9 * (wspan + abs(x[5] - w0)) / hp.T_CAP                 # below the floor: capped
        assert hp.capped(x[4], x[5], w0, wspan)
        assert "peak 0" in refused(x, _cabi.E_INVALID, "capped width")
        x = c["x"].copy()
        x[2] = np.nan
        refused(x, _cabi.E_INVALID, "NaN")
        x[2] = np.inf
        refused(x, _cabi.E_INVALID, "inf")
        refused(np.concatenate([c["x"][:4], np.tile(c["x"][4:7], 25)]), _cabi.E_UNSUPPORTED, "P = 25")
        out = np.empty(1)
        assert L.nmrfit_jacobian_analytic(ev.handle, 2, None, None, None, None, None, _cabi.ptr(out)) == _cabi.E_INVALID
        after = ev.jacobian_analytic(c["x"], J=True, r=True, normal=True)
        for k in ("J", "r", "A", "g"):
            np.testing.assert_array_equal(after[k], before[k], err_msg=k)
        assert after["f"] == before["f"]


def exact_norm(r):
    """sqrt(sum_j r_j^2) from the EXACT sum of the exact squares, rounded once."""
    p, e = S.two_product(r, r)
    return math.sqrt(math.fsum(np.concatenate((p, e)).tolist()))


@pytest.mark.parametrize("N,P", [(1101, 24), (8781, 2), (65, 5), (1, 1), (8781, 0)])
def test_sums(N, P):
    """A and g against lsq_support.exact_normal_equations of the returned J and r within lsq_support.sum_bound; f against
    the exactly summed squares of the returned r within f (sum_bound(N, 1) + 4 u) -- one sum of N squares within sum_bound
    of the exact one, and a root; A symmetric bit for bit."""
    worst = {k: hp.Worst("analytic/sums/%d/%d/%s" % (N, P, k)) for k in ("A", "g", "f")}
    for particle in (0, 8) if P else (0, 1):
        c = _case(N, P, seed=N + P, particle=particle)
        with Evaluator(*c["spec"]) as ev:
            out = ev.jacobian_analytic(c["x"], J=True, r=True, normal=True)
        J, r, Ad, gd, f = out["J"], out["r"], out["A"], out["g"], out["f"]
        np.testing.assert_array_equal(Ad, Ad.T)
        Ae, ge, absA, absg = S.exact_normal_equations(J, r)
        D = J.shape[1]
        for a in range(D):
            worst["g"].check(gd[a], ge[a], S.sum_bound(N, absg[a]), (particle, a))
            for b in range(a, D):
                worst["A"].check(Ad[a, b], Ae[a, b], S.sum_bound(N, absA[a, b]), (particle, a, b))
        worst["f"].check(f, exact_norm(r), f * (S.sum_bound(N, 1.0) + 4 * S.U), (particle,))
        assert np.isfinite(f) and f > 0
    fails = [x for wo in worst.values() for x in wo.report()]
    assert not fails, fails[:5]


# ---- one order ----------------------------------------------------------------------------------------------------------

# every fit's per-segment sums exceed half a MiB of doubles: with NMRFIT_LSQ_WORKSPACE_MB=1 every fit is a group of its own
ORDER_FITS = ((8781, 24), (8000, 23), (4500, 24))
ORDER = (0, 1, 2, 0, 2, 1, 0)            # seven fits: two parts (a batch splits from K = 6); fit 0 at either end


def _segment_sums(N, P):
    tiles = (N + 63) // 64
    per = (tiles + 63) // 64
    D = 4 + 3 * P
    return ((tiles + per - 1) // per) * (D * (D + 1) // 2 + D + 1)


@pytest.fixture(scope="module")
def order_fits():
    assert all(2 * _segment_sums(N, P) > (1 << 17) for N, P in ORDER_FITS)
    return [_case(N, P, seed=50 + k, particle=(0, 9, 12)[k]) for k, (N, P) in enumerate(ORDER_FITS)]


def test_one_order(order_fits, monkeypatch):
    from nmrfit_amd.batch import FitBatch
    fits = order_fits
    lone = []
    for c in fits:
        with Evaluator(*c["spec"]) as ev:
            a = ev.jacobian_analytic(c["x"], J=True, r=True, normal=True)
            b = ev.jacobian_analytic(c["x"], J=True, r=True, normal=True)
            for k in ("J", "r", "A", "g"):
                np.testing.assert_array_equal(a[k], b[k], err_msg="two calls: " + k)
            assert a["f"] == b["f"]
            only = ev.jacobian_analytic(c["x"], normal=True)                     # (no J, no r asked for: the same sums)
            np.testing.assert_array_equal(only["A"], a["A"])
            ev.set_variant(_cabi.VARIANT_FARFIELD)                               # (no objective kernel is launched)
            far = ev.jacobian_analytic(c["x"], normal=True)
            np.testing.assert_array_equal(far["g"], a["g"])
        assert np.isfinite(a["A"]).all() and a["A"].any() and a["g"].any()
        lone.append(a)
    X = [fits[k]["x"] for k in ORDER]
    for fit_im in (False, "sum"):        # a batch with a fit_im mode is served its real channel
        with FitBatch([fits[k]["spec"] for k in ORDER], [fits[k]["lower"] for k in ORDER], [fits[k]["upper"] for k in ORDER],
                      swarmsize=8, seeds=list(range(1, len(ORDER) + 1)), fit_im=fit_im) as fb:
            for budget in (None, "1"):
                if budget:
                    monkeypatch.setenv("NMRFIT_LSQ_WORKSPACE_MB", budget)
                else:
                    monkeypatch.delenv("NMRFIT_LSQ_WORKSPACE_MB", raising=False)
                got = fb.normal_equations(X, jac="analytic")
                for i, ((Ab, gb, fk), k) in enumerate(zip(got, ORDER)):
                    np.testing.assert_array_equal(Ab, lone[k]["A"], err_msg="A of fit %d (position %d), budget %s" % (k, i, budget))
                    np.testing.assert_array_equal(gb, lone[k]["g"], err_msg="g of fit %d (position %d), budget %s" % (k, i, budget))
                    assert fk == lone[k]["f"], (k, i, budget)
            # a refused call leaves the batch as it was
            bad = [x.copy() for x in X]
            bad[-1][4] = 0.0
            with pytest.raises(_cabi.NmrfitError) as ei:
                fb.normal_equations(bad, jac="analytic")
            assert ei.value.code == _cabi.E_INVALID and "fit 6" in str(ei.value)
            again = fb.normal_equations(X, jac="analytic")
            np.testing.assert_array_equal(again[-1][0], lone[ORDER[-1]]["A"])
            with pytest.raises(ValueError):
                fb.normal_equations(X, channels="both", jac="analytic")


def test_poisoned_allocations_change_no_bit(tmp_path):
    """The driver of tests/lsq_analytic_support.py -- a context call and a ragged batch call in a fresh process, where the
    knob is read -- with NMRFIT_POISON_ALLOC unset, 255 (every fresh double a NaN) and 63: the three files byte-identical."""
    files = []
    for poison in (None, "255", "63"):
        env = dict(os.environ)
        env.pop("NMRFIT_POISON_ALLOC", None)
        if poison:
            env["NMRFIT_POISON_ALLOC"] = poison
        out = str(tmp_path / ("poison_%s.npz" % poison))
        run = subprocess.run([sys.executable, "-m", "tests.lsq_analytic_support", out], cwd=ROOT, env=env, capture_output=True,
                             text=True, timeout=300)
        assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]
        files.append(np.load(out))
    keys = sorted(files[0].files)
    assert len(keys) >= 8
    for other in files[1:]:
        assert sorted(other.files) == keys
        for k in keys:
            assert files[0][k].tobytes() == other[k].tobytes(), k
            assert np.isfinite(files[0][k]).all(), k


def test_better_than_forward_differences():
    """At every probed entry the analytic J is within its bound; the forward-difference J of the same point (scipy's step)
    is printed in units of the same bound -- no assertion on the latter."""
    w, u, v = RS.class_grid("uniform1101")
    N = w.size
    probes = A.grid_probes(N)
    wt, _ = RS.hostile_weights(N, probes, seed=77)
    worst = worsts("analytic/better")
    fd = hp.Worst("forward differences, in units of the analytic bound")
    s = 1.0 / np.sqrt(N)
    with Evaluator(w, u, v, wt) as ev:
        for j in probes[::2]:
            for n, x in list(enumerate(A.particles(w, j, 2)))[:11]:
                t = jt.point(x, w, u, v, wt, j)
                out = ev.jacobian_analytic(x, J=True, r=True)
                A.check_entries(worst, out["J"][j], out["r"][j], t, (j, n))
                rows, h = lsq.forward_rows(x)
                Jf = ev.jacobian(rows, s / h, s, J=True)["J"]
                for i in range(x.size):
                    fd.check(float(Jf[j, i]), float(t["J"][i]), float(t["tol_J"][i]), (j, n, jt.column_name(i)))
    fails = worst["J"].report() + worst["r"].report()
    print("%s: worst err/tol %.3g at %s" % (fd.name, fd.ratio, fd.where))
    assert not fails, fails[:5]


# ---- polish -------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def five():
    return [synth.make_spectrum(1024, 1 + k % 3, seed=60 + k, physical=True) for k in range(5)]


def test_batch_polish_with_the_analytic_jacobian(five):
    from nmrfit_amd.batch import FitBatch
    specs = five
    with FitBatch([S.spectrum_tuple(sp) for sp in specs], [sp["lower"] for sp in specs], [sp["upper"] for sp in specs],
                  swarmsize=64, seeds=[3 + k for k in range(5)]) as fb:
        fb.run(100, 10)
        budget = 100 * max(fb.D)
        forward = fb.polish(max_launches=budget)
        res = fb.polish(max_launches=budget, jac="analytic")
        info = fb.last_polish
        opening = fb.normal_equations([np.clip(x, sp["lower"], sp["upper"]) for (x, _), sp in zip(fb.best(), specs)])
        closing = fb.normal_equations([x for x, _ in res])
        with pytest.raises(ValueError):
            fb.polish(channels="both", jac="analytic")
    for k, (sp, (x, f), (xf, ff)) in enumerate(zip(specs, res, forward)):
        f0 = opening[k][2]
        gap = abs(f - ff) / ff
        print("fit %d: start %.9g  analytic %.17g (%s, %d accepted, kept start: %s)  2-point %.17g  relative gap %.3g"
              % (k, f0, f, info["stop"][k], info["accepted"][k], info["kept_start"][k], ff, gap))
        assert f <= f0, (k, f, f0)                                    # never above its start
        assert f == closing[k][2], (k, f, closing[k][2])              # the rows launch's value at the returned x, bit for bit
        assert np.all(x >= sp["lower"]) and np.all(x <= sp["upper"])
        assert gap <= A.FINAL_F_BAR, (k, gap, A.FINAL_F_BAR)


def test_fit_many_polish_jac(five):
    import nmrfit_amd

    def jobs(polish):
        return [dict(data=synth.SynthData(sp["w"], sp["u"], sp["v"], sp["peaks"]), lower=list(sp["lower"]), upper=list(sp["upper"]),
                     options={"swarmsize": 64, "maxiter": 100, "seed": 3 + k, "polish": polish}) for k, sp in enumerate(five)]
    plain = nmrfit_amd.fit_many(jobs(False))
    many = nmrfit_amd.fit_many(jobs(True), batch_polish=True, polish_jac="analytic")
    per_fit = nmrfit_amd.fit_many(jobs(True)[:2], polish_jac="analytic")          # (the per-fit path: lsq.polish(jac="analytic"))
    for k, (a, c) in enumerate(zip(plain, many)):
        print("fit %d: swarm %.9g  polished %.9g" % (k, a.error, c.error))
        assert c.error <= a.error, (k, c.error, a.error)
        assert np.all(c.params >= c.lower) and np.all(c.params <= c.upper)
    assert any(c.error < a.error for a, c in zip(plain, many))
    for a, c in zip(plain, per_fit):
        assert c.error <= a.error
    with pytest.raises(ValueError):
        nmrfit_amd.fit_many(jobs(True), batch_polish="both", polish_jac="analytic")

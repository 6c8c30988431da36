"""
CPU tier of the device-side least-squares pieces (csrc/lsq.hip, include/nmrfit_amd_lsq.h): the numpy statement of the
normal equations against exactly summed truth, the lock-step Levenberg-Marquardt loop (lsq.lm_polish) on the C
restatement of the residual -- bounds, monotone objective, flipped steps, a singular system -- its minimum against scipy
TRF's, and the header against its ctypes table.  No GPU.
"""
import fractions
import os
import re

import numpy as np
import pytest

from tests import lsq_support as S
from nmrfit_amd import _cabi, lsq, synth
from oracle import c_oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def oracle_rows(sp):
    return lambda rows: c_oracle.residual_batch(rows, *S.spectrum_tuple(sp))


@pytest.fixture(scope="module")
def cases():
    return S.polish_cases()


@pytest.fixture(scope="module")
def polished(cases):
    """lm_polish on the three cases as ONE lock-step problem, default settings (30 launches)."""
    lowers, uppers = [sp["lower"] for sp, _ in cases], [sp["upper"] for sp, _ in cases]
    seen = []
    inner = lsq.rows_provider([oracle_rows(sp) for sp, _ in cases], lowers, uppers)

    def provider(X):
        seen.append([None if x is None else np.array(x) for x in X])
        return inner(X)
    X, f, info = lsq.lm_polish(provider, [x0 for _, x0 in cases], lowers, uppers)
    return X, f, info, seen


def test_two_product_truth_is_the_rational_sum():
    """The exact sums the bounds are checked against (lsq_support.exact_normal_equations), on a small case against
    Python's rationals."""
    rng = np.random.default_rng(3)
    J = rng.standard_normal((37, 3)) * 10.0 ** rng.integers(-6, 6, (37, 3))
    r = rng.standard_normal(37)
    A, g, absA, absg = S.exact_normal_equations(J, r)
    F = fractions.Fraction
    for i in range(3):
        for k in range(3):
            assert A[i, k] == float(sum(F(a) * F(b) for a, b in zip(J[:, i], J[:, k])))
            exact_abs = float(sum(abs(F(a) * F(b)) for a, b in zip(J[:, i], J[:, k])))
            assert exact_abs * (1 - 200 * S.U) <= absA[i, k] <= exact_abs         # a lower estimate, and a close one
        assert g[i] == float(sum(F(a) * F(b) for a, b in zip(J[:, i], r)))
        exact_abs = float(sum(abs(F(a) * F(b)) for a, b in zip(J[:, i], r)))
        assert exact_abs * (1 - 200 * S.U) <= absg[i] <= exact_abs


@pytest.mark.parametrize("P, N", [(1, 700), (3, 1024)])
def test_normal_equations_host_within_the_derived_bound_of_exact_sums(P, N):
    """|A - A_exact| <= 1.01 (N + 1) 2^-53 sum_j |J_ji J_jk|, and g likewise: holds for any summation order, with or
    without FMA (lsq_support.sum_bound), so for numpy's here and for the device's in tests/test_gpu_lsq_batch.py."""
    sp = synth.make_spectrum(N, P, seed=21 + P, physical=True)
    x = S.perturbed_start(sp, 5)
    rows, h = lsq.forward_rows(x, sp["lower"], sp["upper"])
    R, _ = oracle_rows(sp)(rows)
    s = 1.0 / np.sqrt(N)
    A, g, J, r = lsq.normal_equations_host(R, s / h, s)
    assert J.shape == (N, 4 + 3 * P) and J.flags.c_contiguous
    np.testing.assert_array_equal(r, R[0] * s)
    np.testing.assert_array_equal(J, ((R[1:] - R[0]) * (s / h[:, None])).T)
    Ax, gx, absA, absg = S.exact_normal_equations(J, r)
    print("max |A - exact| / bound %.3g, g %.3g" % (np.max(np.abs(A - Ax) / S.sum_bound(N, absA)),
                                                    np.max(np.abs(g - gx) / S.sum_bound(N, absg))))
    assert np.all(np.abs(A - Ax) <= S.sum_bound(N, absA))
    assert np.all(np.abs(g - gx) <= S.sum_bound(N, absg))


def test_lm_polish_respects_bounds_and_never_raises_f(cases, polished):
    X, f, info, seen = polished
    assert info["launches"] <= 30 and len(seen) == info["launches"]
    for k, (sp, x0) in enumerate(cases):
        lo, hi = np.asarray(sp["lower"]), np.asarray(sp["upper"])
        for trial in seen:                      # every point ever evaluated lies in the box
            if trial[k] is not None:
                assert np.all(trial[k] >= lo) and np.all(trial[k] <= hi)
        assert np.all(X[k] >= lo) and np.all(X[k] <= hi)
        hist = info["history"][k]
        assert all(b <= a for a, b in zip(hist, hist[1:])), hist
        f0 = c_oracle.objective_batch(x0, *S.spectrum_tuple(sp))[0]
        assert hist[0] == pytest.approx(f0, rel=1e-12)
        assert f[k] == hist[-1] < 0.5 * f0      # (the starts are 2 % of the box off: the polish has work to do)
        assert f[k] == pytest.approx(c_oracle.objective_batch(X[k], *S.spectrum_tuple(sp))[0], rel=1e-12)
        assert info["stop"][k] in ("ftol", "lambda", "budget", "frozen")


def test_lm_polish_in_lock_step_equals_the_fits_alone(cases, polished):
    """K problems in one loop are K independent problems: each ends where it ends alone."""
    X, f, info, _ = polished
    sp, x0 = cases[1]
    Xa, fa, _ = lsq.lm_polish(lsq.rows_provider([oracle_rows(sp)], [sp["lower"]], [sp["upper"]]), [x0], [sp["lower"]],
                              [sp["upper"]])
    np.testing.assert_array_equal(Xa[0], X[1])
    assert fa[0] == f[1]


def test_start_on_the_upper_bound_takes_flipped_steps():
    sp = synth.make_spectrum(1024, 2, seed=42, physical=True)
    lo, hi = np.asarray(sp["lower"], float), np.asarray(sp["upper"], float)
    x0 = hi.copy()
    rows, h = lsq.forward_rows(x0, lo, hi)
    assert np.all(h < 0) and np.all(rows >= lo) and np.all(rows <= hi)      # every c_i = s / h_i is negative
    f0 = c_oracle.objective_batch(x0, *S.spectrum_tuple(sp))[0]
    X, f, info = lsq.lm_polish(lsq.rows_provider([oracle_rows(sp)], [lo], [hi]), [x0], [lo], [hi])
    assert np.all(X[0] >= lo) and np.all(X[0] <= hi)
    assert f[0] < f0 and info["accepted"][0] >= 1
    assert np.any(X[0] < hi)                   # it left the corner


def test_singular_system_terminates_inside_the_budget():
    """physical=False: the imaginary channel is noise, the phase is degenerate with the areas -- the scaled A is
    singular to working precision.  The loop must end within its launches with f <= f0."""
    sp = synth.make_spectrum(1024, 2, seed=44, physical=False)
    x0 = S.perturbed_start(sp, 45)
    calls = []
    inner = lsq.rows_provider([oracle_rows(sp)], [sp["lower"]], [sp["upper"]])

    def provider(X):
        calls.append(1)
        return inner(X)
    X, f, info = lsq.lm_polish(provider, [x0], [sp["lower"]], [sp["upper"]], max_launches=12)
    f0 = c_oracle.objective_batch(x0, *S.spectrum_tuple(sp))[0]
    assert len(calls) == info["launches"] <= 12
    assert f[0] <= f0 * (1 + 1e-12) and np.isfinite(f[0])
    # a system that IS singular (a zero row and column) raises lambda instead of failing
    A = np.diag([1.0, 0.0, 2.0])

    def flat(X):
        return [None if x is None else (A, np.array([1.0, 0.0, -1.0]), 1.0) for x in X]
    X, f, info = lsq.lm_polish(flat, [np.zeros(3)], [-np.ones(3)], [np.ones(3)], max_launches=50)
    assert info["stop"][0] == "lambda" and info["launches"] <= 50 and f[0] == 1.0 and np.all(X[0] == 0.0)


def test_same_minimum_as_scipy_trf(cases):
    """Both descend the same smooth function from the same start; each gets scipy's default budget of 100 D evaluations
    (the one-peak case is a curved valley in (p0, p1): TRF itself takes about 120 there).  The final objectives agree
    within lsq_support.FINAL_F_BAR -- ten times the gap measured here (profiles/lsq_timing.txt), with TRF at lm_polish's
    own tolerance (lsq_support.TRF_TOL: at scipy's default 1e-8 TRF stops 1.4e-6 above this minimum on the one-peak
    case, which is its own stopping rule and not another minimum)."""
    worst = 0.0
    for sp, x0 in cases:
        res = oracle_rows(sp)
        D = len(x0)
        X, f, info = lsq.lm_polish(lsq.rows_provider([res], [sp["lower"]], [sp["upper"]]), [x0], [sp["lower"]], [sp["upper"]],
                                   max_launches=100 * D)
        xt, ft = S.trf_on_rows(res, x0, sp["lower"], sp["upper"])
        gap = abs(f[0] - ft) / ft
        worst = max(worst, gap)
        print("P = %d: lm %.17g (%d launches, %s)  trf %.17g  relative gap %.3g" % ((D - 4) // 3, f[0], info["launches"],
                                                                                   info["stop"][0], ft, gap))
        assert gap <= S.FINAL_F_BAR, (gap, S.FINAL_F_BAR)
    assert S.FINAL_F_BAR <= 1e-6 and S.FINAL_F_BAR == pytest.approx(min(10 * S.MEASURED_GAP, 1e-6))


def _declared(header):
    text = open(os.path.join(ROOT, "include", header)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return set(re.findall(r"\b(nmrfit_[a-z0-9_]+)\s*\(", text))


def test_lsq_header_has_its_own_ctypes_table():
    names = _declared("nmrfit_amd_lsq.h")
    assert names == set(_cabi.LSQ_SIGNATURES) == {"nmrfit_jacobian", "nmrfit_batch_normal_equations"}
    product = _declared("nmrfit_amd.h")
    assert len(product) == 46 and not (names & product)          # the product header stays as thin as it is
    assert not (names & set(_cabi.ALL_SIGNATURES)) and not (names & set(_cabi.PREP_SIGNATURES))
    L = _cabi.lib()
    for n in names:
        assert getattr(L, n).argtypes == _cabi.LSQ_SIGNATURES[n]
    text = open(os.path.join(ROOT, "include", "nmrfit_amd_lsq.h")).read()
    assert "#define NMRFIT_LSQ_MAX_D %d\n" % _cabi.LSQ_MAX_D in text


def test_null_arguments_are_refused_without_a_gpu():
    L = _cabi.lib()
    assert L.nmrfit_jacobian(None, 1, None, None, 1.0, None, None, None, None, None) == _cabi.E_INVALID
    assert b"null context" in L.nmrfit_last_error()
    assert L.nmrfit_batch_normal_equations(None, None, None, None, None, None, None) == _cabi.E_INVALID
    assert b"null batch handle" in L.nmrfit_last_error()


def test_batch_polish_is_fit_manys_own_argument(monkeypatch):
    """The flag reaches the batch read-back in fit_many's call record and nothing else; without it the record is the
    plain call's."""
    from nmrfit_amd import core
    got = []

    def fake_local(jobs, call):
        got.append((call.device_weights, call.batch_polish))
        return []
    monkeypatch.setattr(core, "_fit_many_local", fake_local)
    core.fit_many([], batch_polish=True)
    core.fit_many([])
    core.fit_many([], device_weights=True, batch_polish=True)
    assert got == [(False, True), (False, False), (True, True)]

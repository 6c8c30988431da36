"""
CPU tier of least squares on both channels (include/nmrfit_amd_lsq_im.h, lsq.combine_channels): the header against its
ctypes table, the combined gradient against a central difference of the objective in closed form, H symmetric positive
semi-definite, a channel at zero dropping out, one channel alone reproducing today's normal equations and step, and the
lock-step loop over the combined host provider -- monotone, and how far its end is from a long run's
(lsq_im_support.MEASURED_GAP_IM).  No GPU.
"""
import os
import re

import numpy as np
import pytest

from nmrfit_amd import _cabi, lsq, synth
from tests import lsq_im_support as M
from tests import lsq_support as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 2.0 ** -52


def _declared(header):
    text = open(os.path.join(ROOT, "include", header)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return set(re.findall(r"\b(nmrfit_[a-z0-9_]+)\s*\(", text))


def test_lsq_im_header_has_its_own_ctypes_table():
    names = _declared("nmrfit_amd_lsq_im.h")
    assert names == set(_cabi.LSQ_IM_SIGNATURES) == {"nmrfit_residual_batch_im", "nmrfit_jacobian_im",
                                                     "nmrfit_batch_normal_equations_im"}
    for other in (_cabi.ALL_SIGNATURES, _cabi.PREP_SIGNATURES, _cabi.LSQ_SIGNATURES):
        assert not (names & set(other))
    for header in ("nmrfit_amd.h", "nmrfit_amd_diag.h", "nmrfit_amd_prep.h", "nmrfit_amd_lsq.h"):
        assert not (names & _declared(header)), header
    L = _cabi.lib()
    for n in names:
        assert getattr(L, n).argtypes == _cabi.LSQ_IM_SIGNATURES[n]
        assert getattr(L, n).restype is not None
    assert L.nmrfit_abi_version() == _cabi.ABI_VERSION == 6         # found by symbol lookup: the version does not move


def test_null_arguments_are_refused_without_a_gpu():
    L = _cabi.lib()
    assert L.nmrfit_residual_batch_im(None, 1, 1, None, 1, None, None) == _cabi.E_INVALID
    assert b"null context" in L.nmrfit_last_error()
    assert L.nmrfit_jacobian_im(None, 1, None, None, 1.0, 1, None, None, None, None, None) == _cabi.E_INVALID
    assert b"null context" in L.nmrfit_last_error()
    assert L.nmrfit_batch_normal_equations_im(None, None, None, None, None, None, None) == _cabi.E_INVALID
    assert b"null batch handle" in L.nmrfit_last_error()


def _parts(sp, x, mode):
    rows, h = lsq.forward_rows(x, sp["lower"], sp["upper"])
    R_re, R_im, f2 = M.residual_rows(rows, *S.spectrum_tuple(sp), mode)
    s = 1.0 / np.sqrt(R_re.shape[1])
    return lsq.normal_equations_host_im(R_re, R_im, s / h, s), f2, rows, h


@pytest.mark.parametrize("mode", M.MODES)
@pytest.mark.parametrize("P", [1, 2, 3])
def test_combined_gradient_is_the_objectives(P, mode):
    """grad . d of combine_channels against (f(x + tau d) - f(x - tau d)) / (2 tau) of the closed-form objective, along
    random d = box * U(-1, 1), tau = 1e-5.  The tolerance is the sum of what each side can be off by, all of it from the
    steps and from the closed form itself (nothing from combine_channels):
      * central difference, truncation: tau^2/6 |g'''|, g(t) = f(x + t d), g''' from a five-point stencil of step 1e-3,
        doubled (the stencil's own error);
      * central difference, rounding: two values of f, each within C eps ||m|| (lsq_im_support.magnitudes; C = 32 as in
        tests/hp_truth.py), over 2 tau;
      * forward-difference Jacobian, truncation: J_ch's column i is r_ch' + (h_i/2) r_ch'' + ..., so the gradient's
        component i is off by at most (|h_i|/2) (||d2 r_re/dx_i^2|| + ||d2 r_im/dx_i^2||)/2 (Cauchy-Schwarz with the unit
        vector r/rho), the second derivatives from central second differences of the closed form, step 1e-4 of the box;
      * forward-difference Jacobian, rounding: two residual vectors, each within C eps ||m||, over |h_i|, per channel."""
    N = 1024
    sp = synth.make_spectrum(N, P, seed=40 + P, physical=True)
    lo, hi = np.asarray(sp["lower"], float), np.asarray(sp["upper"], float)
    x = S.perturbed_start(sp, 50 + P)
    parts, f2, rows, h = _parts(sp, x, mode)
    H, grad, f = lsq.combine_channels(parts)
    assert f == 0.5 * (parts["re"][2] + parts["im"][2])
    assert f == pytest.approx(f2[0].mean(), rel=1e-14) and f == pytest.approx(M.objective(x, sp, mode), rel=1e-14)
    mnorm = M.magnitudes(x, *S.spectrum_tuple(sp))
    C = 32.0

    def resid(y):
        R_re, R_im, _ = M.residual_rows(y, *S.spectrum_tuple(sp), mode)
        return R_re[0] / np.sqrt(N), R_im[0] / np.sqrt(N)
    second = np.empty(x.size)                     # (||r_re,ii|| + ||r_im,ii||) / 2
    for i in range(x.size):
        d = np.zeros(x.size)
        d[i] = 1e-4 * (hi[i] - lo[i])
        (ap, bp), (a0, b0), (am, bm) = resid(x + d), resid(x), resid(x - d)
        second[i] = 0.5 * (np.linalg.norm(ap - 2 * a0 + am) + np.linalg.norm(bp - 2 * b0 + bm)) / d[i] ** 2
    rng = np.random.default_rng(7 * P + mode)
    tau, delta = 1e-5, 1e-3
    for trial in range(4):
        d = (hi - lo) * rng.uniform(-1.0, 1.0, x.size)
        g = lambda t: M.objective(x + t * d, sp, mode)
        central = (g(tau) - g(-tau)) / (2 * tau)
        g3 = abs(g(2 * delta) - 2 * g(delta) + 2 * g(-delta) - g(-2 * delta)) / (2 * delta ** 3)
        tol = (2 * g3 * tau * tau / 6 + C * EPS * mnorm / tau
               + float(np.sum(np.abs(d) * (np.abs(h) / 2) * second)) + float(np.sum(np.abs(d) * 2 * C * EPS * mnorm / np.abs(h))))
        got = float(grad @ d)
        print("P %d mode %d trial %d: grad.d %.12g central %.12g |diff| %.3g tol %.3g" % (P, mode, trial, got, central,
                                                                                         abs(got - central), tol))
        assert abs(got - central) <= tol
        assert tol < 1e-5                                # (derivatives along the box are 0.01 .. 1: a wrong factor cannot hide in it)


@pytest.mark.parametrize("mode", M.MODES)
def test_H_is_symmetric_positive_semidefinite_and_a_zero_channel_drops_out(mode):
    sp = synth.make_spectrum(1024, 2, seed=42, physical=True)
    x = S.perturbed_start(sp, 52)
    parts, _, _, _ = _parts(sp, x, mode)
    H, grad, f = lsq.combine_channels(parts)
    np.testing.assert_array_equal(H, H.T)
    scale = np.sqrt(np.diag(H))
    ev = np.linalg.eigvalsh(H / np.outer(scale, scale))
    assert ev.min() >= -len(x) * EPS * ev.max()             # (an eigenvalue's rounding: D eps of the largest)
    # a channel with rho = 0 (or a lost one) contributes nothing to H and the gradient; f counts it as it is
    A_re, g_re, rho_re = parts["re"]
    junk = np.full_like(A_re, 7.0)
    for rho in (0.0, np.nan, np.inf):
        H1, g1, f1 = lsq.combine_channels({"re": parts["re"], "im": (junk, junk[0], rho)})
        np.testing.assert_array_equal(H1, A_re * (0.5 / rho_re))
        np.testing.assert_array_equal(g1, g_re * (0.5 / rho_re))
        if rho == 0.0:
            assert f1 == 0.5 * rho_re
    # a sequence is taken like the dict
    H2, g2, f2 = lsq.combine_channels([parts["re"], parts["im"]])
    np.testing.assert_array_equal(H2, H)
    np.testing.assert_array_equal(g2, grad)
    assert f2 == f


def test_one_channel_is_todays_normal_equations():
    """One channel alone gives (A, g, f) times (1/(2 rho), 1/(2 rho), 1/2).  With the scalar a power of FOUR every
    operation of _lm_step commutes with it exactly (the Cholesky factor scales by its square root, a power of two), so the
    step is today's bit for bit; with rho as it comes, H and grad are today's A and g times the one rounded scalar."""
    sp = synth.make_spectrum(1024, 2, seed=42, physical=True)
    x = S.perturbed_start(sp, 52)
    lo, hi = np.asarray(sp["lower"], float), np.asarray(sp["upper"], float)
    rows, h = lsq.forward_rows(x, lo, hi)
    R_re, _, f2 = M.residual_rows(rows, *S.spectrum_tuple(sp), 2)
    s = 1.0 / np.sqrt(R_re.shape[1])
    A, g, _, r = lsq.normal_equations_host(R_re, s / h, s)
    rho = float(np.sqrt(r @ r))
    H, grad, f = lsq.combine_channels([(A, g, rho)])
    np.testing.assert_array_equal(H, A * (0.5 / rho))
    np.testing.assert_array_equal(grad, g * (0.5 / rho))
    assert f == 0.5 * rho
    scale = np.maximum(hi - lo, 1e-12)
    for rho4, k in ((0.125, 4.0), (2.0, 0.25), (0.5, 1.0)):
        H4, g4, _ = lsq.combine_channels({"re": (A, g, rho4)})
        np.testing.assert_array_equal(H4, A * k)
        np.testing.assert_array_equal(g4, g * k)
        for lam in (1e-3, 1.0, 1e3):
            want = lsq._lm_step(A, g, x, lo, hi, scale, lam)
            got = lsq._lm_step(H4, g4, x, lo, hi, scale, lam)
            assert want is not None
            np.testing.assert_array_equal(got, want)


@pytest.mark.parametrize("mode", M.MODES)
def test_lm_polish_on_both_channels(mode):
    """lsq.lm_polish over the combined host provider, P = 1, 2, 3, N = 1024, perturbed starts, as ONE lock-step problem:
    f = (rho_re + rho_im)/2 never rises, every point stays in its box, the end is the closed-form objective at the
    returned point, and its relative gap to a long run of the same loop (2000 D launches, ftol = 0) is what
    lsq_im_support.MEASURED_GAP_IM records (the largest printed here over both modes)."""
    cases = S.polish_cases()
    specs = [sp for sp, _ in cases]
    lowers, uppers = [sp["lower"] for sp in specs], [sp["upper"] for sp in specs]
    X0 = [x0 for _, x0 in cases]
    D = max(len(x) for x in X0)
    provider = M.host_provider(specs, mode)
    X, f, info = lsq.lm_polish(provider, X0, lowers, uppers, max_launches=100 * D)
    Xl, fl, infol = lsq.lm_polish(provider, X0, lowers, uppers, max_launches=2000 * D, ftol=0.0)
    worst = 0.0
    for k, (sp, x0) in enumerate(cases):
        hist = info["history"][k]
        assert all(b <= a for a, b in zip(hist, hist[1:])), hist
        assert all(b <= a for a, b in zip(infol["history"][k], infol["history"][k][1:]))
        assert hist[0] == pytest.approx(M.objective(x0, sp, mode), rel=1e-13)
        assert f[k] == hist[-1] < hist[0]                   # (the starts are 2 % of the box off: there is work to do)
        assert f[k] == pytest.approx(M.objective(X[k], sp, mode), rel=1e-13)
        assert np.all(X[k] >= sp["lower"]) and np.all(X[k] <= sp["upper"])
        gap = (f[k] - fl[k]) / fl[k]
        worst = max(worst, gap)
        print("mode %d P %d: start %.9g  end %.17g (%s, %d accepted)  long run %.17g (%s)  relative gap %.3g"
              % (mode, (len(x0) - 4) // 3, hist[0], f[k], info["stop"][k], info["accepted"][k], fl[k], infol["stop"][k], gap))
        assert gap <= M.FINAL_F_BAR_IM, (gap, M.FINAL_F_BAR_IM)
    # the recorded figure is this measurement (to the rounding of a value of 1e-3: a few 1e-16 relative), not a guess
    assert worst <= M.MEASURED_GAP_IM * 1.05 + 5e-16
    assert M.FINAL_F_BAR_IM == pytest.approx(min(10 * M.MEASURED_GAP_IM, 1e-6)) and M.FINAL_F_BAR_IM <= 1e-6


def test_residual_model_keeps_todays_default_and_fit_many_carries_the_mode(monkeypatch):
    """ResidualModel's fit_im defaults to 0; fit_many's call record carries "both" as it is and True / False as before."""
    import inspect
    from nmrfit_amd import core
    assert inspect.signature(lsq.ResidualModel.__init__).parameters["fit_im"].default == 0
    assert inspect.signature(lsq.polish).parameters["channels"].default == "real"
    got = []
    monkeypatch.setattr(core, "_fit_many_local", lambda jobs, call: got.append(call.batch_polish) or [])
    core.fit_many([], batch_polish="both")
    core.fit_many([], batch_polish=True)
    core.fit_many([])
    assert got == ["both", True, False]
    with pytest.raises(ValueError):
        lsq.polish(None, np.zeros(7), np.zeros(7), np.ones(7), fit_im=False, channels="both")

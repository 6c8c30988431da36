"""
GPU tier of the device-batched phase correction: the three scores against the reference's values and the host
mirror, the device Nelder-Mead against scipy.optimize.fmin bit for bit, and the Python entry points
(approximate_phase_many, shift_phase_many) against the host path on the golden spectrum and on a mixed batch.
"""
import ctypes
import os

import numpy as np
import pytest
import scipy.optimize

from nmrfit_amd import _cabi, containers, proc_autophase, synth
from nmrfit_amd.containers import Data, shift_phase_many

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def g(golden_dir):
    return np.load(os.path.join(golden_dir, "data_container.npz"))


def _z(g):
    return g["u"] + 1j * g["v"]


def _ragged(Ns, seed=7):
    """spectra with a few lines and noise (a physical imaginary channel) of the given lengths"""
    rng = np.random.default_rng(seed)
    out = []
    for k, N in enumerate(Ns):
        if N >= 64:
            sp = synth.make_spectrum(N, 1 + k % 4, seed=seed + k, physical=True)
            out.append(sp["u"] + 1j * sp["v"])
        else:
            out.append(rng.standard_normal(N) + 1j * rng.standard_normal(N))
    return out


def test_scores_match_the_reference_on_the_golden_spectrum(g):
    z = _z(g)
    acme = proc_autophase.phase_scores([z], g["score_phases"], "acme")[0]
    np.testing.assert_allclose(acme, g["acme"], rtol=1e-12, atol=0)
    minima = proc_autophase.phase_scores([z], g["score_phases"], "peak_minima")[0]
    np.testing.assert_allclose(minima, g["peak_minima"], rtol=1e-12, atol=1e-15)


def test_acme_on_a_ragged_batch_matches_the_host_and_the_lone_call():
    Ns = (2, 3, 63, 64, 65, 4096, 65537)
    zs = _ragged(Ns)
    rng = np.random.default_rng(11)
    ph = rng.uniform(-1e3, 1e3, (len(Ns), 5, 2))
    ph[:, 0] = 0.0
    got = proc_autophase.phase_scores(zs, ph, "acme")
    want = np.array([[proc_autophase._ps_acme_score(p, z) for p in phk] for z, phk in zip(zs, ph)])
    rel = np.abs(got - want) / np.maximum(np.abs(want), 1e-300)
    assert np.all((got == want) | (rel <= 1e-12)), rel.max()
    for k, z in enumerate(zs):
        np.testing.assert_array_equal(proc_autophase.phase_scores([z], ph[k], "acme")[0], got[k])
    again = proc_autophase.phase_scores(zs, ph, "acme")
    np.testing.assert_array_equal(again, got)


def test_peak_minima_on_a_ragged_batch_matches_the_host():
    Ns = (2000, 4096, 65537, 1000)
    zs = _ragged(Ns, seed=3)
    ph = np.random.default_rng(5).uniform(-40, 40, (len(Ns), 4, 2))
    want = np.array([[proc_autophase._ps_peak_minima_score(p, z) for p in phk] for z, phk in zip(zs, ph)])
    got = proc_autophase.phase_scores(zs, ph, "peak_minima")
    np.testing.assert_allclose(got, want, rtol=1e-12, atol=1e-15)
    for k, z in enumerate(zs):
        np.testing.assert_array_equal(proc_autophase.phase_scores([z], ph[k], "peak_minima")[0], got[k])


def test_brute_levels_are_the_host_loops_values():
    zs = _ragged((2, 65, 4096, 12000, 30001), seed=9)
    angles = np.arange(-np.pi, np.pi, np.pi / 45)
    got = proc_autophase.brute_levels([z.real for z in zs], [z.imag for z in zs], angles)
    for k, z in enumerate(zs):
        u, v = z.real.copy(), z.imag.copy()
        n = max(1, int(len(u) / 5000))
        for m, a in enumerate(angles):
            V, _ = proc_autophase.ps2(u, v, a, 0.0)
            err = np.sqrt((V[:n].mean() - V[-n:].mean()) ** 2)
            if np.max(V) > abs(np.min(V)):
                assert got[k, m] == err, (k, m, got[k, m], err)
            else:
                assert np.isnan(got[k, m])


def _rosen(x):
    return (1 - x[0]) ** 2 + 100 * (x[1] - x[0] ** 2) ** 2


def test_device_nelder_mead_equals_scipy_fmin_bit_for_bit():
    """The optimiser alone, on an analytic score computed on the device: x, f, nfev, nit all equal scipy's.  The starts
    include zero components (the zdelt vertex), a start that meets a shrink step ([-1.45, -1.49]) and a long run."""
    starts = np.array([[-1.2, 1.0], [0.0, 0.0], [0.0, 2.5], [3.0, 0.0], [-1.45, -1.49], [-1.9, -2.46], [40.0, 30.0],
                       [1.0, 1.0], [10.0, -7.0], [1000.0, 1000.0], [-1000.0, 500.0], [1e4, -1e4]])
    S = len(starts)
    x = np.zeros((S, 2))
    f = np.zeros(S)
    nfev = np.zeros(S, dtype=np.int32)
    nit = np.zeros(S, dtype=np.int32)
    p = _cabi.ptr
    _cabi.check(_cabi.lib().nmrfit_diag_phase_nm_rosenbrock(0, S, p(np.ascontiguousarray(starts)), p(x), p(f), p(nfev), p(nit)))
    shrinks = exhausted = 0
    for k, x0 in enumerate(starts):
        xs, fs, its, fev, warn = scipy.optimize.fmin(_rosen, list(x0), disp=False, full_output=True)
        np.testing.assert_array_equal(x[k], xs)
        assert f[k] == fs and nfev[k] == fev and nit[k] == its, (k, f[k], fs, nfev[k], fev, nit[k], its)
        shrinks += fev - 3 > 2 * (its - 1)      # (an iteration with a shrink makes four calls, the others one or two)
        exhausted += warn == 1                  # maxfun reached: the call past it refused, the simplex sorted anyway
    assert shrinks >= 1 and exhausted >= 3


def test_approximate_phase_many_on_the_golden_spectrum(g):
    z = _z(g)
    x, f, nfev, nit = proc_autophase.estimate_many([z], "acme")
    xs, fs, its, fev, _ = scipy.optimize.fmin(proc_autophase._ps_acme_score, [0.0, 0.0], args=(z,), disp=False,
                                              full_output=True)
    np.testing.assert_allclose(x[0], np.asarray(g["approx_acme"]) * 180 / np.pi, rtol=0, atol=1e-8)
    assert nfev[0] == fev and nit[0] == its
    rad = proc_autophase.approximate_phase_many([z], "acme")
    np.testing.assert_allclose(rad[0], g["approx_acme"], rtol=1e-8)
    deg = proc_autophase.estimate_many([z], "peak_minima", p0=5.0, p1=-3.0)[0]
    np.testing.assert_allclose(deg[0], np.asarray(g["approx_minima"]) * 180 / np.pi, rtol=0, atol=1e-8)
    np.testing.assert_allclose(proc_autophase.approximate_phase_many([z], "peak_minima", p0=5.0, p1=-3.0)[0],
                               g["approx_minima"], rtol=1e-8)
    phased = proc_autophase.autops_many([z], "acme")[0]
    np.testing.assert_allclose(phased, g["autops_acme"], rtol=0, atol=1e-9 * np.abs(z).max())


def test_empty_peak_minima_window_raises_like_the_reference(g):
    z = _z(g).copy()
    z[10] += 1e6 * np.abs(z).max()              # the tallest point sits in the first 100 points at every phase tried
    with pytest.raises(ValueError):
        proc_autophase.approximate_phase(z, "peak_minima")
    with pytest.raises(ValueError, match="spectrum 1"):
        proc_autophase.approximate_phase_many([_z(g), z], "peak_minima")
    with pytest.raises(ValueError, match="spectrum 0"):
        proc_autophase.phase_scores([z], [[0.0, 0.0]], "peak_minima")


def test_shift_phase_many_on_the_golden_data(g):
    d = Data(g["w"], g["u"], g["v"])
    shift_phase_many([d], method="auto")
    np.testing.assert_allclose([d.p0, d.p1], g["auto_p"], rtol=1e-8)
    np.testing.assert_allclose(d.V, g["auto_V"], rtol=0, atol=1e-8 * np.abs(g["auto_V"]).max())
    shift_phase_many([d], method="brute", step=np.pi / 90)
    np.testing.assert_array_equal([d.p0, d.p1], g["brute_p"])
    np.testing.assert_array_equal(d.V, g["brute_V"])
    shift_phase_many([d], method="manual", p0=0.1, p1=-0.2)
    ref = Data(g["w"], g["u"], g["v"])
    ref.shift_phase(method="manual", p0=0.1, p1=-0.2)
    assert (d.p0, d.p1) == (ref.p0, ref.p1)
    np.testing.assert_array_equal(d.V, ref.V)
    np.testing.assert_array_equal(d.I, ref.I)


def _batch(S=64, seed=21):
    rng = np.random.default_rng(seed)
    out = []
    for k in range(S):
        N = int(rng.integers(600, 9000))
        sp = synth.make_spectrum(N, int(rng.integers(1, 7)), seed=seed + k, physical=True)
        out.append(Data(sp["w"], sp["u"], sp["v"]))
    return out


def test_shift_phase_many_on_a_mixed_batch_matches_the_lone_host_call():
    datas = _batch()
    hosts = _batch()
    for h in hosts:
        h.shift_phase(method="auto")
    shift_phase_many(datas, method="auto")
    dev_deg = np.array([[d.p0, d.p1] for d in datas]) * 180 / np.pi
    host_deg = np.array([[h.p0, h.p1] for h in hosts]) * 180 / np.pi
    diff = np.abs(dev_deg - host_deg).max(axis=1)
    print("auto: max |device - host| per spectrum (degrees): max %.3g, median %.3g, over 1e-8: %d of %d"
          % (diff.max(), np.median(diff), int((diff > 1e-8).sum()), len(diff)))
    assert diff.max() <= 2e-4
    assert np.all(diff <= 1e-8), np.flatnonzero(diff > 1e-8)
    for d, h in zip(datas, hosts):
        np.testing.assert_array_equal(d.V, proc_autophase.ps2(d.u, d.v, d.p0, d.p1)[0])
    again = _batch()
    shift_phase_many(again, method="auto")
    np.testing.assert_array_equal([[d.p0, d.p1] for d in again], [[d.p0, d.p1] for d in datas])

    for h in hosts:
        h.shift_phase(method="brute")
    shift_phase_many(datas, method="brute")
    for d, h in zip(datas, hosts):
        assert (d.p0, d.p1) == (h.p0, h.p1)
        np.testing.assert_array_equal(d.V, h.V)
        np.testing.assert_array_equal(d.I, h.I)
    shift_phase_many(again, method="brute")
    np.testing.assert_array_equal([[d.p0, d.p1] for d in again], [[d.p0, d.p1] for d in datas])


def test_estimate_on_a_batch_that_mixes_both_workgroup_sizes():
    """Spectra from 16384 points up are reduced by 512 threads, shorter ones by 256: one launch holds both, and every
    spectrum's optimisation equals its lone device call bit for bit and the host's fmin (same nfev and nit, end point
    within 1e-8 degrees)."""
    zs = _ragged((4096, 20000, 65537, 3000, 16384), seed=31)
    for fn, p0, p1 in (("acme", 0.0, 0.0), ("peak_minima", 5.0, -3.0)):
        x, f, nfev, nit = proc_autophase.estimate_many(zs, fn, p0, p1)
        for k, z in enumerate(zs):
            xs, fs, its, fev, _ = scipy.optimize.fmin(proc_autophase._SCORES[fn], [p0, p1], args=(z,), disp=False,
                                                      full_output=True)
            np.testing.assert_allclose(x[k], xs, rtol=0, atol=1e-8)
            assert nfev[k] == fev and nit[k] == its, (fn, k, nfev[k], fev, nit[k], its)
            lone = proc_autophase.estimate_many([z], fn, p0, p1)
            np.testing.assert_array_equal(lone[0][0], x[k])
            assert lone[1][0] == f[k] and lone[2][0] == nfev[k] and lone[3][0] == nit[k]


@pytest.mark.parametrize("N, i", [(50, 30), (80, 79), (99, 1), (50, 0), (150, 60), (150, 120), (2, 1)])
def test_peak_minima_window_slices_like_python_on_short_spectra(N, i):
    """real[i - 100:i] with i < 100: a negative start counts from the end of the array and then clips at 0, so the
    left window is real[0:i] when N < 100 and empty when N - 100 + i >= i.  The device scores what the host scores
    and refuses where the host raises."""
    rng = np.random.default_rng(N + i)
    z = 0.1 * rng.standard_normal(N) + 0.1j * rng.standard_normal(N)
    z[i] = 50.0                                 # the tallest real point at phase (0, 0)
    try:
        want = proc_autophase._ps_peak_minima_score([0.0, 0.0], z)
    except ValueError:
        want = None
    if want is None:
        with pytest.raises(ValueError, match="spectrum 0"):
            proc_autophase.phase_scores([z], [[0.0, 0.0]], "peak_minima")
    else:
        got = proc_autophase.phase_scores([z], [[0.0, 0.0]], "peak_minima")[0, 0]
        assert got == pytest.approx(want, rel=1e-12, abs=1e-15)


def test_long_lists_are_cut_into_calls_without_changing_a_value(monkeypatch):
    """The library takes at most 65535 spectra per call; the Python layer cuts longer lists.  Cut every 2 spectra
    here: the scores, the optimisation and the brute levels equal those of one call."""
    zs = _ragged((300, 4096, 20000, 1000, 2000), seed=41)
    ph = np.random.default_rng(2).uniform(-30, 30, (4, 2))
    angles = np.arange(-np.pi, np.pi, np.pi / 30)
    whole = (proc_autophase.phase_scores(zs, ph, "acme"), proc_autophase.estimate_many(zs, "acme"),
             proc_autophase.brute_levels([z.real for z in zs], [z.imag for z in zs], angles))
    monkeypatch.setattr(proc_autophase, "_MAX_SPECTRA_PER_CALL", 2)
    cut = (proc_autophase.phase_scores(zs, ph, "acme"), proc_autophase.estimate_many(zs, "acme"),
           proc_autophase.brute_levels([z.real for z in zs], [z.imag for z in zs], angles))
    np.testing.assert_array_equal(cut[0], whole[0])
    for a, b in zip(cut[1], whole[1]):
        np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(cut[2], whole[2])

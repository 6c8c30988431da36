"""
CPU tier of the device-batched phase correction (nmrfit_phase_scores / _estimate / _brute_levels): the entry points are
exported and bound, every argument error is refused before any device work (no GPU needed), and a callable score runs
the reference's host loop unchanged.
"""
import ctypes
import os

import numpy as np
import pytest

from nmrfit_amd import _cabi, proc_autophase, synth


def test_phase_entry_points_are_exported_and_bound():
    L = ctypes.CDLL(_cabi.LIB_PATH)
    for name in ("nmrfit_phase_scores", "nmrfit_phase_estimate", "nmrfit_phase_brute_levels"):
        assert hasattr(L, name) and name in _cabi.SIGNATURES
    assert hasattr(L, "nmrfit_diag_phase_nm_rosenbrock") and "nmrfit_diag_phase_nm_rosenbrock" in _cabi.DIAG_SIGNATURES
    assert _cabi.ABI_VERSION == _cabi.lib().nmrfit_abi_version()
    assert (_cabi.PHASE_ACME, _cabi.PHASE_PEAK_MINIMA, _cabi.PHASE_BRUTE_LEVEL) == (0, 1, 2)


def _arrays(Ns=(64, 100)):
    N = np.array(Ns, dtype=np.int64)
    u = np.ones(int(N.sum()))
    return N, u, u.copy()


def _scores(kind=0, S=2, N=None, u=None, v=None, M=3, cand=True, score=True, status=True):
    N0, u0, v0 = _arrays()
    N = N0 if N is None else N
    u = u0 if u is None else u
    v = v0 if v is None else v
    c = np.zeros((max(S, 1), max(M, 1), 2))
    sc = np.zeros((max(S, 1), max(M, 1)))
    st = np.zeros(max(S, 1), dtype=np.int32)
    p = _cabi.ptr
    return _cabi.lib().nmrfit_phase_scores(0, kind, S, p(N) if N is not False else None, p(u) if u is not False else None,
                                           p(v) if v is not False else None, M, p(c) if cand else None,
                                           p(sc) if score else None, p(st) if status else None)


def _estimate(kind=0, S=2, N=None, nulls=()):
    N0, u, v = _arrays()
    N = N0 if N is None else N
    x0 = np.zeros((max(S, 1), 2))
    x = np.zeros_like(x0)
    f = np.zeros(max(S, 1))
    ints = [np.zeros(max(S, 1), dtype=np.int32) for _ in range(3)]
    args = dict(N=N, u=u, v=v, x0=x0, x=x, f=f, nfev=ints[0], nit=ints[1], status=ints[2])
    p = {k: (None if k in nulls else _cabi.ptr(a)) for k, a in args.items()}
    return _cabi.lib().nmrfit_phase_estimate(0, kind, S, p["N"], p["u"], p["v"], p["x0"], p["x"], p["f"], p["nfev"],
                                             p["nit"], p["status"])


def _refused(rc, text):
    assert rc == _cabi.E_INVALID
    msg = _cabi.lib().nmrfit_last_error().decode()
    assert text in msg, msg


@pytest.mark.parametrize("kind", [0, 1, 2])
def test_phase_scores_argument_errors_need_no_gpu(kind):
    _refused(_scores(kind, S=0), "S must be")
    _refused(_scores(kind, M=0), "M must be")
    _refused(_scores(kind, N=np.array([64, 1], dtype=np.int64)), "N >= 2")
    for key in ("N", "u", "v"):
        _refused(_scores(kind, **{key: False}), "null pointer")
    for key in ("cand", "score", "status"):
        _refused(_scores(kind, **{key: False}), "null pointer")
    _refused(_scores(kind=3), "unknown score kind")
    _refused(_scores(kind=-1), "unknown score kind")


def test_phase_estimate_argument_errors_need_no_gpu():
    _refused(_estimate(S=0), "S must be")
    _refused(_estimate(N=np.array([2, 0], dtype=np.int64)), "N >= 2")
    for key in ("N", "u", "v", "x0", "x", "f", "nfev", "nit", "status"):
        _refused(_estimate(nulls=(key,)), "null pointer")
    _refused(_estimate(kind=_cabi.PHASE_BRUTE_LEVEL), "kind must be")
    _refused(_estimate(kind=7), "kind must be")
    L = _cabi.lib()
    assert L.nmrfit_diag_phase_nm_rosenbrock(0, 0, None, None, None, None, None) == _cabi.E_INVALID


def _brute(S=2, N=None, n_mean=(1, 1), M=3, nulls=()):
    N0, u, v = _arrays()
    N = N0 if N is None else N
    if N is not N0:
        u = np.ones(int(N.sum()))
        v = u.copy()
    args = dict(N=N, n_mean=np.array(n_mean, dtype=np.int64), u=u, v=v, cand=np.zeros((max(S, 1), max(M, 1), 2)),
                score=np.zeros((max(S, 1), max(M, 1))))
    p = {k: (None if k in nulls else _cabi.ptr(a)) for k, a in args.items()}
    return _cabi.lib().nmrfit_phase_brute_levels(0, S, p["N"], p["n_mean"], p["u"], p["v"], M, p["cand"], p["score"])


def test_brute_levels_argument_errors_need_no_gpu():
    """nmrfit_phase_brute_levels refuses before any device work: null pointers, S and M out of range, a mean length
    below 1 (E_INVALID) or above 128 (E_UNSUPPORTED, naming the spectrum and its mean length)."""
    _refused(_brute(S=0), "S must be")
    _refused(_brute(M=0), "M must be")
    _refused(_brute(N=np.array([64, 1], dtype=np.int64)), "N >= 2")
    for key in ("N", "n_mean", "u", "v", "cand", "score"):
        _refused(_brute(nulls=(key,)), "null pointer")
    _refused(_brute(n_mean=(1, 0)), "mean length must be >= 1 (spectrum 1)")
    _refused(_brute(n_mean=(-5, 1)), "mean length must be >= 1 (spectrum 0)")
    assert _brute(n_mean=(3, 129)) == _cabi.E_UNSUPPORTED
    msg = _cabi.lib().nmrfit_last_error().decode()
    assert "spectrum 1" in msg and "mean length of 129" in msg, msg
    # the refusal is keyed on the mean length, not on N: 128 points of mean over a 100-point spectrum passes validation
    assert _brute(n_mean=(128, 128)) in (_cabi.OK, _cabi.E_NO_DEVICE)


def test_brute_level_kind_refuses_from_645000_points_before_the_device():
    """nmrfit_phase_scores(kind = BRUTE_LEVEL) keeps its own rule, n = max(1, N // 5000) <= 128."""
    for N, ok in ((645000, False), (644999, True)):
        Ns = np.array([64, N], dtype=np.int64)
        u = np.ones(int(Ns.sum()))
        rc = _scores(_cabi.PHASE_BRUTE_LEVEL, N=Ns, u=u, v=u.copy())
        if ok:
            assert rc in (_cabi.OK, _cabi.E_NO_DEVICE), _cabi.lib().nmrfit_last_error()
        else:
            assert rc == _cabi.E_UNSUPPORTED
            assert "N < 645000" in _cabi.lib().nmrfit_last_error().decode()


def _host_levels(us, vs, angles, device=0, n=None):
    """brute_levels computed as Data._brute_phase's loop body does it, with the mean length asked for"""
    out = np.empty((len(us), len(angles)))
    for k, (u, v) in enumerate(zip(us, vs)):
        nk = max(1, len(u) // 5000) if n is None else int(np.broadcast_to(n, (len(us),))[k])
        for m, a in enumerate(angles):
            V, _ = proc_autophase.ps2(u, v, a, 0.0)
            err = np.sqrt((V[:nk].mean() - V[-nk:].mean()) ** 2)
            out[k, m] = err if np.max(V) > abs(np.min(V)) else np.nan
    return out


def test_shift_phase_many_brute_takes_the_hosts_mean_length(monkeypatch):
    """Data._brute_phase takes n from len(self.V), and select_bounds crops u, v but not V.  On a 65536-point Data
    cropped to 19660 points the host's n is 13, not 3, and the chosen angle differs.  shift_phase_many passes the
    host's n; brute_levels is replaced by a host emulation so that this needs no GPU."""
    from nmrfit_amd.containers import Data, shift_phase_many
    monkeypatch.setattr(proc_autophase, "brute_levels", _host_levels)
    sp = synth.make_spectrum(65536, 4, seed=0, physical=True)
    noise = 0.002 * np.max(sp["u"]) * np.random.default_rng(100).standard_normal((2, 65536))
    twins = [Data(sp["w"], sp["u"] + noise[0], sp["v"] + noise[1]) for _ in range(2)]
    lo, hi = np.percentile(sp["w"], [20, 50])
    for d in twins:
        d.select_bounds(lo, hi)
    host, dev = twins
    step = np.pi / 90
    host.shift_phase("brute", step=step)
    shift_phase_many([dev], "brute", step=step)
    print("cropped %d of 65536 points: host p0 %r, shift_phase_many p0 %r" % (len(dev.u), host.p0, dev.p0))
    assert len(dev.u) == 19660
    assert (dev.p0, dev.p1) == (host.p0, host.p1)
    np.testing.assert_array_equal(dev.V, host.V)
    # (n from len(u) would pick another angle here: the test can tell the two apart)
    angles = np.arange(-np.pi, np.pi, step)
    e = _host_levels([dev.u], [dev.v], angles)[0]
    assert angles[np.flatnonzero(e == e[e < np.inf].min())[0]] != host.p0


def test_constant_spectrum_acme_end_point_is_set_by_rounding():
    """fmin on the ACME score of a constant 1 + 1j spectrum: near the optimum (p0 = -45 degrees, p1 ~ 0.04) the slopes
    are differences of nearly equal rotated values, so the end point depends on the last ulp of the rotation.  Turning
    the ramp exp(i theta) into cos(theta) + i sin(theta) with theta scaled by 1 + 2e-16 moves scipy's own end point by
    more than xatol = 1e-4 degrees.  This is why tests/test_gpu_phase_edges.py compares the device with fmin on every
    degenerate spectrum except this one: the device's sincos is not numpy's exp to the last ulp."""
    N = 4096
    z = np.full(N, 1.0 + 1.0j)

    def acme(ph, scale):
        theta = (ph[0] * np.pi / 180.0 + (ph[1] * np.pi / 180.0 * np.arange(N) / N)) * scale
        real = np.cos(theta) * z.real - np.sin(theta) * z.imag
        slope = np.abs((real[1:] - real[:-1]) / 2.0)
        prob = slope / np.sum(slope)
        prob[prob == 0] = 1
        neg = real - np.abs(real)
        return np.sum(-prob * np.log(prob)) + 1000 * (np.sum((neg / 2) ** 2) if np.sum(neg) < 0 else 0.0)

    import scipy.optimize
    with np.errstate(all="ignore"):
        ends = [scipy.optimize.fmin(acme, [0.0, 0.0], args=(s,), disp=False) for s in (1.0, 1.0 + 2e-16)]
    assert np.max(np.abs(ends[0] - ends[1])) > 1e-4, ends


def test_python_layer_refuses_bad_input_before_the_device():
    z = np.ones(64, dtype=complex)
    with pytest.raises(ValueError, match="fn must be"):
        proc_autophase.phase_scores([z], [[0.0, 0.0]], fn="entropy")
    with pytest.raises(ValueError, match="phases must be"):
        proc_autophase.phase_scores([z, z], np.zeros((3, 3, 2)))
    with pytest.raises(ValueError, match="fn must be"):
        proc_autophase.approximate_phase_many([z], fn="entropy")
    from nmrfit_amd import containers
    with pytest.raises(ValueError, match="Method must be"):
        containers.shift_phase_many([], method="best")


def test_callable_score_runs_the_host_loop():
    """A callable fn is not a device score: approximate_phase_many / autops_many run approximate_phase / autops per
    spectrum, with the per-spectrum starting points."""
    zs = []
    for k, N in enumerate((512, 700)):
        sp = synth.make_spectrum(N, 2, seed=3 + k, physical=True)
        zs.append(sp["u"] + 1j * sp["v"])
    fn = proc_autophase._ps_acme_score
    got = proc_autophase.approximate_phase_many(zs, fn, p0=[1.0, 2.0], p1=-1.0)
    want = [proc_autophase.approximate_phase(z, fn, a, -1.0) for z, a in zip(zs, (1.0, 2.0))]
    assert got.shape == (2, 2)
    np.testing.assert_array_equal(got, np.array(want))
    phased = proc_autophase.autops_many(zs, fn)
    for z, ph in zip(zs, phased):
        np.testing.assert_array_equal(ph, proc_autophase.autops(z, fn))


def test_device_path_without_gpu_fails_loudly():
    if _cabi.device_count() != 0:
        pytest.skip("a GPU is visible: tests/test_gpu_phase.py covers the device path")
    z = np.ones(64, dtype=complex)
    with pytest.raises(_cabi.NmrfitError) as ei:
        proc_autophase.approximate_phase_many([z])
    assert ei.value.code == _cabi.E_NO_DEVICE

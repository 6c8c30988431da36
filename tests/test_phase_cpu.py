"""
CPU tier of the device-batched phase correction (nmrfit_phase_scores / nmrfit_phase_estimate): the entry points are
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
    for name in ("nmrfit_phase_scores", "nmrfit_phase_estimate"):
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

"""
CPU tier of the noise replicas (nmrfit_amd/noise.py, csrc/noise.hip, include/nmrfit_amd_noise.h): the numpy mirror of
the deviates against 200-bit truth and as a sample of a standard normal, the ctypes table against the header, the
library's argument checks (made before any device work), and the statistics of ``ReplicaFits`` on hand-made fits.
"""
import ctypes
import os
import re

import numpy as np
import pytest

import nmrfit_amd
from nmrfit_amd import _cabi, noise
from tests import noise_support as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_mirror_against_200_bit_truth():
    """normals(7, 2000) within 2 e of the mpmath values, e = 2^-52 max(1, r).  Measured: 1.000 e against the truth
    rounded to fp64, which is what tests/noise_support.py keeps and both tiers measure against (two doubles differ by
    whole ulps: here two ulps of a z_v of 0.94); against the unrounded 200-bit values the worst is 0.948 e."""
    zu, zv = noise.normals(T.TRUTH_SEED, T.TRUTH_N)
    worst = T.worst_error(zu, zv)
    print("mirror: worst error %.3f e" % worst)
    assert worst <= 2.0


def test_moments_of_the_deviates():
    """Scores of n = 4096 deviates per seed that are ~N(0, 1) for independent standard normals: all below 4."""
    n = 4096
    z = {s: noise.normals(s, n) for s in (0, 1, 2)}
    scores = {}
    for s, (zu, zv) in z.items():
        for name, x in (("u", zu), ("v", zv)):
            scores["mean %s seed %d" % (name, s)] = x.mean() * np.sqrt(n)
            scores["var %s seed %d" % (name, s)] = (x.var() - 1.0) * np.sqrt(n / 2.0)
            scores["lag1 %s seed %d" % (name, s)] = np.mean(x[:-1] * x[1:]) * np.sqrt(n)
        scores["cross channel seed %d" % s] = np.mean(zu * zv) * np.sqrt(n)
    for ch, name in enumerate("uv"):
        scores["cross seed 1 x 2 %s" % name] = np.mean(z[1][ch] * z[2][ch]) * np.sqrt(n)
    worst = max(scores, key=lambda k: abs(scores[k]))
    print("largest score: %s = %.3f" % (worst, scores[worst]))
    for name, val in scores.items():
        assert abs(val) < 4.0, (name, val)


def test_deviates_depend_on_seed_and_point_only():
    """A prefix of a longer draw is the shorter draw; the high seed word matters; the stream is not the swarm's."""
    zu, zv = noise.normals(5, 700)
    zu2, zv2 = noise.normals(5, 100)
    assert np.array_equal(zu[:100], zu2) and np.array_equal(zv[:100], zv2)
    assert not np.array_equal(noise.normals(5 + (1 << 32), 100)[0], zu2)
    assert np.all(np.isfinite(zu)) and np.all(np.isfinite(zv))
    assert noise.NOISE_TAG >= 1 << 28        # (the swarm's counter word 2 is a particle index, below 2^28: batch.hip)


def test_replicas_host():
    rng = np.random.default_rng(3)
    u, v = rng.standard_normal(50), rng.standard_normal(50)
    u[3], v[4] = -0.0, np.nan
    zu, zv = noise.normals(9, 50)
    a, b = noise.replicas_host(u, v, 0.5, 0.25, 9)
    assert np.array_equal(a, u + 0.5 * zu) and np.array_equal(b, v + 0.25 * zv, equal_nan=True) and np.isnan(b[4])
    (a0, b0), (a1, b1) = noise.replicas_host([u, u[:7]], [v, v[:7]], [0.0, 0.5], [0.0, 0.25], [1, 9])
    assert a0.tobytes() == u.tobytes() and b0.tobytes() == v.tobytes() and a0 is not u      # sigma 0: the bits stay
    assert np.array_equal(a1, a[:7])
    assert u[3] == 0 and np.signbit(u[3])                                                   # (the input is not written)


def _declared(header):
    text = open(os.path.join(ROOT, "include", header)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return set(re.findall(r"\b(nmrfit_[a-z0-9_]+)\s*\(", text))


def test_table_and_header():
    """NOISE_SIGNATURES is what include/nmrfit_amd_noise.h declares, the library exports it, the product header and the
    ABI number are as they were."""
    names = _declared("nmrfit_amd_noise.h")
    assert names == set(_cabi.NOISE_SIGNATURES), (names, set(_cabi.NOISE_SIGNATURES))
    assert len(names) == 3 and not (names & _declared("nmrfit_amd.h"))
    L = _cabi.lib()
    for n in names:
        assert hasattr(L, n), n
    assert L.nmrfit_abi_version() == _cabi.ABI_VERSION == 6
    assert "0x%08X" % noise.NOISE_TAG in open(os.path.join(ROOT, "include", "nmrfit_amd_noise.h")).read()


def test_argument_validation_needs_no_gpu():
    """nmrfit_noise_replicas reports a null pointer, K = 0, N[k] = 0 and a sigma of -1, NaN or inf as NMRFIT_E_INVALID
    before anything touches a device; the two batch calls refuse a null handle."""
    L = _cabi.lib()
    p = _cabi.ptr
    K = 2
    N = np.array([4, 3], dtype=np.int64)
    u, v = np.zeros(7), np.zeros(7)
    su, sv = np.array([1.0, 0.0]), np.array([0.5, 0.0])
    seed = np.array([1, 2], dtype=np.uint64)
    uo, vo = np.empty(7), np.empty(7)
    good = [0, K, p(N), p(u), p(v), p(su), p(sv), p(seed), p(uo), p(vo)]
    for i in range(2, len(good)):
        args = list(good)
        args[i] = None
        assert L.nmrfit_noise_replicas(*args) == _cabi.E_INVALID, i
    args = list(good)
    args[1] = 0
    assert L.nmrfit_noise_replicas(*args) == _cabi.E_INVALID
    args[1] = -3
    assert L.nmrfit_noise_replicas(*args) == _cabi.E_INVALID
    args = list(good)
    args[2] = p(np.array([4, 0], dtype=np.int64))
    assert L.nmrfit_noise_replicas(*args) == _cabi.E_INVALID
    assert b"N > 0" in L.nmrfit_last_error()
    for bad in (-1.0, np.nan, np.inf):
        for i in (5, 6):
            args = list(good)
            s = np.array([0.5, bad])
            args[i] = p(s)
            assert L.nmrfit_noise_replicas(*args) == _cabi.E_INVALID, (bad, i)
            assert b"sigma" in L.nmrfit_last_error()
    assert L.nmrfit_batch_add_noise(None, p(su), p(sv), p(seed)) == _cabi.E_INVALID
    assert L.nmrfit_batch_spectrum(None, 0, p(uo), p(vo)) == _cabi.E_INVALID
    # beyond the per-call limits (checked before the device too): unsupported, not invalid
    big = np.array([(1 << 26) + 1], dtype=np.int64)
    args = list(good)
    args[1], args[2] = 1, p(big)
    assert L.nmrfit_noise_replicas(*args) == _cabi.E_UNSUPPORTED
    if _cabi.device_count() == 0:       # with valid arguments and no GPU: loudly, no CPU path
        assert L.nmrfit_noise_replicas(*good) == _cabi.E_NO_DEVICE
        with pytest.raises(_cabi.NmrfitError):
            noise.replicas([u], [v], 1.0, 1.0, [1])


class _Fit:
    def __init__(self, params, error):
        self.params, self.error = np.asarray(params, dtype=float), error

    calculate_area_fraction = nmrfit_amd.utils.FitUtility.calculate_area_fraction
    get_areas = nmrfit_amd.utils.FitUtility.get_areas


def test_replica_fits_statistics():
    """std with ddof = 1 over the noisy fits only, the original left out; percentiles of the same set."""
    head = [0.1, 0.2, 0.5, 0.0]
    areas = [(10.0, 1.0), (10.0, 2.0), (10.0, 3.0), (10.0, 6.0), (10.0, 0.5)]      # (peak, satellite): fraction s / (10 + s)
    fits = [_Fit(head + [1.0, 3.1, a, 1.0, 3.4, s], 0.01 * k) for k, (a, s) in enumerate(areas)]
    frac = np.array([s / (a + s) for a, s in areas])
    rf = noise.ReplicaFits(fits, [(0.0, 0.0)] + [(0.1, 0.2)] * 4, range(5), iterations=[5, 6, 7, 8, 9], stop=[1, 2, 0, 1, 2])
    assert rf.params.shape == (5, 10) and np.array_equal(rf.errors, 0.01 * np.arange(5))
    assert np.allclose(rf.area_fractions, frac, rtol=1e-15)
    assert rf.area_fraction_std == np.std(rf.area_fractions[1:], ddof=1)
    assert rf.area_fraction_std != np.std(rf.area_fractions, ddof=1) and rf.area_fraction_std != np.std(rf.area_fractions[1:])
    assert np.array_equal(rf.params_std, np.std(rf.params[1:], axis=0, ddof=1)) and rf.params_std[0] == 0.0
    assert rf.percentile(50) == np.percentile(rf.area_fractions[1:], 50)
    assert np.array_equal(rf.percentile([2.5, 97.5]), np.percentile(rf.area_fractions[1:], [2.5, 97.5]))
    assert rf.sigma.shape == (5, 2) and rf.seeds == [0, 1, 2, 3, 4]
    assert list(rf.iterations) == [5, 6, 7, 8, 9] and list(rf.stop) == [1, 2, 0, 1, 2]
    allnoisy = noise.ReplicaFits(fits, [(0.1, 0.2)] * 5, range(5), include_original=False)
    assert allnoisy.area_fraction_std == np.std(allnoisy.area_fractions, ddof=1)


def test_fit_replicas_needs_a_sigma():
    from nmrfit_amd import synth
    sp = synth.make_spectrum(256, 2, seed=1)
    data = synth.SynthData(sp["w"], sp["u"], sp["v"], sp["peaks"])
    with pytest.raises(ValueError, match="sigma"):
        nmrfit_amd.fit_replicas(data, sp["lower"], sp["upper"], replicas=4)
    with pytest.raises(ValueError):
        nmrfit_amd.fit_replicas(data, sp["lower"], sp["upper"], replicas=4, sigma=(1.0, 2.0, 3.0))
    with pytest.raises(ValueError):
        nmrfit_amd.fit_replicas(data, sp["lower"], sp["upper"], replicas=4, sigma=-1.0)
    assert nmrfit_amd.fit_replicas is noise.fit_replicas and nmrfit_amd.fit_replicas_many is noise.fit_replicas_many
    # noise_region: sample_noise of each channel
    x0, x1 = 3.0, 3.05
    su, sv = noise._job_sigma(dict(noise_region=(x0, x1)), data)
    from nmrfit_amd import utils
    assert su == utils.sample_noise(data.w, data.u, x0, x1) and sv == utils.sample_noise(data.w, data.v, x0, x1) and su > 0

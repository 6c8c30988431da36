"""
GPU tier of the sandwich covariance (csrc/lsq_cov.hip, include/nmrfit_amd_cov.h, nmrfit_amd/uncertainty.py): the
device's meat against numpy at the shapes where the kernel can go wrong, A, g and f against nmrfit_jacobian's bits, the
same bits alone and anywhere in any batch, the standard errors against the linear-response truth of
tests/calibration_support.py, and fit_many(uncertainty=...) against a replica study.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import nmrfit_amd
from nmrfit_amd import _cabi, lsq, synth, uncertainty
from nmrfit_amd.batch import FitBatch
from nmrfit_amd.equations import Evaluator

from . import calibration_support as cs
from . import uncertainty_support as us
from .lsq_support import perturbed_start, spectrum_tuple

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (N, P): one ragged tile; two segments, the second holding one point; 65 tiles -- two tiles per segment, a last segment
# of one; the smallest D; D = 76, every accumulator of every thread in use
MEAT_SHAPES = ((63, 2), (65, 2), (4160, 2), (130, 1), (130, 24))


def _same(a, b):
    return all(np.array_equal(np.asarray(p), np.asarray(q)) for p, q in zip(a, b))


@pytest.mark.parametrize("N,P", MEAT_SHAPES)
def test_meat_against_numpy(N, P):
    """The device's M against numpy's (q J)^T J made from the device's OWN J and numpy's q, sigma_v = 2 sigma_u, entry by
    entry within the derived bound (uncertainty_support.meat_bound); M symmetric to the bit; A, g and f nmrfit_jacobian's
    bits; the batch call's bits the context's."""
    sp = synth.make_spectrum(N, P, seed=3 + P, physical=True)
    x = perturbed_start(sp, 9 + N)
    su = 1e-3 * float(np.max(np.abs(sp["u"])))
    sv = 2.0 * su
    s = 1.0 / np.sqrt(N)
    with Evaluator(*spectrum_tuple(sp)) as ev:
        rows, h = lsq.ResidualModel(ev, sp["lower"], sp["upper"]).rows(x)
        ref = ev.jacobian(rows, s / h, s, J=True, normal=True)
        got = ev.sandwich(rows, s / h, s, su, sv)
    J = ref["J"]
    q = uncertainty.residual_variance(sp["weights"], x, su, sv)
    want = (q[:, None] * J).T @ J
    assert np.array_equal(want, uncertainty.sandwich_host(J, sp["weights"], x, su, sv))
    bound = us.meat_bound(J, q, x, su, sv)
    err = np.abs(got["M"] - want)
    print("N=%d D=%d: worst |M_dev - M_numpy| / bound %.3g" % (N, J.shape[1], np.max(err / bound)))
    assert np.all(np.isfinite(got["M"])) and np.all(err <= bound), np.max(err / bound)
    assert np.array_equal(got["M"], got["M"].T)
    assert np.array_equal(got["A"], ref["A"]) and np.array_equal(got["g"], ref["g"]) and got["f"] == ref["f"]
    twin = synth.make_spectrum(64, 1, seed=1, physical=True)      # (a batch holds the fit second, behind another shape)
    A, M, g, f = us.batch_sandwich([twin, sp], [twin["x_true"], x], [(su, sv), (su, sv)], (0, 1))[1]
    assert np.array_equal(M, got["M"]) and np.array_equal(A, got["A"]) and np.array_equal(g, got["g"]) and f == got["f"]


def test_too_many_peaks_are_unsupported():
    """P = 25 (D = 79) is beyond the accumulators: NMRFIT_E_UNSUPPORTED on a context and on a batch, which stays usable."""
    sp = synth.make_spectrum(130, 25, seed=4, physical=True)
    small = synth.make_spectrum(130, 1, seed=5, physical=True)
    s = 1.0 / np.sqrt(130)
    with Evaluator(*spectrum_tuple(sp)) as ev:
        rows, h = lsq.ResidualModel(ev, sp["lower"], sp["upper"]).rows(sp["x_true"])
        with pytest.raises(_cabi.NmrfitError) as ei:
            ev.sandwich(rows, s / h, s, 1.0, 1.0)
        assert ei.value.code == _cabi.E_UNSUPPORTED
        assert np.all(np.isfinite(ev.jacobian(rows, s / h, s, J=True)["J"]))
    specs = [small, sp]
    with FitBatch([spectrum_tuple(q) for q in specs], [q["lower"] for q in specs], [q["upper"] for q in specs], swarmsize=8,
                  seeds=[1, 2]) as fb:
        with pytest.raises(_cabi.NmrfitError) as ei:
            fb.sandwich([q["x_true"] for q in specs], 1.0, 1.0)
        assert ei.value.code == _cabi.E_UNSUPPORTED
        fb.run(2, 1)
        assert all(np.isfinite(f) for _, f in fb.best())


@pytest.fixture(scope="module")
def record():
    """uncertainty_support.device_record() of this process (computed once, read-only)."""
    rec = us.device_record()
    for a in rec.values():
        a.setflags(write=False)
    return rec


def test_same_bits_alone_and_in_any_batch(record, monkeypatch):
    """Lone context against batch; first, middle and last position in a ragged batch of different N and P; two calls; a
    workspace budget that makes every fit its own group: the same bits of A, M, g and f."""
    sps, X, sig = us.bits_problems()
    for k in range(len(sps)):
        for name in us.BITS_KEYS:
            a, b = record["lone.%d.%s" % (k, name)], record["batch.%d.%s" % (k, name)]
            assert np.all(np.isfinite(a)) and np.array_equal(a, b), (k, name)
    base = [tuple(record["batch.%d.%s" % (k, name)] for name in us.BITS_KEYS) for k in range(len(sps))]
    for order in ((1, 2, 0), (2, 0, 1)):      # with (0, 1, 2): every fit first, in the middle and last
        got = us.batch_sandwich(sps, X, sig, order)
        assert all(_same(got[k], base[k]) for k in range(len(sps))), order
    again = us.device_record()
    assert sorted(again) == sorted(record) and all(np.array_equal(again[k], record[k]) for k in record)
    monkeypatch.setenv("NMRFIT_LSQ_WORKSPACE_MB", "1")
    got = us.batch_sandwich(sps, X, sig, (0, 1, 2))
    assert all(_same(got[k], base[k]) for k in range(len(sps)))


@pytest.mark.parametrize("poison", ("255", "63"))
def test_same_bits_under_poisoned_allocations(record, poison, tmp_path):
    """NMRFIT_POISON_ALLOC=255 (every fresh double a NaN) and 63 (a plausible finite value), each in a fresh child
    process: the record of this process, byte for byte -- no bit of A, M, g or f leans on what a fresh block holds."""
    out = str(tmp_path / "record.npz")
    env = dict(os.environ, NMRFIT_POISON_ALLOC=poison)
    run = subprocess.run([sys.executable, "-m", "tests.uncertainty_support", out], cwd=ROOT, env=env, capture_output=True,
                         text=True, timeout=120)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-3000:]
    with np.load(out) as child:
        assert sorted(child.files) == sorted(record)
        for k in record:
            assert child[k].tobytes() == record[k].tobytes(), k


def test_device_against_the_truth():
    """FitBatch.uncertainty at Truth.x0 of four calibration cases in ONE batch (no fitting: X is given): standard errors,
    area-fraction error and covariance within the bars measured on the CPU mirror; nothing fixed, and x0 the minimiser."""
    names = us.DEVICE_CASES
    truths = [cs.truth(n) for n in names]
    cases = [t.case for t in truths]
    with FitBatch([c.spectrum_tuple() for c in cases], [c.lower for c in cases], [c.upper for c in cases], swarmsize=8,
                  seeds=[1, 2, 3, 4]) as fb:
        got = fb.uncertainty([t.x0 for t in truths], [c.sigma_u for c in cases], [c.sigma_v for c in cases])
    for name, t, fu in zip(names, truths, got):
        dev = us.deviations(name, fu)
        cpu = us.deviations(name, us.mirror(name))
        print("%-18s device std %.3e af %.3e cov %.3e (CPU mirror %.3e %.3e %.3e) distance %.2e"
              % (name, dev["std"], dev["af"], dev["cov"], cpu["std"], cpu["af"], cpu["cov"], fu.distance))
        assert fu.status == "ok" and not fu.fixed.any() and fu.sigma == (t.case.sigma_u, t.case.sigma_v)
        for k, v in dev.items():
            assert v <= us.bars(name)[k], (name, k, v, us.bars(name)[k])
        assert fu.distance < 1e-4, (name, fu.distance)
        assert fu.area_fraction == cs.area_fraction(t.x0)


def test_end_to_end():
    """fit_many with options['polish'], batch_polish=True and uncertainty=dict(sigma=(su, sv)) on n1024_p3_v2 against
    fit_replicas with the case's 63 documented seeds and polish: for every parameter and for the area fraction the
    replicas' standard deviation over the first-order standard error lies inside sqrt(chi2_quantiles(62)) = [0.60, 1.45]
    (the linear-response reference alone: 0.84 ... 1.18 and 1.07), and the polished fit stands closer to its minimiser
    than the polish's stopping distance."""
    c = cs.case("n1024_p3_v2")
    sigma = (c.sigma_u, c.sigma_v)
    jobs = [dict(data=c.data(), lower=c.lower, upper=c.upper, options={'seed': c.seed0 + k, 'polish': True}) for k in (0, 1)]
    fits = nmrfit_amd.fit_many(jobs, batch_polish=True, uncertainty=dict(sigma=sigma))
    plain = nmrfit_amd.fit_many(jobs, batch_polish=True)
    lo, hi = (float(np.sqrt(q)) for q in cs.chi2_quantiles(c.M - 1))
    assert c.M == 63 and abs(lo - 0.60) < 0.01 and abs(hi - 1.45) < 0.01
    rf = nmrfit_amd.fit_replicas(c.data(), c.lower, c.upper, replicas=c.M, sigma=sigma, seed=c.seed0, options={'polish': True})
    assert rf.seeds == c.seeds
    for f, p in zip(fits, plain):
        fu = f.uncertainty
        assert isinstance(fu, uncertainty.FitUncertainty) and fu.status == "ok" and fu.sigma == sigma
        assert np.array_equal(f.params, p.params) and f.error == p.error      # params and error never change
        assert np.array_equal(fu.x, f.params)
        ratio = rf.params_std / fu.params_std
        af_ratio = rf.area_fraction_std / fu.area_fraction_std
        print("replica std / params_std %s; area fraction %.3f; distance %.3g (stopping distance %.3g)"
              % (np.round(ratio, 3), af_ratio, fu.distance, cs.stopping_distance(c.N)))
        assert np.all((ratio >= lo) & (ratio <= hi)), ratio
        assert lo <= af_ratio <= hi, af_ratio
        assert fu.distance < cs.stopping_distance(c.N), fu.distance
        assert fu.area_fraction == f.calculate_area_fraction()


def test_fit_many_paths():
    """A fit that ran alone goes through a context and gets the batch's record to the bit; a job's own sigma wins over the
    call's; noise_region means what it means in fit_replicas_many; params and error are the plain call's."""
    a, b = cs.case("user_n512_p2"), cs.case("user_n1024_p3_v2")
    opts = {'maxiter': 20, 'swarmsize': 32}
    jobs = [dict(data=a.data(), lower=a.lower, upper=a.upper, options=dict(opts, seed=1)),
            dict(data=b.data(), lower=b.lower, upper=b.upper, sigma=(b.sigma_u, b.sigma_v), options=dict(opts, seed=2))]
    batched = nmrfit_amd.fit_many(jobs, uncertainty=dict(sigma=a.sigma_u))
    alone = nmrfit_amd.fit_many(jobs, batch=False, uncertainty=dict(sigma=a.sigma_u))
    for f, g, want in zip(batched, alone, ((a.sigma_u, a.sigma_u), (b.sigma_u, b.sigma_v))):
        assert np.array_equal(f.params, g.params) and f.error == g.error
        assert f.uncertainty.sigma == g.uncertainty.sigma == want
        for name in ("A", "M", "g", "cov", "params_std", "newton_step"):
            assert np.array_equal(getattr(f.uncertainty, name), getattr(g.uncertainty, name), equal_nan=True), name
        # an unpolished swarm of 20 generations stands many standard errors from the minimiser, and the record says so
        assert f.uncertainty.status == "ok" and f.uncertainty.distance > 1.0
    w = np.asarray(a.w)
    region = (float(w.min()), float(w.min() + 0.1 * (w.max() - w.min())))
    from nmrfit_amd.noise import _job_sigma
    got = nmrfit_amd.fit_many(jobs[:1], uncertainty=dict(noise_region=region))[0]
    assert got.uncertainty.sigma == _job_sigma(dict(noise_region=region), jobs[0]["data"])
    lone = nmrfit_amd.utils.FitUtility.uncertainty(batched[0], sigma=a.sigma_u)
    assert np.array_equal(lone.cov, batched[0].uncertainty.cov)


def test_refusals():
    """A fit_im batch and a context set to another kernel variant are NMRFIT_E_UNSUPPORTED; null required pointers and a
    bad sigma NMRFIT_E_INVALID; after each the batch / context works.  (The NMRFIT_E_STATE of a reconstruction in flight
    cannot be reached from a test: the reconstruction begins and ends inside one call of the library -- as for
    nmrfit_batch_normal_equations.)"""
    specs = [synth.make_spectrum(n, p, seed=30 + p, physical=True) for n, p in ((300, 1), (513, 2))]
    X = [sp["x_true"] for sp in specs]
    L = _cabi.lib()

    def make(fit_im):
        return FitBatch([spectrum_tuple(sp) for sp in specs], [sp["lower"] for sp in specs], [sp["upper"] for sp in specs],
                        swarmsize=8, seeds=[1, 2], fit_im=fit_im)
    for fit_im in (True, "sum"):
        with make(fit_im) as fb:
            with pytest.raises(_cabi.NmrfitError) as ei:
                fb.sandwich(X, 1.0, 1.0)
            assert ei.value.code == _cabi.E_UNSUPPORTED and "fit_im" in str(ei.value)
            with pytest.raises(_cabi.NmrfitError):
                fb.uncertainty(X, 1.0, 1.0)
            assert len(fb.normal_equations(X, channels="both")) == 2
            fb.run(2, 1)
    with make(False) as fb:
        good = fb.sandwich(X, 1.0, 2.0)
        for bad in (-1.0, float("nan"), float("inf")):
            with pytest.raises(_cabi.NmrfitError) as ei:
                fb.sandwich(X, [1.0, bad], 1.0)
            assert ei.value.code == _cabi.E_INVALID
        rows = np.concatenate([lsq.forward_rows(x, sp["lower"], sp["upper"])[0].ravel() for x, sp in zip(X, specs)])
        cc = np.ones(sum(fb.D))
        ss = np.ones(2)
        out = np.empty(sum(d * d for d in fb.D))
        args = [_cabi.ptr(a) for a in (rows, cc, ss, ss, ss)]
        for null in range(5):
            call = list(args)
            call[null] = None
            assert L.nmrfit_batch_sandwich(fb._h, *call, _cabi.ptr(out), None, None, None) == _cabi.E_INVALID, null
        assert _same(fb.sandwich(X, 1.0, 2.0)[1], good[1])
        # every output pointer may be NULL, and any subset gives the bits of the full call
        A, M, g, f = fb.sandwich(X, 1.0, 2.0)[0]
        only = np.empty(sum(d * d for d in fb.D))
        s = 1.0 / np.sqrt(fb.Ns.astype(np.float64))
        cs_ = np.concatenate([s[k] / lsq.forward_rows(x, sp["lower"], sp["upper"])[1] for k, (x, sp) in enumerate(zip(X, specs))])
        su, sv = np.full(2, 1.0), np.full(2, 2.0)
        assert L.nmrfit_batch_sandwich(fb._h, _cabi.ptr(rows), _cabi.ptr(cs_), _cabi.ptr(s), _cabi.ptr(su), _cabi.ptr(sv), None,
                                       _cabi.ptr(only), None, None) == _cabi.OK
        assert np.array_equal(only[:fb.D[0] ** 2].reshape(fb.D[0], fb.D[0]), M)
        assert L.nmrfit_batch_sandwich(fb._h, _cabi.ptr(rows), _cabi.ptr(cs_), _cabi.ptr(s), _cabi.ptr(su), _cabi.ptr(sv), None,
                                       None, None, None) == _cabi.OK
        fb.run(2, 1)
        assert all(np.isfinite(fx) for _, fx in fb.best())
    sp, x = specs[1], X[1]
    with Evaluator(*spectrum_tuple(sp)) as ev:
        m = lsq.ResidualModel(ev, sp["lower"], sp["upper"])
        good = m.sandwich(x, 1.0, 2.0)
        ev.set_variant(_cabi.VARIANT_FARFIELD)
        with pytest.raises(_cabi.NmrfitError) as ei:
            m.sandwich(x, 1.0, 2.0)
        assert ei.value.code == _cabi.E_UNSUPPORTED
        ev.set_variant(_cabi.VARIANT_DEFAULT)
        with pytest.raises(_cabi.NmrfitError) as ei:
            m.sandwich(x, -1.0, 2.0)
        assert ei.value.code == _cabi.E_INVALID
        rows, h = m.rows(x)
        c = np.ascontiguousarray(m._scale / h)
        for r_, c_ in ((None, _cabi.ptr(c)), (_cabi.ptr(rows), None)):
            assert L.nmrfit_sandwich(ev.handle, 2, r_, c_, m._scale, 1.0, 2.0, None, None, None, None) == _cabi.E_INVALID
        assert _same(m.sandwich(x, 1.0, 2.0), good)
        M = np.empty((len(x), len(x)))      # the meat alone
        assert L.nmrfit_sandwich(ev.handle, 2, _cabi.ptr(rows), _cabi.ptr(c), m._scale, 1.0, 2.0, None, _cabi.ptr(M), None,
                                 None) == _cabi.OK
        assert np.array_equal(M, good[1])
        with pytest.raises(ValueError):
            lsq.ResidualModel(ev, sp["lower"], sp["upper"], fit_im=True).sandwich(x, 1.0, 2.0)

"""
GPU tier of the two-channel sandwich (csrc/lsq_cov_im.hip, include/nmrfit_amd_cov_im.h, nmrfit_amd/uncertainty.py): the
device's three blocks against numpy at the shapes where the kernel can go wrong, the corner of Mt_rr against
nmrfit_sandwich's bits, A, g and rho against nmrfit_batch_normal_equations_im's bits, the same bits alone and anywhere in
any batch, the refusals, the records against the CPU mirror and a replica study, and fit_many(uncertainty=dict(...,
channels="both")) on a mixed list.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import nmrfit_amd
from nmrfit_amd import _cabi, lsq, noise, synth, uncertainty
from nmrfit_amd.equations import Evaluator

from . import calibration_support as cs
from . import uncertainty_im_support as U
from .lsq_support import spectrum_tuple

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("mode", U.MODES)
@pytest.mark.parametrize("N,P", U.DEVICE_SHAPES)
def test_blocks_against_numpy(N, P, mode):
    """The device's Mt_rr, Mt_ii, Mt_ri against numpy's (q Jt_a)^T Jt_b made from the device's OWN J and r and numpy's
    q_ab, sigma_v = 2 sigma_u, entry by entry within the derived bound (uncertainty_im_support.blocks_bound); the
    symmetric blocks symmetric to the bit; the D x D corner of Mt_rr nmrfit_sandwich's M to the bit; A, g and rho
    nmrfit_jacobian_im's bits; with sigma_u == sigma_v the cross block exactly zero and the corner still the real
    channel's."""
    sp, x, (su, sv) = U.device_problem(N, P)
    s = 1.0 / np.sqrt(N)
    D = 4 + 3 * P
    with Evaluator(*spectrum_tuple(sp)) as ev:
        rows, h = lsq.ResidualModel(ev, sp["lower"], sp["upper"]).rows(x)
        ref = ev.jacobian_im(rows, s / h, s, mode, J=True, r=True, normal=True)
        got = ev.sandwich_im(rows, s / h, s, mode, su, sv)
        real = ev.sandwich(rows, s / h, s, su, sv)
        equal = ev.sandwich_im(rows, s / h, s, mode, sv, sv)
        real_equal = ev.sandwich(rows, s / h, s, sv, sv)
    Jt = [np.column_stack((ref["J"][ch], ref["r"][ch])) for ch in (0, 1)]
    q = uncertainty.residual_covariances(sp["weights"], x, su, sv)
    want = uncertainty.sandwich_host_im(ref["J"][0], ref["r"][0], ref["J"][1], ref["r"][1], sp["weights"], x, su, sv)
    assert got["M"].shape == (3, D + 1, D + 1) and np.all(np.isfinite(got["M"]))
    for k, (kind, a, b) in enumerate((("rr", 0, 0), ("ii", 1, 1), ("ri", 0, 1))):
        assert np.array_equal(want[k], (q[k][:, None] * Jt[a]).T @ Jt[b])
        bound = U.blocks_bound(Jt[a], Jt[b], q[k], kind, sp["weights"], x, su, sv)
        err = np.abs(got["M"][k] - want[k])
        some = bound > 0.0      # (the offset does not reach the imaginary channel: its row and column of J_im are zeros, exactly)
        print("N=%d D=%d mode %d %s: worst |Mt_dev - Mt_numpy| / bound %.3g" % (N, D, mode, kind, np.max(err[some] / bound[some])))
        assert np.all(err <= bound), (kind, float(np.max(err[some] / bound[some])))
    assert np.array_equal(got["M"][0], got["M"][0].T) and np.array_equal(got["M"][1], got["M"][1].T)
    assert np.any(got["M"][2] != got["M"][2].T)
    assert np.array_equal(got["M"][0][:D, :D], real["M"])
    for name, key in (("A", "A"), ("g", "g"), ("f2", "f2")):
        assert np.array_equal(got[name], ref[key]), name
    assert np.array_equal(got["A"][0], real["A"]) and np.array_equal(got["g"][0], real["g"])
    assert not np.any(equal["M"][2]) and np.array_equal(equal["M"][0][:D, :D], real_equal["M"])
    assert np.array_equal(equal["A"], got["A"])


@pytest.fixture(scope="module")
def record():
    """uncertainty_im_support.device_record() of this process (computed once, read-only)."""
    rec = U.device_record()
    for a in rec.values():
        a.setflags(write=False)
    return rec


@pytest.mark.parametrize("mode", U.MODES)
def test_ragged_batch_and_the_normal_equations(mode):
    """A ragged batch of three fits of different N and P: every fit's record the lone context's to the bit, in every
    position of the batch and from call to call; A, g and rho the bits of nmrfit_batch_normal_equations_im itself; any
    subset of the outputs the bits of the full call.  (Groups and parts: test_groups_and_parts.)"""
    probs = [U.device_problem(N, P) for N, P in U.RAGGED]
    lone = [U.flat(*U.lone_sandwich_im(sp, x, mode, sig)) for sp, x, sig in probs]
    for order in ((0, 1, 2), (1, 2, 0), (2, 0, 1)):
        with U.batch_of([probs[k][0] for k in order], mode) as fb:
            X = [probs[k][1] for k in order]
            su, sv = [probs[k][2][0] for k in order], [probs[k][2][1] for k in order]
            got = fb.sandwich_im(X, su, sv)
            again = fb.sandwich_im(X, su, sv)
            combined = fb.normal_equations(X, channels="both")
            raw = U.raw_normal_equations_im(fb, X)
            if order == (0, 1, 2):
                # the meat alone, and nothing at all
                Dk = np.asarray(fb.D, dtype=np.int64)
                rows = np.concatenate([lsq.forward_rows(x, sp["lower"], sp["upper"])[0].ravel() for sp, x, _ in probs])
                s = 1.0 / np.sqrt(fb.Ns.astype(np.float64))
                c = np.concatenate([s[k] / lsq.forward_rows(x, sp["lower"], sp["upper"])[1] for k, (sp, x, _) in enumerate(probs)])
                only = np.empty(int(np.sum(3 * (Dk + 1) ** 2)))
                L = _cabi.lib()
                su_, sv_ = np.array(su), np.array(sv)
                args = [_cabi.ptr(a) for a in (rows, c, s, su_, sv_)]
                assert L.nmrfit_batch_sandwich_im(fb._h, *args, None, None, None, _cabi.ptr(only)) == _cabi.OK
                assert np.array_equal(only, np.concatenate([lone[k]["M"].ravel() for k in range(3)]))
                assert L.nmrfit_batch_sandwich_im(fb._h, *args, None, None, None, None) == _cabi.OK
        for place, k in enumerate(order):
            assert U.same_bits(U.flat(*got[place]), lone[k]) and U.same_bits(U.flat(*again[place]), lone[k]), (order, k)
            mine = U.flat(*got[place])
            assert all(np.array_equal(mine[name], raw[place][name]) for name in ("A", "g", "rho")), (order, k)
            H, grad, f = lsq.combine_channels(got[place][0])
            assert np.array_equal(H, combined[place][0]) and np.array_equal(grad, combined[place][1]) and f == combined[place][2]


@pytest.mark.parametrize("mode", U.MODES)
def test_groups_and_parts(mode, monkeypatch):
    """Seven fits of three shapes in one batch, which the library divides over two parts, under two workspace groupings:
    the default budget (one group per part) and NMRFIT_LSQ_WORKSPACE_MB=1, under which any two of the fits exceed the
    budget and every fit is a group of its own (uncertainty_im_support.GROUP_SHAPES).  Every fit's A, g, rho and blocks
    are the lone context's to the bit wherever its share of the outputs lies -- behind another part's, behind other
    groups' -- and A, g and rho are the bits of nmrfit_batch_normal_equations_im itself under the same grouping."""
    probs = [U.device_problem(N, P) for N, P in U.GROUP_SHAPES]
    rows = sorted(2 * (4 + 3 * P + 1) * N for N, P in U.GROUP_SHAPES)
    assert rows[0] + rows[1] > (1 << 17) and len(U.GROUP_ORDER) >= 6      # (1 MiB of doubles; two parts from six fits on)
    lone = [U.flat(*U.lone_sandwich_im(sp, x, mode, sig)) for sp, x, sig in probs]
    order = U.GROUP_ORDER
    X = [probs[k][1] for k in order]
    su, sv = [probs[k][2][0] for k in order], [probs[k][2][1] for k in order]
    with U.batch_of([probs[k][0] for k in order], mode) as fb:
        for budget in (None, "1"):
            if budget is not None:
                monkeypatch.setenv("NMRFIT_LSQ_WORKSPACE_MB", budget)
            got = fb.sandwich_im(X, su, sv)
            raw = U.raw_normal_equations_im(fb, X)
            for place, k in enumerate(order):
                mine = U.flat(*got[place])
                assert np.all(np.isfinite(mine["M"])) and U.same_bits(mine, lone[k]), (budget, place, k)
                assert all(np.array_equal(mine[name], raw[place][name]) for name in ("A", "g", "rho")), (budget, place, k)
        monkeypatch.delenv("NMRFIT_LSQ_WORKSPACE_MB")


def test_same_bits_from_call_to_call(record):
    """The record of this process again; alone on a context and in the batch the same bits."""
    again = U.device_record()
    assert sorted(again) == sorted(record) and all(np.array_equal(again[k], record[k]) for k in record)
    for k in range(len(U.RAGGED)):
        for name in ("A", "g", "rho", "M"):
            a, b = record["lone.%d.%s" % (k, name)], record["batch.%d.%s" % (k, name)]
            assert np.all(np.isfinite(a)) and np.array_equal(a, b), (k, name)


@pytest.mark.parametrize("poison", ("255", "63"))
def test_same_bits_under_poisoned_allocations(record, poison, tmp_path):
    """NMRFIT_POISON_ALLOC=255 (every fresh double a NaN) and 63 (a plausible finite value), each in a fresh child
    process: the record of this process, byte for byte -- no bit of A, g, rho or the blocks leans on what a fresh block
    of memory holds."""
    out = str(tmp_path / "record.npz")
    env = dict(os.environ, NMRFIT_POISON_ALLOC=poison)
    run = subprocess.run([sys.executable, "-m", "tests.uncertainty_im_support", out], cwd=ROOT, env=env, capture_output=True,
                         text=True, timeout=120)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-3000:]
    with np.load(out) as child:
        assert sorted(child.files) == sorted(record)
        for k in record:
            assert child[k].tobytes() == record[k].tobytes(), k


def test_refusals():
    """A fit_im = 0 batch is NMRFIT_E_INVALID, a context set to another kernel variant NMRFIT_E_UNSUPPORTED, more than 24
    peaks NMRFIT_E_UNSUPPORTED; null required pointers, a bad mode and a bad sigma NMRFIT_E_INVALID; after each the batch
    / context works and gives the bits it gave before.  (The NMRFIT_E_STATE of a reconstruction in flight cannot be
    reached from a test: the reconstruction begins and ends inside one call of the library.)"""
    specs = [synth.make_spectrum(n, p, seed=30 + p, noise=1e-3, physical=True) for n, p in ((300, 1), (513, 2))]
    X = [sp["x_true"] for sp in specs]
    L = _cabi.lib()
    with U.batch_of(specs, 0) as fb:
        with pytest.raises(_cabi.NmrfitError) as ei:
            fb.sandwich_im(X, 1.0, 1.0)
        assert ei.value.code == _cabi.E_INVALID and "fit_im = 0" in str(ei.value)
        with pytest.raises(_cabi.NmrfitError):
            fb.uncertainty(X, 1.0, 1.0, channels="both")
        assert len(fb.sandwich(X, 1.0, 2.0)) == 2
        fb.run(2, 1)
    with U.batch_of(specs, "sum") as fb:
        good = [U.flat(*pm) for pm in fb.sandwich_im(X, 1.0, 2.0)]
        for bad in (-1.0, float("nan"), float("inf")):
            with pytest.raises(_cabi.NmrfitError) as ei:
                fb.sandwich_im(X, [1.0, bad], 1.0)
            assert ei.value.code == _cabi.E_INVALID
            with pytest.raises(_cabi.NmrfitError) as ei:
                fb.sandwich_im(X, 1.0, [bad, 1.0])
            assert ei.value.code == _cabi.E_INVALID
        rows = np.concatenate([lsq.forward_rows(x, sp["lower"], sp["upper"])[0].ravel() for x, sp in zip(X, specs)])
        cc, ss = np.ones(sum(fb.D)), np.ones(2)
        out = np.empty(sum(3 * (d + 1) ** 2 for d in fb.D))
        args = [_cabi.ptr(a) for a in (rows, cc, ss, ss, ss)]
        for null in range(5):
            call = list(args)
            call[null] = None
            assert L.nmrfit_batch_sandwich_im(fb._h, *call, None, None, None, _cabi.ptr(out)) == _cabi.E_INVALID, null
        with pytest.raises(_cabi.NmrfitError):      # (the real channel's call still refuses the batch)
            fb.sandwich(X, 1.0, 2.0)
        assert all(U.same_bits(U.flat(*pm), g) for pm, g in zip(fb.sandwich_im(X, 1.0, 2.0), good))
        fb.run(2, 1)
        assert all(np.isfinite(fx) for _, fx in fb.best())
    big = synth.make_spectrum(130, 25, seed=4, noise=1e-3, physical=True)
    with U.batch_of([specs[0], big], True) as fb:
        with pytest.raises(_cabi.NmrfitError) as ei:
            fb.sandwich_im([X[0], big["x_true"]], 1.0, 1.0)
        assert ei.value.code == _cabi.E_UNSUPPORTED
        fb.run(2, 1)
    sp, x = specs[1], X[1]
    with Evaluator(*spectrum_tuple(sp)) as ev:
        m = lsq.ResidualModel(ev, sp["lower"], sp["upper"], fit_im="sum")
        good = U.flat(*m.sandwich_im(x, 1.0, 2.0))
        ev.set_variant(_cabi.VARIANT_FARFIELD)
        with pytest.raises(_cabi.NmrfitError) as ei:
            m.sandwich_im(x, 1.0, 2.0)
        assert ei.value.code == _cabi.E_UNSUPPORTED
        ev.set_variant(_cabi.VARIANT_DEFAULT)
        with pytest.raises(_cabi.NmrfitError) as ei:
            m.sandwich_im(x, -1.0, 2.0)
        assert ei.value.code == _cabi.E_INVALID
        rows, h = m.rows(x)
        c = np.ascontiguousarray(m._scale / h)
        for r_, c_ in ((None, _cabi.ptr(c)), (_cabi.ptr(rows), None)):
            assert L.nmrfit_sandwich_im(ev.handle, 2, 2, r_, c_, m._scale, 1.0, 2.0, None, None, None, None) == _cabi.E_INVALID
        for bad_mode in (0, 3, -1):
            assert L.nmrfit_sandwich_im(ev.handle, 2, bad_mode, _cabi.ptr(rows), _cabi.ptr(c), m._scale, 1.0, 2.0, None, None,
                                        None, None) == _cabi.E_INVALID
        assert U.same_bits(U.flat(*m.sandwich_im(x, 1.0, 2.0)), good)
        M = np.empty((3, len(x) + 1, len(x) + 1))      # the blocks alone
        assert L.nmrfit_sandwich_im(ev.handle, 2, 2, _cabi.ptr(rows), _cabi.ptr(c), m._scale, 1.0, 2.0, None, None, None,
                                    _cabi.ptr(M)) == _cabi.OK
        assert np.array_equal(M, good["M"])
        with pytest.raises(ValueError):      # (the existing refusal stays)
            m.sandwich(x, 1.0, 2.0)


@pytest.mark.parametrize("mode", U.MODES)
def test_records_against_the_cpu_mirror(mode):
    """FitBatch.uncertainty(channels="both") at the CPU base's minimiser, sigma_v = sigma_u and 2 sigma_u in ONE batch (no
    fitting: X is given), against the CPU mirror.  The device's rows and the closed form are two float64 evaluations of
    the same residual: they differ by roundings, ~ 1e2 eps of the terms' magnitude, and a forward difference divides that
    by h = 1.5e-8 -- a few 1e-6 of a Jacobian entry's scale, which the sandwich carries into the standard errors.  So the
    device's per-parameter deviations from the linear-response truth are the mirror's to the fourth digit (1e-4 of a
    standard error), and it keeps the mirror's bars; standard errors and the area fraction's agree to 1e-4 relative;
    nothing is fixed and x0 is the device's minimiser too."""
    ps = [U.problem(mode, ratio) for ratio in U.RATIOS]
    with U.batch_of([p.sp for p in ps], mode) as fb:
        got = fb.uncertainty([p.x0 for p in ps], [p.sigma_u for p in ps], [p.sigma_v for p in ps], channels="both")
    for p, fu in zip(ps, got):
        cpu, G = U.mirror(p.sp, p.x0, mode, p.sigma_u, p.sigma_v)
        truth = U.response_truth(mode, p.ratio)
        dev = np.max([np.abs(U.predicted_shift(fu, G, *p.direction(seed)) - want) / cpu.params_std
                      for seed, want in zip(U.DIRECTION_SEEDS, truth)], axis=0)
        ref = U.response_deviation(mode, p.ratio)
        rel = float(np.max(np.abs(fu.params_std / cpu.params_std - 1.0)))
        af = abs(fu.area_fraction_std / cpu.area_fraction_std - 1.0)
        print("mode %d ratio %g: |deviation_dev - deviation_cpu| %.3g; params_std rel %.3g, area fraction %.3g; distance %.3g"
              % (mode, p.ratio, float(np.max(np.abs(dev - ref))), rel, af, fu.distance))
        assert fu.status == "ok" and fu.channels == "both" and not fu.fixed.any() and fu.sigma == (p.sigma_u, p.sigma_v)
        assert np.all(np.abs(dev - ref) <= 1e-4) and np.all(dev <= U.response_bar(mode, p.ratio))
        assert rel <= 1e-4 and af <= 1e-4
        assert fu.distance < 1e-3, fu.distance
        assert fu.area_fraction == uncertainty.area_fraction(p.x0) and fu.rho == tuple(q[2] for q in fu.parts)


def test_end_to_end():
    """63 replicas of the CPU base (N = 512, P = 2, mode 2, sigma_v = 2 sigma_u) made on the device (noise.replicas, seeds
    REPLICA_SEED0 + k) and refitted as ONE batch by FitBatch.polish(channels="both") from the base's minimiser -- no
    swarm result is used: the batch takes one generation of eight particles only because polish reads best() first.
    The replicas' variance over params_std^2 of the base's device record, per parameter and for the area fraction, lies
    inside the two-sided 1e-6 quantiles of chi^2_62 / 62.  (How far the device's minimisers lie from the CPU study's, in
    standard errors, is printed: the device's deviates are the host mirror's up to the last bits of log, sin and cos.)"""
    mode = 2
    p = U.problem(mode, 2.0)
    seeds = [U.REPLICA_SEED0 + k for k in range(U.REPLICAS)]
    uv = noise.replicas([p.sp["u"]] * U.REPLICAS, [p.sp["v"]] * U.REPLICAS, p.sigma_u, p.sigma_v, seeds)
    with U.batch_of([p.sp], mode) as fb:
        fu = fb.uncertainty([p.x0], p.sigma_u, p.sigma_v, channels="both")[0]
    with U.batch_of([dict(p.sp, u=u, v=v) for u, v in uv], mode) as fb:
        fb.run(1, 1)
        out = fb.polish([p.x0] * U.REPLICAS, channels="both", max_launches=100)
        info = fb.last_polish
    X = np.array([x for x, _ in out])
    ratio = np.var(X, axis=0, ddof=1) / fu.params_std ** 2
    af = np.var([uncertainty.area_fraction(x) for x in X], ddof=1) / fu.area_fraction_std ** 2
    lo, hi = cs.chi2_quantiles(U.REPLICAS - 1)
    gap = float(np.max(np.abs(X - U.replica_minimisers(mode)) / fu.params_std))
    print("var(replicas) / params_std^2 in %.3f .. %.3f, area fraction %.3f; quantiles (%.3f, %.3f); %d launches, stops %s; "
          "device minimisers within %.3g standard errors of the CPU's"
          % (ratio.min(), ratio.max(), af, lo, hi, info["launches"], sorted(set(info["stop"])), gap))
    assert fu.status == "ok" and not fu.fixed.any()
    assert np.all((ratio > lo) & (ratio < hi)) and lo < af < hi


def test_fit_many_on_a_mixed_list():
    """fit_many(jobs, batch_polish="both", uncertainty=dict(sigma=..., channels="both")) on fit_im False, True and "sum"
    jobs, two of each: every fit carries a record; the fit_im=False fits carry the bits of the same call without
    ``channels``; the fit_im fits the two-channel record; params and error are the plain call's; a fit that ran alone gets the batch's record to the bit; without channels="both" the call is refused."""
    p = U.problem(2, 2.0)
    sigma = (p.sigma_u, p.sigma_v)
    data = synth.SynthData(p.sp["w"], p.sp["u"], p.sp["v"], p.sp["peaks"])
    opts = {'maxiter': 30, 'swarmsize': 32, 'polish': True}
    jobs = [dict(data=data, lower=p.lower, upper=p.upper, fit_im=fit_im, options=dict(opts, seed=seed))
            for fit_im in (False, True, "sum") for seed in (1, 2)]
    fits = nmrfit_amd.fit_many(jobs, batch_polish="both", uncertainty=dict(sigma=sigma, channels="both"))
    plain = nmrfit_amd.fit_many(jobs, batch_polish="both")
    real = nmrfit_amd.fit_many(jobs[:2], batch_polish="both", uncertainty=dict(sigma=sigma))
    with pytest.raises(ValueError, match="real channel"):
        nmrfit_amd.fit_many(jobs, batch_polish="both", uncertainty=dict(sigma=sigma))
    for k, (f, q) in enumerate(zip(fits, plain)):
        fu = f.uncertainty
        assert isinstance(fu, uncertainty.FitUncertainty) and fu.status == "ok" and fu.sigma == sigma
        assert np.array_equal(f.params, q.params) and f.error == q.error and np.array_equal(fu.x, f.params)
        print("job %d fit_im=%r: distance %.3g, params_std %s" % (k, jobs[k]["fit_im"], fu.distance, np.round(fu.params_std, 8)))
        if k < 2:
            assert not hasattr(fu, "channels")
            for name in ("A", "M", "g", "cov", "params_std", "newton_step"):
                assert np.array_equal(getattr(fu, name), getattr(real[k].uncertainty, name)), name
        else:
            assert fu.channels == "both" and len(fu.rho) == 2 and all(r > 0.0 for r in fu.rho)
            # (error is the objective the swarm and the polish minimised: the record's two norms are its halves)
            assert abs(f.error - 0.5 * (fu.rho[0] + fu.rho[1])) <= 1e-12 * f.error
    lone = nmrfit_amd.utils.FitUtility.uncertainty(fits[4], sigma=sigma, channels="both")
    assert np.array_equal(lone.cov, fits[4].uncertainty.cov) and np.array_equal(lone.M, fits[4].uncertainty.M)
    with pytest.raises(ValueError, match="real channel"):
        nmrfit_amd.utils.FitUtility.uncertainty(fits[4], sigma=sigma)

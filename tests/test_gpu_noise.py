"""
GPU tier of the noise replicas (csrc/noise.hip, include/nmrfit_amd_noise.h; nmrfit_amd/noise.py, FitBatch.add_noise /
spectrum, nmrfit_amd.fit_replicas): the device's deviates against the numpy mirror and against 200-bit truth, the
in-place path against the out-of-place one bit for bit, the fits that follow, the state rule, and the whole call.
"""
import numpy as np
import pytest

import nmrfit_amd
from nmrfit_amd import _cabi, noise, synth
from nmrfit_amd.batch import FitBatch
from tests import calibration_support as C
from tests import noise_support as T

pytestmark = pytest.mark.gpu

# The device's worst error against the 200-bit truth on the 2000 points of seed 7, in units of e = 2^-52 max(1, r),
# measured on the MI355X (test_truth prints it; the truth is rounded to fp64, so the figure is a whole number of ulps of
# the worst point: two ulps of a z_v of 0.94, the mirror's worst point too): B_MEASURED = 1.000 e.  The bound is twice
# that, rounded up: B = 2 e.
B_MEASURED = 1.000
B = 2.0

NS = (300, 513, 1025, 512, 64, 1000, 2048)       # seven fits: two parts; lengths around the 512-point chunk
PS = (1, 2, 3, 1, 1, 2, 1)
SIGMA_U = np.array([2e-3, 1e-3, 0.0, 5e-4, 3e-3, 0.0, 1e-3])
SIGMA_V = np.array([1e-3, 3e-3, 0.0, 5e-4, 0.0, 0.0, 2e-3])      # fits 2 and 5: sigma 0; fit 4: one channel only
SEEDS = [11, 12, 13, (1 << 32) + 14, 15, 16, (1 << 63) + 17]


@pytest.fixture(scope="module")
def seven():
    """The seven spectra, and their replicas made out of place (read-only: shared between the tests)."""
    specs = [synth.make_spectrum(n, p, seed=20 + k, physical=True) for k, (n, p) in enumerate(zip(NS, PS))]
    noisy = noise.replicas([s["u"] for s in specs], [s["v"] for s in specs], SIGMA_U, SIGMA_V, SEEDS)
    for a, b in noisy:
        a.setflags(write=False)
        b.setflags(write=False)
    return specs, noisy


def make_batch(specs, uv=None, fit_im=False):
    uv = [(s["u"], s["v"]) for s in specs] if uv is None else uv
    return FitBatch([(s["w"], u, v, s["weights"]) for s, (u, v) in zip(specs, uv)], [s["lower"] for s in specs],
                    [s["upper"] for s in specs], swarmsize=16, seeds=[101 + k for k in range(len(specs))], fit_im=fit_im)


def same_best(a, b):
    return all(np.array_equal(xa, xb) and fa == fb for (xa, fa), (xb, fb) in zip(a, b))


def test_mirror():
    """noise.replicas against replicas_host on lengths around the 512-point chunk: every value within
    (B + 1) e sigma + ulp(|out|) (device within B e of the truth, mirror within 1 e, one rounding of the sum); sigma 0
    untouched; the same bytes again, and alone."""
    Ns = (1, 511, 512, 513, 1025)
    rng = np.random.default_rng(4)
    us = [rng.standard_normal(n) for n in Ns]
    vs = [rng.standard_normal(n) for n in Ns]
    us[1][5], vs[3][7], us[2][0] = np.nan, np.nan, -0.0
    su = np.array([0.5, 2.0, 0.0, 1e-3, 0.25])
    sv = np.array([0.25, 1.0, 0.0, 2e-3, 4.0])
    seeds = [1, 2, 3, (1 << 32) + 5, (1 << 40) + 1]
    got = noise.replicas(us, vs, su, sv, seeds)
    want = noise.replicas_host(us, vs, su, sv, seeds)
    worst = 0.0
    for k, n in enumerate(Ns):
        zu, zv = noise.normals(seeds[k], n)
        e = 2.0 ** -52 * np.maximum(1.0, np.hypot(zu, zv))
        for g, w, s in ((got[k][0], want[k][0], su[k]), (got[k][1], want[k][1], sv[k])):
            assert g.shape == (n,)
            ok = np.isfinite(w)
            assert np.array_equal(np.isnan(g), ~ok)                       # NaN passes through, and nothing else is one
            tol = (B + 1.0) * e * s + np.spacing(np.abs(w))
            assert np.all(np.abs(g - w)[ok] <= tol[ok]), (k, np.max((np.abs(g - w) / tol)[ok]))
            worst = max(worst, float(np.max((np.abs(g - w) / tol)[ok])))
    print("device against mirror: worst |difference| / tolerance = %.3f" % worst)
    assert got[2][0].tobytes() == us[2].tobytes() and got[2][1].tobytes() == vs[2].tobytes()      # sigma 0: the bits stay
    again = noise.replicas(us, vs, su, sv, seeds)
    assert all(a.tobytes() == c.tobytes() and b.tobytes() == d.tobytes() for (a, b), (c, d) in zip(got, again))
    for k in range(len(Ns)):
        (a, b), = noise.replicas([us[k]], [vs[k]], su[k], sv[k], [seeds[k]])
        assert a.tobytes() == got[k][0].tobytes() and b.tobytes() == got[k][1].tobytes(), k


def test_truth():
    """u = v = 0, sigma = 1: the output is z itself.  Its worst error against the 200-bit values is printed and must
    stay within B e (B: twice the measured worst, rounded up)."""
    n = T.TRUTH_N
    (zu, zv), = noise.replicas([np.zeros(n)], [np.zeros(n)], 1.0, 1.0, [T.TRUTH_SEED])
    worst = T.worst_error(zu, zv)
    print("device: worst error %.3f e (B_MEASURED %.3f, B %.1f)" % (worst, B_MEASURED, B))
    assert worst <= 8.0, "more than the rounding of log, sin and cos is wrong"
    assert worst <= B


def test_in_place(seven):
    """FitBatch.add_noise on seven fits in two parts: spectrum(k) is noise.replicas of the same inputs bit for bit;
    before the call, and for the sigma-0 fits after it, it is what was uploaded."""
    specs, noisy = seven
    with make_batch(specs) as fb:
        for k, s in enumerate(specs):
            u, v = fb.spectrum(k)
            assert u.tobytes() == s["u"].tobytes() and v.tobytes() == s["v"].tobytes(), k
        fb.add_noise(SIGMA_U, SIGMA_V, SEEDS)
        for k, s in enumerate(specs):
            u, v = fb.spectrum(k)
            assert np.array_equal(u, noisy[k][0]) and np.array_equal(v, noisy[k][1]), k
            if k in (2, 5):
                assert u.tobytes() == s["u"].tobytes() and v.tobytes() == s["v"].tobytes(), k
            else:
                assert not np.array_equal(u, s["u"]), k
        assert np.array_equal(fb.spectrum(4)[1], specs[4]["v"])          # sigma_v = 0: v + 0 * z_v


@pytest.mark.parametrize("fit_im", [False, True])
def test_chain(seven, fit_im):
    """The fits that follow: a batch uploaded with the host copies of the replicas and a batch perturbed in place give
    the same best() after 30 generations; with every sigma 0 the call changes nothing.  Real channel: two replicas of
    ONE spectrum under different noise seeds move as their own noise predicts, each its own way (``check_two_seeds``)."""
    specs, noisy = seven
    with make_batch(specs, uv=noisy, fit_im=fit_im) as fa, make_batch(specs, fit_im=fit_im) as fb:
        fb.add_noise(SIGMA_U, SIGMA_V, SEEDS)
        fa.run(maxiter=30)
        fb.run(maxiter=30)
        a, b = fa.best(), fb.best()
    assert same_best(a, b)
    with make_batch(specs, fit_im=fit_im) as fc, make_batch(specs, fit_im=fit_im) as fd:
        fc.add_noise(0.0, 0.0, SEEDS)
        fc.run(maxiter=30)
        fd.run(maxiter=30)
        c, d = fc.best(), fd.best()
    assert same_best(c, d)
    assert not same_best(a, c)                                            # (the noise does reach the fits)
    if not fit_im:
        check_two_seeds()


def check_two_seeds():
    """Replicas 1 and 2 of tests/calibration_support.py's first case (an exactly fitted spectrum, noise seeds 101 and
    102), run and polished beside the unperturbed fit: D_k = x_k - x0 is within the bar of the linear response to its own
    noise, so the two are as uncorrelated as their predictions -- sum_i D_1i D_2i / sigma_x,i^2 equals the predictions'
    within b (|L_1| + |L_2|) + b^2 per parameter -- and not one draw used twice."""
    c, t = C.case("n512_p2"), C.truth("n512_p2")
    b = C.bar(c)
    with FitBatch([c.spectrum_tuple()] * 3, [c.lower] * 3, [c.upper] * 3, swarmsize=64, seeds=c.seeds[:3]) as fb:
        fb.add_noise([0.0, c.sigma_u, c.sigma_u], [0.0, c.sigma_v, c.sigma_v], c.seeds[:3])
        fb.run()
        got = fb.polish(max_launches=200, ftol=C.FTOL)
        assert all(st in ("ftol", "lambda") for st in fb.last_polish["stop"])      # (converged: not the budget)
    d = (np.array([x for x, _ in got])[1:] - t.x0) / t.sigma_x
    lin = t.lin[:2] / t.sigma_x
    assert np.all(np.abs(d - lin) <= b)
    tol = np.sum(b * (np.abs(lin[0]) + np.abs(lin[1])) + b * b)
    print("two seeds: sum D_1 D_2 / sigma_x^2 = %.4f, predicted %.4f, tolerance %.4f; against one draw twice: %.4f"
          % (d[0] @ d[1], lin[0] @ lin[1], tol, lin[0] @ lin[0]))
    assert abs(d[0] @ d[1] - lin[0] @ lin[1]) <= tol
    assert abs(lin[0] @ lin[0] - lin[0] @ lin[1]) > tol                   # (the check tells the two apart)


def test_state(seven):
    """Once, and only before generation 0; a bad k is invalid; the batch runs and closes cleanly afterwards."""
    specs, _ = seven
    with make_batch(specs) as fb:
        fb.add_noise(SIGMA_U, SIGMA_V, SEEDS)
        with pytest.raises(_cabi.NmrfitError) as ei:
            fb.add_noise(SIGMA_U, SIGMA_V, SEEDS)
        assert ei.value.code == _cabi.E_STATE
        for k in (-1, len(specs)):
            with pytest.raises(_cabi.NmrfitError) as ei:
                fb.spectrum(k)
            assert ei.value.code == _cabi.E_INVALID
        fb.run(maxiter=3)
        assert all(np.isfinite(f) for _, f in fb.best())
    with make_batch(specs) as fb:
        fb.run(maxiter=1)
        with pytest.raises(_cabi.NmrfitError) as ei:
            fb.add_noise(SIGMA_U, SIGMA_V, SEEDS)
        assert ei.value.code == _cabi.E_STATE
        with pytest.raises(_cabi.NmrfitError) as ei:
            fb.add_noise(-1.0, 0.0, SEEDS)
        assert ei.value.code == _cabi.E_INVALID
        u, v = fb.spectrum(6)                                             # any state
        assert u.tobytes() == specs[6]["u"].tobytes() and v.tobytes() == specs[6]["v"].tobytes()
        fb.run(maxiter=2)
        assert len(fb.status()) == len(specs) and all(np.isfinite(f) for _, f in fb.best())


def test_end_to_end():
    """fit_replicas: fit 0 is the lone fit bit for bit, the call repeats, the data is not written; fit_replicas_many
    gives job 0 the same params.  The spread: with ``options['polish']`` every noisy fit is within the bar of the Newton
    prediction of its own noise (tests/calibration_support.py, case "end_to_end": this spectrum, these seeds; the base is
    noisy, so the prediction takes the full Hessian) and ``params_std`` / ``area_fraction_std`` are the predictions'
    spreads within the bar's propagation; the swarm alone (this test's 64 particles, 300 generations) never has the
    smaller error and its spread is printed beside them."""
    opts = {'swarmsize': 64, 'maxiter': 300}
    spec = synth.make_spectrum(1024, 2, noise=1e-3, physical=True)
    data = synth.SynthData(spec["w"], spec["u"], spec["v"], spec["peaks"])
    u0, v0 = data.u.copy(), data.v.copy()
    rf = nmrfit_amd.fit_replicas(data, spec["lower"], spec["upper"], replicas=8, sigma=spec["sigma"], seed=11, options=opts)
    lone = nmrfit_amd.fit(data, spec["lower"], spec["upper"], summary=False, options=dict(opts, seed=11))
    assert len(rf.fits) == 9 and rf.params.shape == (9, 10)
    assert np.array_equal(rf.fits[0].params, lone.params) and np.array_equal(rf.fits[0].error, lone.error)
    assert rf.seeds == list(range(11, 20)) and np.array_equal(rf.sigma[0], [0.0, 0.0]) and np.all(rf.sigma[1:] == spec["sigma"])
    again = nmrfit_amd.fit_replicas(data, spec["lower"], spec["upper"], replicas=8, sigma=spec["sigma"], seed=11, options=opts)
    assert np.array_equal(again.params, rf.params)
    c, t = C.case("end_to_end"), C.truth("end_to_end")
    assert data.u.tobytes() == c.u.tobytes() and spec["sigma"] == c.sigma_u and rf.seeds == c.seeds
    fine = nmrfit_amd.fit_replicas(data, spec["lower"], spec["upper"], replicas=8, sigma=spec["sigma"], seed=11,
                                   options=dict(opts, polish=True))
    assert np.all(fine.errors <= rf.errors) and np.array_equal(fine.iterations, rf.iterations)
    b = C.bar(c)
    pw = C.pointwise(t, fine.params[1:] - t.x0)
    want = np.std(t.lin, axis=0, ddof=1)
    af = np.array([C.area_fraction(t.x0 + d) for d in t.lin])
    af_tol = C.spread_tolerance(1.01 * b * np.sum(np.abs(t.af_grad) * t.sigma_x), c.M)
    print("end to end: polished, worst |D_k - D_lin,k| / sigma_x %.4f (bar %.4f); params_std / predicted: polished %s, "
          "swarm alone %s; area_fraction_std: polished %.4e, swarm alone %.4e, predicted %.4e"
          % (pw.max(), b, np.round(fine.params_std / want, 4), np.round(rf.params_std / want, 2), fine.area_fraction_std,
             rf.area_fraction_std, np.std(af, ddof=1)))
    assert np.all(pw <= b) and np.all(np.abs(fine.params[0] - t.x0) <= b * t.sigma_x)
    assert np.all(np.abs(fine.params_std - want) <= C.spread_tolerance(b, c.M) * t.sigma_x)
    assert abs(fine.area_fraction_std - np.std(af, ddof=1)) <= af_tol
    assert np.isfinite(rf.area_fraction_std) and rf.area_fraction_std > 0
    assert len({p.tobytes() for p in rf.params}) == 9                     # nine different fits
    assert data.u.tobytes() == u0.tobytes() and data.v.tobytes() == v0.tobytes()
    other = synth.make_spectrum(1500, 3, noise=1e-3, physical=True, seed=2)
    jobs = [dict(data=data, lower=spec["lower"], upper=spec["upper"], sigma=spec["sigma"]),
            dict(data=synth.SynthData(other["w"], other["u"], other["v"], other["peaks"]), lower=other["lower"],
                 upper=other["upper"], sigma=(other["sigma"], 2 * other["sigma"]))]
    many = nmrfit_amd.fit_replicas_many(jobs, replicas=8, seed=11, options=opts)
    assert len(many) == 2 and np.array_equal(many[0].params, rf.params)
    assert many[1].seeds == list(range(20, 29)) and many[1].params.shape == (9, 13)
    assert np.isfinite(many[1].area_fraction_std)

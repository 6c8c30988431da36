"""
GPU tier of the replica calibration (tests/calibration_support.py): what ``fit_replicas`` delivers -- noise made on the
device, swarms in a device batch, the polish, the spread -- against the linear response of every replica to its own
noise.  One ``FitBatch`` per problem: fit 0 the uploaded spectrum, fits 1 .. M its noisy copies.
"""
import time

import numpy as np
import pytest

import nmrfit_amd
from nmrfit_amd import lsq, noise
from nmrfit_amd.batch import FitBatch
from tests import calibration_support as C

pytestmark = pytest.mark.gpu

DEVICE_CASES = ("n512_p2", "n512_p2_unit", "n1024_p3_v2", "n1024_p3_unit")
POLISH_BUDGET = 200          # provider calls: far beyond what a fit takes (asserted: nobody stops on it)
_STUDIES = {}


def run_study(c, swarmsize=None, polish=True):
    """The study of case ``c`` on the device: noise in place, the swarms, then the polish.  ``swarmsize`` None: the
    library's default."""
    t = C.truth(c.name)
    K = c.M + 1
    su = np.concatenate(([0.0], np.full(c.M, c.sigma_u)))
    sv = np.concatenate(([0.0], np.full(c.M, c.sigma_v)))
    kw = {} if swarmsize is None else dict(swarmsize=swarmsize)
    out = dict(case=c, truth=t)
    t0 = time.perf_counter()
    with FitBatch([c.spectrum_tuple()] * K, [c.lower] * K, [c.upper] * K, seeds=c.seeds, **kw) as fb:
        fb.add_noise(su, sv, c.seeds)
        fb.run()
        out["status"] = fb.status()
        out["swarm"] = np.array([x for x, _ in fb.best()])
        out["swarm_f"] = np.array([f for _, f in fb.best()])
        if polish:
            got = fb.polish(max_launches=POLISH_BUDGET, ftol=C.FTOL)
            out["polished"] = np.array([x for x, _ in got])
            out["polished_f"] = np.array([f for _, f in got])
            out["info"] = fb.last_polish
            out["normal"] = fb.normal_equations([t.x0] * K)[0]
            out["final_normal"] = fb.normal_equations(list(out["polished"]))
            out["quality"] = fb.residual_stats(list(out["polished"]))
    out["seconds"] = time.perf_counter() - t0
    return out


def study(name):
    """(computed once per case, read-only: shared between the tests)"""
    if name not in _STUDIES:
        _STUDIES[name] = run_study(C.case(name))
    return _STUDIES[name]


def quantiles(a):
    return np.median(a), np.percentile(a, 95), np.max(a)


@pytest.mark.parametrize("name", DEVICE_CASES)
def test_polish_stops_on_ftol(name):
    """No fit stops on the budget (or frozen on a bound).  The noisy fits stop on ``ftol``, or -- a few -- on "lambda":
    their last accepted step still gained more than ``ftol`` and after it no trial point lowers f by a single bit, which
    is convergence too; so is fit 0's stop, whose f is 0 at its minimum (relative decreases never become small).  What
    the stopping distance in the bar assumes is then checked directly on EVERY noisy fit: the Gauss-Newton step left at
    the polished point, from the device's own normal equations there, is within sqrt(2 N ftol) sigma_x."""
    s = study(name)
    c, t, info = s["case"], s["truth"], s["info"]
    stops = {k: info["stop"][1:].count(k) for k in sorted(set(info["stop"][1:]))}
    left = np.array([np.abs(np.linalg.solve(A, g)) / t.sigma_x for A, g, _ in s["final_normal"][1:]])
    print("%s: %d launches, %.2f s for swarms + polish; stops of the noisy fits: %s, of fit 0: %s; worst step left "
          "%.2e sigma_x (stopping distance %.2e)" % (name, info["launches"], s["seconds"], stops, info["stop"][0], left.max(),
                                                     C.stopping_distance(c.N)))
    assert info["launches"] < POLISH_BUDGET
    assert all(st in ("ftol", "lambda") for st in info["stop"]), info["stop"]
    assert np.all(left <= C.stopping_distance(c.N))
    assert np.all(s["polished_f"] <= s["swarm_f"])


@pytest.mark.parametrize("name", DEVICE_CASES)
def test_pointwise(name):
    """Every D_k = x_k - x0 of the polished fits is within the bar of D_lin,k, per parameter; fit 0 is at x0."""
    s = study(name)
    c, t = s["case"], s["truth"]
    b = C.bar(c)
    delta = s["polished"] - t.x0
    pw = C.pointwise(t, delta[1:])
    print("%s: worst |D_k - D_lin,k| / sigma_x on the device %.4f (host TRF %.4f, bar %.4f); per parameter %s"
          % (name, pw.max(), C.REMAINDER_MEASURED[c.key], b, np.round(pw.max(axis=0), 4)))
    print("%s: fit 0: worst |x - x0| / sigma_x %.2e" % (name, np.max(np.abs(delta[0]) / t.sigma_x)))
    assert np.all(pw <= b), np.argwhere(pw > b)[:5]
    assert np.all(np.abs(delta[0]) / t.sigma_x <= b)
    # what a ReplicaFits reports of these fits: the spread of the noisy ones, ddof 1
    got, want = np.std(s["polished"][1:], axis=0, ddof=1), np.std(t.lin, axis=0, ddof=1)
    print("%s: spread of the polished fits / spread of the predictions: %s" % (name, np.round(got / want, 4)))
    assert np.all(np.abs(got - want) <= C.spread_tolerance(b, c.M) * t.sigma_x)


@pytest.mark.parametrize("name", DEVICE_CASES)
def test_area_fraction(name):
    """The area fraction of every polished fit against the function at the predicted point x0 + D_lin,k, through its
    gradient there: |af_k - af(x0 + D_lin,k)| <= 1.01 bar sum_i |grad_i| sigma_x,i (the 1 %: the gradient's change over
    the bar's distance, which is 1e-4 relative).  Their spread against the spread of the predictions."""
    s = study(name)
    c, t = s["case"], s["truth"]
    b = C.bar(c)
    got = np.array([C.area_fraction(x) for x in s["polished"][1:]])
    want = np.array([C.area_fraction(t.x0 + d) for d in t.lin])
    tol = np.array([1.01 * b * np.sum(np.abs(C.area_fraction_gradient(t.x0 + d)) * t.sigma_x) for d in t.lin])
    print("%s: area fraction: worst |af_k - prediction| / sigma_af %.4f (tolerance / sigma_af %.4f); spread %.6e "
          "predicted %.6e, sandwich %.6e" % (name, np.max(np.abs(got - want)) / t.af_sigma, tol.max() / t.af_sigma,
                                             np.std(got, ddof=1), np.std(want, ddof=1), t.af_sigma))
    assert np.all(np.abs(got - want) <= tol)
    # (first order: the function at the predicted point is the gradient at x0 applied to D_lin,k)
    lin = t.af0 + t.lin @ t.af_grad
    assert np.all(np.abs(want - lin) <= 0.01 * t.af_sigma)
    assert abs(np.std(got, ddof=1) - np.std(want, ddof=1)) <= C.spread_tolerance(tol.max(), c.M)


@pytest.mark.parametrize("name", ("n512_p2_unit", "n1024_p3_unit"))
def test_residual_sums(name):
    """Unit weights: ``residual_stats`` gives every replica's whole-grid sum of squares equal to
    RSS_k = N |dr_k + J D_lin,k|^2 within the measured remainder of the reference (twice, rounded up), and the mean of
    ``chi2_reduced(sigma, nparams=D)`` over the replicas lies inside the 1e-6 quantiles of chi^2 with M (N - D) degrees
    of freedom over M (N - D)."""
    s = study(name)
    c, t = s["case"], s["truth"]
    see = np.array([q.whole.rows[0, 2] for q in s["quality"]])
    want = t.rss(t.replicas)
    rel = np.abs(see[1:] - want) / want
    print("%s: worst |sum e^2 - RSS_k| / RSS_k %.3e (host TRF %.3e, bar %.3e)" % (name, rel.max(), C.RSS_REMAINDER_MEASURED, C.rss_bar()))
    assert np.all(rel <= C.rss_bar())
    assert see[0] <= 1e-20 * c.N                                                # (fit 0: the model fits the data)
    chi = np.array([q.chi2_reduced(c.sigma_u, nparams=c.D) for q in s["quality"][1:]])
    lo, hi = C.chi2_quantiles(c.M * (c.N - c.D))
    print("%s: mean chi2_reduced %.5f in (%.5f, %.5f)" % (name, chi.mean(), lo, hi))
    assert lo < chi.mean() < hi


@pytest.mark.parametrize("name", DEVICE_CASES)
def test_normal_equations(name):
    """``fb.normal_equations`` at x0 (fit 0: the unperturbed spectrum) against the host's central-difference J^T J.
    The device's column i is the forward difference of step h_i: J_i + (h_i / 2) d^2 r / dx_i^2 + O(h_i^2), and every
    residual value it differences carries a few roundings.  With E_i = |h_i| |S_i| (the truncation twice over: the
    O(h^2) term and the second difference's own error are far inside the factor 2) + 32 * 2^-53 max|weights (|V_data|
    + |V_fit|)| / |h_i| (sixteen roundings of the terms' size on either residual value, over all N points in norm), an
    entry of A may differ by E_i |J_j| + E_j |J_i| + E_i E_j.  sigma_x from the device's A, through the same sandwich,
    agrees to |A^-1| tol |A^-1| propagated."""
    s = study(name)
    c, t = s["case"], s["truth"]
    A, g, f = s["normal"]
    _, h = lsq.forward_rows(t.x0, c.lower, c.upper)
    S = C.second_differences(c, t.x0)
    size = float(np.max(c.weights * 2.0 * np.abs(c.u + 1j * c.v))) + float(np.max(np.abs(t.r0))) * np.sqrt(c.N)
    E = np.abs(h) * np.linalg.norm(S, axis=0) + 32.0 * 2.0 ** -53 * size / np.abs(h)
    nJ = np.linalg.norm(t.J, axis=0)
    tol = E[:, None] * nJ[None, :] + E[None, :] * nJ[:, None] + E[:, None] * E[None, :]
    err = np.abs(A - t.A)
    scale = np.sqrt(np.outer(np.diag(t.A), np.diag(t.A)))
    print("%s: worst |A - J^T J| / tolerance %.3f; worst |A - J^T J| / sqrt(A_ii A_jj) %.2e, tolerance / sqrt(A_ii A_jj) %.2e"
          % (name, np.max(err / tol), np.max(err / scale), np.max(tol / scale)))
    assert np.all(err <= tol)
    assert f <= 1e-12
    # sigma_x: cov = A^-1 (J^T diag(var) J) A^-1; the middle factor is the host's, A the device's
    mid = t.J.T @ (t.var[:, None] * t.J)
    Ai = np.linalg.inv(A)
    cov = Ai @ mid @ Ai
    dAi = np.abs(t.Ainv) @ tol @ np.abs(t.Ainv)                                # |d(A^-1)| <= |A^-1| |dA| |A^-1|, first order
    dcov = 2.1 * (dAi @ np.abs(mid) @ np.abs(t.Ainv))
    sx = np.sqrt(np.diag(cov))
    rel = np.abs(sx - t.sigma_x) / t.sigma_x
    bound = np.diag(dcov) / (2.0 * t.sigma_x ** 2) * 1.01
    print("%s: sigma_x from the device's A: worst relative difference %.2e (bound %.2e)" % (name, rel.max(), bound.max()))
    assert np.all(rel <= bound)


def swarm_alone(s):
    """|x_swarm,k - x_polished,k| / sigma_x of the noisy fits [M x D], and the inflation of the swarm's spreads over the
    linear predictions'."""
    c, t = s["case"], s["truth"]
    dist = np.abs(s["swarm"][1:] - s["polished"][1:]) / t.sigma_x
    std_infl = np.std(s["swarm"][1:], axis=0, ddof=1) / np.std(t.lin, axis=0, ddof=1)
    af = np.array([C.area_fraction(x) for x in s["swarm"][1:]])
    want = np.array([C.area_fraction(t.x0 + d) for d in t.lin])
    return dist, std_infl, np.std(af, ddof=1) / np.std(want, ddof=1)


def swarm_report(s, label):
    dist, infl, af = swarm_alone(s)
    stops = np.bincount([st["stop"] for st in s["status"]], minlength=3)
    its = [st["iteration"] for st in s["status"]]
    return ("%-28s |x_swarm - x_polished| / sigma_x: median %.3g, 95 %% %.3g, worst %.3g; params_std inflation "
            "median %.3g, worst %.3g; area_fraction_std inflation %.3g; stops (maxiter, minfunc, minstep) %s, "
            "generations median %d" % (label, *quantiles(dist), np.median(infl), infl.max(), af, stops.tolist(), np.median(its)))


@pytest.mark.parametrize("name", ("n512_p2", "n1024_p3_v2"))
def test_swarm_alone(name):
    """The same batch before ``polish``: how far pyswarm's rule stops from the replica's minimiser, in standard errors,
    and what that does to the spreads (printed: DESIGN.md section 4.11 carries the table).  Asserted: the polish moves
    every fit downhill from there, and the inflation is that of a positive independent term."""
    s = study(name)
    print(swarm_report(s, name + " default swarm:"))
    dist, infl, af = swarm_alone(s)
    assert np.all(np.isfinite(dist)) and np.all(s["polished_f"][1:] <= s["swarm_f"][1:])


# -- user level ------------------------------------------------------------------------------------------------------
USER_REPLICAS, USER_SEED = C.USER_REPLICAS, C.USER_SEED
USER_OPTS = {'polish': True}


def user_jobs():
    a, b = C.case("user_n512_p2"), C.case("user_n1024_p3_v2")
    return (a, b), [dict(data=a.data(), lower=a.lower, upper=a.upper, sigma=a.sigma_u),
                    dict(data=b.data(), lower=b.lower, upper=b.upper, sigma=(b.sigma_u, b.sigma_v))]


def check_user(rf, c):
    """``rf`` (a ReplicaFits made with the case's sigmas and seed0) against the case's predictions."""
    t = C.truth(c.name)
    lin, M, b = t.lin, c.M, C.bar(c)
    af = np.array([C.area_fraction(t.x0 + d) for d in lin])
    assert rf.seeds == c.seeds
    pw = C.pointwise(t, rf.params[1:] - t.x0, lin)
    want = np.std(lin, axis=0, ddof=1)
    print("%s: user level: worst pointwise %.4f (bar %.4f); params_std / prediction %s; area_fraction_std %.6e, "
          "prediction %.6e" % (c.name, pw.max(), b, np.round(rf.params_std / want, 4), rf.area_fraction_std, np.std(af, ddof=1)))
    assert np.all(pw <= b)
    assert np.all(np.abs(rf.params_std - want) <= C.spread_tolerance(b, M) * t.sigma_x)
    af_tol = 1.01 * b * np.sum(np.abs(t.af_grad) * t.sigma_x)
    assert abs(rf.area_fraction_std - np.std(af, ddof=1)) <= C.spread_tolerance(af_tol, M)


def test_user_level():
    """``fit_replicas_many`` with two jobs of different N (one with sigma_v = 2 sigma_u) and ``options['polish']``:
    ``params_std`` and ``area_fraction_std`` are the standard deviations of the linear predictions of the NOISY fits,
    within the bar's propagation; the seeds are ``seed + m (replicas + 1) + k``; ``fit_replicas`` gives job 0 the same."""
    (a, b), jobs = user_jobs()
    many = nmrfit_amd.fit_replicas_many(jobs, replicas=USER_REPLICAS, seed=USER_SEED, options=USER_OPTS)
    assert b.seeds[0] == USER_SEED + (USER_REPLICAS + 1)
    for c, rf in zip((a, b), many):
        check_user(rf, c)
    lone = nmrfit_amd.fit_replicas(jobs[0]["data"], a.lower, a.upper, replicas=USER_REPLICAS, sigma=a.sigma_u, seed=USER_SEED,
                                   options=USER_OPTS)
    assert np.array_equal(lone.params, many[0].params)


def test_user_level_without_polish_is_the_swarm():
    """Without ``options['polish']`` the call is what it was (the swarm's result), and polishing only moves downhill."""
    (a, _), jobs = user_jobs()
    plain = nmrfit_amd.fit_replicas_many(jobs[:1], replicas=4, seed=USER_SEED)[0]
    fine = nmrfit_amd.fit_replicas_many(jobs[:1], replicas=4, seed=USER_SEED, options=USER_OPTS)[0]
    assert np.all(fine.errors <= plain.errors) and np.array_equal(plain.iterations, fine.iterations)
    lone = nmrfit_amd.fit(jobs[0]["data"], a.lower, a.upper, summary=False, options={'seed': USER_SEED})
    assert np.array_equal(plain.fits[0].params, lone.params)


def test_user_level_fit_im_polish():
    """``fit_im`` replicas: the polish runs on both channels and f does not rise (the objective is a sum of norms: no
    linear prediction is claimed for it)."""
    (a, _), jobs = user_jobs()
    plain = nmrfit_amd.fit_replicas_many(jobs[:1], replicas=4, seed=5, fit_im=True, options={'swarmsize': 64})[0]
    fine = nmrfit_amd.fit_replicas_many(jobs[:1], replicas=4, seed=5, fit_im=True, options={'swarmsize': 64, 'polish': True})[0]
    assert np.all(fine.errors <= plain.errors) and np.any(fine.errors < plain.errors)


def test_device_sigma():
    """``device_sigma=True`` on a spectrum whose ``noise_region`` holds a quadratic plus device-made noise of known
    sigma: the sigma the study uses has sigma_hat^2 n / (n - 3) / sigma^2 inside the 1e-6 quantiles of
    chi^2_(n-3) / (n - 3), on each channel (sigma_v = 2 sigma_u)."""
    c = C.case("n512_p2")
    region = (3.30, 3.70)                                                      # between the two lines (3.1 and 3.9)
    sel = (c.w >= region[0]) & (c.w <= region[1])
    n = int(sel.sum())
    su, sv = 1e-3, 2e-3
    (zu, zv), = noise.replicas([np.zeros(c.N)], [np.zeros(c.N)], su, sv, [(1 << 40) + 3])
    x = c.w - 3.5
    u, v = c.u.copy(), c.v.copy()
    u[sel] = (0.01 + 0.2 * x - 0.5 * x * x + zu)[sel]
    v[sel] = (-0.02 + 0.1 * x + 0.3 * x * x + zv)[sel]
    data = nmrfit_amd.synth.SynthData(c.w, u, v, c.spec["peaks"])
    rf = nmrfit_amd.fit_replicas_many([dict(data=data, lower=c.lower, upper=c.upper)], replicas=1, seed=1, noise_region=region,
                                      device_sigma=True, options={'swarmsize': 16, 'maxiter': 3})[0]
    lo, hi = C.chi2_quantiles(n - 3)
    for got, s in zip(rf.sigma[1], (su, sv)):
        ratio = got * got * n / (n - 3) / (s * s)
        print("device_sigma: n = %d, sigma_hat^2 n / (n - 3) / sigma^2 = %.4f in (%.4f, %.4f)" % (n, ratio, lo, hi))
        assert lo < ratio < hi

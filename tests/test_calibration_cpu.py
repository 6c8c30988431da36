"""
CPU tier of the replica calibration (tests/calibration_support.py): the host truth alone.  scipy's TRF refits of every
replica stay within the bar of the linear prediction (and measure the bar), the seeds chosen give prediction spreads
inside their chi^2 quantiles, and every fault a replica study could carry unnoticed breaks the check.  Nothing here
touches a GPU, and of the package only ``synth`` and ``noise.normals`` / ``noise.replicas_host`` are used.
"""
import numpy as np
import pytest

from tests import calibration_support as C

NAMES = [c.name for c in C.cases()]
_REFITS = {}


def refits(name):
    """x_k - x0 of the TRF refits of every replica of the case (computed once, read-only)."""
    if name not in _REFITS:
        t = C.truth(name)
        d = t.refit(t.replicas)
        d.setflags(write=False)
        _REFITS[name] = d
    return _REFITS[name]


@pytest.mark.parametrize("name", NAMES)
def test_reference_within_bar(name):
    """The reference alone: |D_k - D_lin,k| / sigma_x of the TRF refits, per replica and parameter, within the bar --
    and within the measured constant the bar is made of, so that the bar is twice what is measured here."""
    c, t = C.case(name), C.truth(name)
    pw = C.pointwise(t, refits(name))
    print("%s: N %d, P %d, M %d, key %s: measured remainder %.5f (constant %.5f), bar %.5f (of it the stopping distance %.1e)"
          % (name, c.N, c.P, c.M, c.key, pw.max(), C.REMAINDER_MEASURED[c.key], C.bar(c), C.stopping_distance(c.N)))
    assert pw.max() <= C.REMAINDER_MEASURED[c.key] <= 0.5 * C.bar(c)
    # the base fit is inside its box by many standard errors: no bound takes part
    assert np.min(np.minimum(t.x0 - c.lower, c.upper - t.x0) / t.sigma_x) > 50.0
    sd, sl = np.std(refits(name), axis=0, ddof=1), np.std(t.lin, axis=0, ddof=1)
    print("%s: spread of the refits / spread of the predictions: %s" % (name, np.round(sd / sl, 4)))
    assert np.all(np.abs(sd - sl) <= C.spread_tolerance(C.bar(c), c.M) * t.sigma_x)


def test_constants_are_the_measured_ones():
    """Every measured constant is the worst of its cases, to the digits written down."""
    worst = {}
    for name in NAMES:
        c = C.case(name)
        worst[c.key] = max(worst.get(c.key, 0.0), float(C.pointwise(C.truth(name), refits(name)).max()))
    for key, value in worst.items():
        print("%s: measured %.6f, constant %.6f" % (key, value, C.REMAINDER_MEASURED[key]))
        assert 0.995 * C.REMAINDER_MEASURED[key] <= value <= C.REMAINDER_MEASURED[key]
    rel = 0.0
    for name in NAMES:
        c, t = C.case(name), C.truth(name)
        if c.unit:
            rss = np.array([c.N * np.sum(C.residual(c, t.x0 + d, u, v) ** 2) for d, (u, v) in zip(refits(name), t.replicas)])
            want = t.rss(t.replicas)
            rel = max(rel, float(np.max(np.abs(rss - want) / want)))
    print("residual sums: measured %.4e, constant %.4e, bar %.4e" % (rel, C.RSS_REMAINDER_MEASURED, C.rss_bar()))
    assert 0.995 * C.RSS_REMAINDER_MEASURED <= rel <= C.RSS_REMAINDER_MEASURED


@pytest.mark.parametrize("name", NAMES)
def test_seeds_give_ordinary_spreads(name):
    """A condition on the inputs: the spread of the linear predictions against the sandwich sigma_x lies inside the
    two-sided 1e-6 quantiles of chi^2_(M-1) / (M - 1) on every parameter, and the area fraction's too."""
    c, t = C.case(name), C.truth(name)
    ratio = np.var(t.lin, axis=0, ddof=1) / t.sigma_x ** 2
    af = np.var(t.lin @ t.af_grad, ddof=1) / t.af_sigma ** 2
    lo, hi = C.chi2_quantiles(c.M - 1)
    print("%s: var(D_lin) / sigma_x^2 in %.3f .. %.3f, area fraction %.3f; quantiles (%.3f, %.3f)" % (name, ratio.min(), ratio.max(), af, lo, hi))
    assert np.all((ratio > lo) & (ratio < hi)) and lo < af < hi


def test_area_fraction_is_the_library_s():
    """``area_fraction`` is what FitUtility.calculate_area_fraction computes, its gradient the central difference."""
    from nmrfit_amd.utils import FitUtility
    for name in ("n512_p2", "n1024_p3_v2"):
        c, t = C.case(name), C.truth(name)
        f = FitUtility(c.data(), c.lower, c.upper)
        f.params = t.x0 + t.lin[0]
        assert f.calculate_area_fraction() == C.area_fraction(f.params)
        g = np.zeros(c.D)
        for i in range(c.D):
            e = np.zeros(c.D)
            e[i] = 1e-6 * (c.upper[i] - c.lower[i])
            g[i] = (C.area_fraction(t.x0 + e) - C.area_fraction(t.x0 - e)) / (2.0 * e[i])
        assert np.allclose(g, t.af_grad, rtol=1e-6, atol=1e-9 * np.max(np.abs(t.af_grad)))


FAULT_CASES = [("variance", "n512_p2"), ("sqrt2", "n512_p2"), ("tied", "n512_p2"), ("one_seed", "n512_p2"),
               ("swapped", "n1024_p3_v2")]
FAULT_REPLICAS = 8      # (the first eight copies: a fault that shows on none of them is not caught by a short study either)


@pytest.mark.parametrize("fault,name", FAULT_CASES)
def test_fault_in_the_replica_maker_breaks_the_check(fault, name):
    """Each fault, injected into the host replica maker and refitted by TRF, leaves the pointwise check broken on at
    least one parameter -- printed: by how much."""
    c, t = C.case(name), C.truth(name)
    uv = C.make_replicas(c, fault)[:FAULT_REPLICAS]
    pw = C.pointwise(t, t.refit(uv), t.lin[:FAULT_REPLICAS])
    good = C.pointwise(t, refits(name)[:FAULT_REPLICAS], t.lin[:FAULT_REPLICAS])
    print("fault %-9s on %s: worst |D_k - D_lin,k| / sigma_x %.3f = %.1f bars (without the fault %.4f); parameters "
          "broken: %d of %d" % (fault, name, pw.max(), pw.max() / C.bar(c), good.max(), int(np.sum(pw.max(axis=0) > C.bar(c))), c.D))
    assert good.max() <= C.bar(c)
    assert pw.max() > C.bar(c)


@pytest.mark.parametrize("fault", ["fit0_counted", "ddof0"])
def test_fault_in_the_statistic_breaks_the_check(fault):
    """Fit 0 (the unperturbed data) counted among the draws, and ddof 0 for 1, change a standard deviation by about
    1 / (2 M): the short study at a tenth of the noise (M = 8, bar 0.0057) is where the spread check sees them."""
    name = "n512_p2_fine"
    c, t = C.case(name), C.truth(name)
    d = refits(name)
    tol = C.spread_tolerance(C.bar(c), c.M) * t.sigma_x
    want = np.std(t.lin, axis=0, ddof=1)
    good = np.abs(np.std(d, axis=0, ddof=1) - want)
    bad = np.abs((np.std(np.vstack((np.zeros(c.D), d)), axis=0, ddof=1) if fault == "fit0_counted" else np.std(d, axis=0, ddof=0)) - want)
    print("fault %-12s on %s: worst |spread - predicted| / tolerance %.2f (without the fault %.3f); parameters broken: %d of %d"
          % (fault, name, np.max(bad / tol), np.max(good / tol), int(np.sum(bad > tol)), c.D))
    assert np.all(good <= tol)
    assert np.any(bad > tol)

"""
CPU tier: the high-precision truth of tests/hp_truth.py, pinned to the reference's golden vectors and to scipy, the
one-hot probe that turns an objective into a pointwise readout, and the power of the bound -- perturbations of the size
a subtly wrong kernel would make are flagged, while plain float64 evaluations pass.  The Gaussian recurrence has a term
of its own in the bound: a float64 restatement of it leaves the plain bound and stays inside that one, subtly wrong
recurrences leave it too.  Last, the Python mirror of the kernel's two form predicates, on both sides of every clause.
"""
import math
import os

import numpy as np
import pytest
from scipy.special import dawsn

from nmrfit_amd import synth
from oracle import nmrfit_oracle as onp
from tests import hp_truth as hp


def test_truth_matches_edge_case_residual_rows(golden_dir):
    g = np.load(os.path.join(golden_dir, "objective_edge_cases.npz"))
    worst = 0.0
    for c in range(int(g["n_cases"])):
        w, u, v, wt, x, R = (g["e%d_%s" % (c, k)] for k in ("w", "u", "v", "wt", "x", "R"))
        scale = max(np.abs(R).max(), 1e-300)
        js = sorted(set(np.linspace(0, w.size - 1, min(w.size, 24)).astype(int)))
        for j in js:
            t = hp.point(x, w, u, v, j, imag=False)
            err = abs(wt[j] * t["dV"] - R[j]) / scale
            worst = max(worst, err)
            assert err <= 1e-13, (c, j, wt[j] * t["dV"], R[j])
    print("edge-case residual rows: worst |err|/scale %.3g" % worst)


def test_truth_matches_kramers_kronig_contributions(golden_dir):
    g = np.load(os.path.join(golden_dir, "kramers_kronig.npz"))
    x, w = g["x"], g["w"]
    sr, si = np.abs(g["real_contribs"]).max(), np.abs(g["imag_contribs"]).max()
    zeros = np.zeros_like(w)
    for j in range(0, w.size, 3):
        t = hp.point(x, w, zeros, zeros, j)
        np.testing.assert_allclose(t["real"], g["real_contribs"][:, j], rtol=0, atol=1e-13 * sr)
        np.testing.assert_allclose(t["imag"], g["imag_contribs"][:, j], rtol=0, atol=1e-8 * si)


def test_truth_dawson_against_scipy():
    """The truth's D(x) against scipy's dawsn for |x| from 1e-9 to 1e6 (both branches of the truth: erfi and, beyond
    100, the asymptotic series).  scipy itself is off by up to 4.4e-15 relative near |x| = 0.03, which the truth at 50
    digits confirms; the truth at its own 30 digits agrees with 50 to 1e-25."""
    xs = np.concatenate([10.0 ** np.linspace(-9, 6, 61), [0.25, 0.5, 7.0, 16.0, 16.0 + 2 ** -48, 100.0, 100.5]])
    worst = 0.0
    for x in np.concatenate([xs, -xs]):
        d = float(hp.dawson(x))
        worst = max(worst, abs(d - dawsn(x)) / abs(dawsn(x)))
        assert abs(d - dawsn(x)) <= 5e-15 * abs(dawsn(x)), (x, d, dawsn(x))
    print("truth vs dawsn: worst relative difference %.3g" % worst)
    for x in (1e-9, 0.031622776601683794, 3.0, 99.9, 100.1, 1e6):
        d30 = hp.dawson(x)
        with hp.mpmath.workdps(50):
            d50 = hp.dawson(x)
        assert abs(d30 - d50) <= 1e-25 * abs(d50), x


def _probe_case(N=700, P=5, seed=3):
    rng = np.random.default_rng(seed)
    w = np.linspace(-0.5, 1.5, N)
    u, v = rng.standard_normal(N), rng.standard_normal(N)
    x = np.concatenate([[0.7, -3.1, 0.37, 0.002], np.ravel([[0.01 + 0.05 * rng.random(), rng.uniform(-0.2, 1.2),
                                                           rng.uniform(0.5, 2.0)] for _ in range(P)])])
    return w, u, v, x


def test_one_hot_probe_identity_real_channel():
    """With weights one-hot at j, the objective is |R_j| / sqrt(N): the C oracle's two entry points agree to a few
    ulps."""
    from oracle import c_oracle
    w, u, v, x = _probe_case()
    N = w.size
    R = c_oracle.residual_batch(x, w, u, v, np.ones(N))[0]
    R = R[0] if R.ndim == 2 else R
    for j in (0, 1, 63, 64, 511, 512, N - 1):
        wt = np.zeros(N)
        wt[j] = 1.0
        f = c_oracle.objective_batch(x, w, u, v, wt)[0]
        assert abs(f - abs(R[j]) / math.sqrt(N)) <= 4 * np.finfo(float).eps * f, (j, f, R[j])


def test_one_hot_probe_identity_imaginary_modes():
    """fit_im True / "sum" with one-hot weights: the objective 0.5 (rms_real + rms_imag) is (|dV_j| + |dI_j|)/(2 sqrt N)
    (numpy oracle's real model + synth._dispersion), and the truth agrees with both parts."""
    w, u, v, x = _probe_case()
    N, P = w.size, (x.size - 4) // 3
    V, I = onp.ps2(u, v, x[0], x[1])
    Vf = sum(onp.voigt(w, x[2], x[3], *x[4 + 3 * k:7 + 3 * k]) for k in range(P))
    Ik = [synth._dispersion(w, x[2], *x[4 + 3 * k:7 + 3 * k]) for k in range(P)]
    for j in (0, 64, 333, N - 1):
        wt = np.zeros(N)
        wt[j] = 1.0
        t = hp.point(x, w, u, v, j)
        for mode, If in ((True, Ik[-1]), ("sum", sum(Ik))):
            f = 0.5 * (np.sqrt(np.mean((wt * (V - Vf)) ** 2)) + np.sqrt(np.mean((wt * (I - If)) ** 2)))
            probe = (abs(V[j] - Vf[j]) + abs(I[j] - If[j])) / (2 * math.sqrt(N))
            assert abs(f - probe) <= 4 * np.finfo(float).eps * f
            want, tol = hp.objective_probe(t, mode)
            assert abs(probe * 2 * math.sqrt(N) / 2 - want) <= tol + 1e-13 * want, (j, mode)


# ---- the bar has power ----------------------------------------------------------------------------------------------

def _flagged(got, t, key, tolkey):
    return abs(got - t[key]) > t[tolkey]


def test_plain_float64_passes_and_dropped_gaussian_is_flagged():
    N = 4096
    w = np.linspace(3.0, 4.0, N)
    u, v = np.zeros(N), np.zeros(N)
    j = 1000
    width = 0.004
    tg = math.sqrt(36.0)                          # 2^-t^2 = 2^-36 of the amplitude
    loc = w[j] - tg * width / 2
    x = np.array([0.0, 0.0, 0.0, 0.0, width, loc, 1.3])
    t = hp.point(x, w, u, v, j, imag=False)
    plain = float(onp.voigt(w[j:j + 1], 0.0, 0.0, width, loc, 1.3)[0])
    assert not _flagged(plain, t, "Vf", "tol_Vf")
    assert _flagged(0.0, t, "Vf", "tol_Vf")       # the Gaussian skipped


def test_phase_drift_is_flagged():
    N = 65536
    rng = np.random.default_rng(5)
    w = np.linspace(0.0, 1.0, N)
    u, v = rng.standard_normal(N), rng.standard_normal(N)
    p0, p1 = 0.3, 40.0
    j = hp.block_len(N) * 3 + 63 * 64 + 5          # far from its block's seed
    n = hp.rotation_steps(j, N)
    assert n == 63
    t = hp.point(np.array([p0, p1, 0.5, 0.0]), w, u, v, j, imag=False)
    phi = p0 + p1 * j / N
    plain = math.cos(phi) * u[j] - math.sin(phi) * v[j]
    assert not _flagged(plain, t, "V", "tol_V")
    phd = phi + 1e-12 * n
    assert _flagged(math.cos(phd) * u[j] - math.sin(phd) * v[j], t, "V", "tol_V")


def _lorentz_taylor(wj, lo, hi, width, loc, a, terms):
    """a L(w_j) from a Taylor series in u = (w - centre)/half around the chunk's centre (the far-field form)."""
    ihw = 2.0 / width
    tc = (0.5 * (lo + hi) - loc) * ihw
    hk = 0.5 * (hi - lo) * ihw
    uu = (wj - 0.5 * (lo + hi)) / (0.5 * (hi - lo))
    q = 1.0 / complex(tc, -1.0)                   # L = al Im(1/(t - i)) = al Im(q / (1 + hk u q))
    s = sum(q * (-hk * uu * q) ** n for n in range(terms))
    return a * ihw / math.pi * s.imag, math.sqrt(hk * hk / (1 + tc * tc))


def test_truncated_far_field_series_is_flagged():
    N = 4096
    w = np.linspace(3.0, 4.0, N)
    z = np.zeros(N)
    j = 2 * 512                                     # first point of a chunk
    lo, hi = w[j], w[j + 511]
    width = 0.5 * (hi - lo) / 2                     # hk = 4
    hk = 4.0
    tc = math.sqrt(hk * hk / 0.09 ** 2 - 1.0)       # rho = 0.09
    loc = 0.5 * (lo + hi) - tc * width / 2
    x = np.array([0.0, 0.0, 1.0, 0.0, width, loc, 1.0])
    t = hp.point(x, w, z, z, j, imag=False)
    full, rho = _lorentz_taylor(w[j], lo, hi, width, loc, 1.0, 16)
    assert abs(rho - 0.09) < 1e-9
    assert not _flagged(full, t, "Vf", "tol_Vf")
    short, _ = _lorentz_taylor(w[j], lo, hi, width, loc, 1.0, 10)
    assert _flagged(short, t, "Vf", "tol_Vf")


def test_scaled_needle_tail_is_flagged():
    N = 4096
    w = np.linspace(3.0, 4.0, N)
    z = np.zeros(N)
    j = 2000
    h = w[1] - w[0]
    width = 1e-3 * h
    for r in (1.0, 0.37):
        x = np.array([0.0, 0.0, r, 0.0, width, w[j] + 0.4 * h, 1.0])
        t = hp.point(x, w, z, z, j)
        re = float(synth._lineshape(w[j:j + 1], r, width, x[5], 1.0)[0])
        im = float(synth._dispersion(w[j:j + 1], r, width, x[5], 1.0)[0])
        assert not _flagged(re, t, "Vf", "tol_Vf") and not _flagged(im, t, "If2", "tol_If")
        assert _flagged(4 * re, t, "Vf", "tol_Vf")
        assert _flagged(4 * im, t, "If2", "tol_If")


def test_width_floor_is_the_floor_width_line():
    """Below the floor the truth is the line of the floor width; its dispersion tail a/(pi dw) does not depend on the
    width, so it agrees with the true-width closed form, while the old record's imaginary line (scaled by ihw/lim)
    is flagged."""
    N = 1024
    w = np.linspace(0.0, 1.0, N)
    z = np.zeros(N)
    w0, wspan = hp.grid_frame(w)
    j, loc, a = 100, 0.5, 1.0
    width = 1e-20
    assert hp.capped(width, loc, w0, wspan)
    x = np.array([0.0, 0.0, 1.0, 0.0, width, loc, a])
    t = hp.point(x, w, z, z, j)
    dw = w[j] - loc
    assert t["If2"] == pytest.approx(a / (math.pi * dw), rel=1e-12)
    lim = hp.T_CAP / (wspan + abs(loc - w0))
    old = float(synth._dispersion(w[j:j + 1], 1.0, 2.0 / lim, loc, a)[0]) * (2.0 / width) / lim
    assert _flagged(old, t, "If2", "tol_If")


# ---- the Gaussian recurrence: its own term of the bound ------------------------------------------------------------------

SQRT_LN2_OVER_PI = 0.46971863934982566689      # csrc/objective_math.h kSqrtLn2OverPi


def _rec_emulation(w, width, loc, a, c, lane, c_rel=0.0, skip_step=None, drop_d2=False):
    """csrc/objective_chunk.h gauss_add_rec restated line by line in float64 (numpy exp2: the best case) for one lane of
    the full chunk c of a uniform grid: the eight values AG 2^-t_q^2 at points c*512 + q*64 + lane, r = 0.  The
    keyword arguments make it subtly wrong: C off by c_rel, `ratio *= C` skipped at one step, d^2 dropped from the
    first ratio's exponent."""
    w0, wspan, lane_step, _ = hp.grid_analysis(w)
    assert lane_step != 0.0
    wc = w - w0
    ihw = 2.0 / width
    cc = -(loc - w0) * ihw
    ag2 = 2.0 * a * ihw * SQRT_LN2_OVER_PI
    d = lane_step * ihw
    C = float(np.exp2(-2.0 * d * d)) * (1.0 + c_rel)
    t0 = wc[c * hp.CHUNK + lane] * ihw + cc
    g = ag2 * float(np.exp2(-(t0 * t0 + 1.0)))
    ratio = float(np.exp2(-((t0 + t0) * d + (0.0 if drop_d2 else d * d))))
    out = [g]
    for q in range(1, hp.ROWS):
        g *= ratio
        out.append(g)
        if q + 1 < hp.ROWS and q != skip_step:
            ratio *= C
    return out


def _rec_cases():
    for N in (1101, 4096):
        for desc in (False, True):
            w = np.linspace(4.0, 3.0, N) if desc else np.linspace(3.0, 4.0, N)
            h = abs(w[1] - w[0])
            n_full = N // hp.CHUNK
            for c in sorted({0, n_full // 2, n_full - 1}):
                for steps in (64, 80, 128, 300, 1000):
                    for frac in (0.1, 0.37, 0.5, 0.93):
                        loc = float(w[c * hp.CHUNK]) + (w[1] - w[0]) * frac * hp.CHUNK
                        yield N, desc, w, c, steps * h, loc


def _rec_ratios(w, width, loc, c, lanes, rows=range(hp.ROWS), **mut):
    """(err / plain bound, err / bound with the recurrence term) at the given rows and lanes.  (r = 0, yoff = 0: the
    value is the Gaussian alone, so the second bound is the first plus C eps |G| rec_term -- one truth per point.)"""
    w0, _, lane_step, grid_dev = hp.grid_analysis(w)
    z = np.zeros(w.size)
    x = np.array([0.0, 0.0, 0.0, 0.0, width, loc, 1.3])
    ihw = 2.0 / width
    for lane in lanes:
        got = _rec_emulation(w, width, loc, 1.3, c, lane, **mut)
        w_row0 = float(w[c * hp.CHUNK + lane])
        t0 = (w_row0 - loc) * ihw
        dt0 = (abs(w_row0 - w0) + abs(loc - w0)) * abs(ihw) + abs(t0)
        for q in rows:
            j = c * hp.CHUNK + q * hp.WAVE + lane
            plain = hp.point(x, w, z, z, j, imag=False)
            new_tol = plain["tol_Vf"] + hp.C * hp.EPS * abs(plain["Vf"]) * hp.rec_term(q, t0, lane_step * ihw, dt0, ihw, grid_dev)
            err = abs(got[q] - plain["Vf"])
            yield q, lane, err / plain["tol_Vf"], err / new_tol


def test_default_bound_is_unchanged_by_the_recurrence_argument(golden_dir):
    """Without the argument every bound is bit for bit what hp_truth gave before it had a recurrence term
    (tests/golden/hp_truth_plain_bounds.npz: recorded from that version, same case, same points)."""
    w, u, v, x = _probe_case(N=1500)
    g = np.load(os.path.join(golden_dir, "hp_truth_plain_bounds.npz"))
    for i, j in enumerate(g["j"]):
        t = hp.point(x, w, u, v, int(j), chunk=(-0.3, 0.2))
        for k in g.files:
            if k != "j":
                np.testing.assert_array_equal(t[k], g[k][i], err_msg="%s at %d" % (k, j))
    for j in (0, int(np.argmin(np.abs(w - x[5]))), 1499):           # (the second: at a peak, where G is not ~0)
        a = hp.point(x, w, u, v, j)
        c = hp.point(x, w, u, v, j, rec=hp.grid_analysis(w)[2:])
        assert c["tol_V"] >= a["tol_V"] and c["tol_I2"] == a["tol_I2"] and c["Vf"] == a["Vf"]
        assert (c["tol_V"] > a["tol_V"]) == (0 < j < 1499)
        for k, plain in c["plain"].items():                           # (the plain bounds come along, bit for bit)
            np.testing.assert_array_equal(plain, a[k])
        assert hp.plain_bounds(c)["tol_V"] == a["tol_V"] and hp.plain_bounds(a) is a
    # one Gaussian alone: the bound with the term is the plain one plus C eps |G| rec_term (what _rec_ratios uses)
    w = np.linspace(3.0, 4.0, 4096)
    z = np.zeros(w.size)
    w0, _, lane_step, grid_dev = hp.grid_analysis(w)
    x1 = np.array([0.0, 0.0, 0.0, 0.0, 0.03, 3.4, 1.3])
    j, q = 1024 + 5 * 64 + 9, 5
    a, c = hp.point(x1, w, z, z, j, imag=False), hp.point(x1, w, z, z, j, imag=False, rec=(lane_step, grid_dev))
    ihw, w_row0 = 2.0 / 0.03, float(w[j - q * 64])
    t0 = (w_row0 - 3.4) * ihw
    add = hp.C * hp.EPS * abs(a["Vf"]) * hp.rec_term(q, t0, lane_step * ihw, (abs(w_row0 - w0) + abs(3.4 - w0)) * ihw + abs(t0),
                                                      ihw, grid_dev)
    assert c["tol_Vf"] == pytest.approx(a["tol_Vf"] + add, rel=1e-13) and add > a["tol_Vf"]


def test_recurrence_emulation_within_new_bound_and_breaks_the_plain_one():
    """The float64 restatement of the recurrence stays inside the bound with the recurrence term everywhere, and leaves
    the plain Gaussian bound somewhere (rows far from the lane's first point, |t_q| ~ 0): why the term exists."""
    worst_old, worst_new, where_old, where_new = 0.0, 0.0, None, None

    def scan(tag, ratios):
        nonlocal worst_old, worst_new, where_old, where_new
        for q, lane, r_old, r_new in ratios:
            if r_old > worst_old:
                worst_old, where_old = r_old, tag + (q, lane)
            if r_new > worst_new:
                worst_new, where_new = r_new, tag + (q, lane)
    for N, desc, w, c, width, loc in _rec_cases():
        scan((N, desc, c, width, loc), _rec_ratios(w, width, loc, c, (0, 21, 42, 63)))
    # where the plain bound is thinnest: row 7 of every lane, the centre inside that row, t0 ~ 11 half-widths away
    w = np.linspace(3.0, 4.0, 4096)
    h = w[1] - w[0]
    for c in (2, 3, 4):
        for frac in (0.9, 0.93, 0.96, 0.99):
            loc = float(w[c * hp.CHUNK]) + h * frac * hp.CHUNK
            scan((4096, False, c, 80 * h, loc), _rec_ratios(w, 80 * h, loc, c, range(hp.WAVE), rows=(7,)))
    print("recurrence emulation: worst err/tol %.3g against the plain bound at %s" % (worst_old, where_old))
    print("recurrence emulation: worst err/tol %.3g against the bound with the recurrence term at %s" % (worst_new, where_new))
    assert worst_new < 1.0, (worst_new, where_new)
    assert worst_old > 1.0, (worst_old, where_old)


def _mutant_case():
    N = 4096
    w = np.linspace(3.0, 4.0, N)
    h = w[1] - w[0]
    c = 3
    return w, 300 * h, float(w[c * hp.CHUNK]) + 0.93 * hp.CHUNK * h, c


@pytest.mark.parametrize("mut", [dict(c_rel=1e-12), dict(c_rel=-1e-12), dict(skip_step=3), dict(drop_d2=True)],
                         ids=["C_plus_1e-12", "C_minus_1e-12", "ratio_step_skipped", "d2_dropped"])
def test_subtly_wrong_recurrence_is_flagged(mut):
    """A relative error of 1e-12 in C = 2^(-2 d^2), one skipped `ratio *= C`, d^2 missing from the first ratio's
    exponent: each leaves the bound with the recurrence term, at a row where the correct recurrence is inside."""
    w, width, loc, c = _mutant_case()
    lanes = (0, 31, 63)
    good = max(r for *_, r in _rec_ratios(w, width, loc, c, lanes))
    bad = max(r for *_, r in _rec_ratios(w, width, loc, c, lanes, **mut))
    print("recurrence %s: worst err/tol %.3g (correct: %.3g)" % (mut, bad, good))
    assert good < 1.0
    assert bad > 1.0


# ---- the mirror of the kernel's two form predicates ---------------------------------------------------------------------

def _forms_grid(N=4096):
    w = np.linspace(3.0, 4.0, N)
    return w, w[1] - w[0]


def _particle(r, peaks):
    return np.concatenate([[0.1, 2.0, r, 1e-4], np.ravel(peaks)])


def test_grid_analysis_mirrors_the_context():
    w, h = _forms_grid(1024)
    w0, wspan, lane_step, grid_dev = hp.grid_analysis(w)
    assert (w0, wspan) == hp.grid_frame(w)
    assert lane_step == pytest.approx(64 * h, rel=1e-12) and 0.0 <= grid_dev <= 4 * np.finfo(float).eps * 4.0
    assert hp.grid_analysis(w[::-1].copy())[2] == pytest.approx(-64 * h, rel=1e-12)
    assert hp.grid_analysis(np.linspace(3.0, 4.0, 1023))[2:] == (0.0, 0.0)          # fewer than two chunks
    s = np.linspace(0.0, 1.0, 1101)
    assert hp.grid_analysis(3.0 + s + 0.35 * s * s)[2:] == (0.0, 0.0)               # not uniform
    bent = w.copy()
    bent[500] += 2e-6 * h                                                            # beyond 1e-6 of a step
    assert hp.grid_analysis(bent)[2] == 0.0
    bent[500] = w[500] + 0.5e-6 * h
    assert hp.grid_analysis(bent)[2] != 0.0 and hp.grid_analysis(bent)[3] >= 0.9e-6 * h


def test_kernel_forms_pair_form_clauses():
    w, h = _forms_grid()
    peaks = [[100 * h, 3.1 + 0.05 * k, 1.0] for k in range(17)]
    f = hp.kernel_forms(_particle(0.5, peaks), w)
    assert f["fast"] and f["sign_ok"] and f["fast_margin"] > 50
    flipped = [list(p) for p in peaks]
    flipped[16][2] = -1.0                                                            # a sign flip in the last group
    f = hp.kernel_forms(_particle(0.5, flipped), w)
    assert not f["fast"] and not f["sign_ok"] and f["fast_margin"] == -math.inf
    flipped[16][2], flipped[16][0] = 1.0, -100 * h                                   # ... by the width's sign
    assert not hp.kernel_forms(_particle(0.5, flipped), w)["fast"]
    assert not hp.kernel_forms(_particle(0.0, peaks), w)["fast"]                     # r = 0: al = 0
    assert not hp.kernel_forms(_particle(-0.2, peaks), w)["fast"]
    assert hp.kernel_forms(_particle(0.5, peaks[:0]), w)["fast"]                     # no peak: nothing refuses
    # the exponent budget, by eight needles of one aligned group and not by sign
    needle = [0.8e-5 * h, 3.5, 1.0]                                                  # 32 of the 250 each
    assert hp.kernel_forms(_particle(0.5, [needle]), w)["ehi"] == 32
    seven = [list(needle) for _ in range(7)] + peaks[:9]
    eight = [list(needle) for _ in range(8)] + peaks[:8]
    straddle = peaks[:4] + [list(needle) for _ in range(8)] + peaks[:4]              # four in each of two groups
    f7, f8, fs = (hp.kernel_forms(_particle(0.5, p), w) for p in (seven, eight, straddle))
    assert f8["sign_ok"] and not f8["fast"] and f8["fast_margin"] < 0 and f8["ehi"] >= hp.EXP_BUDGET
    assert f7["fast"] and f7["fast_margin"] > 0 and f8["ehi"] - 32 < f7["ehi"] < hp.EXP_BUDGET
    assert fs["fast"]
    # ... and from below: amplitudes so large that the sum of ilogb(1/al) leaves -250
    big = [[100 * h, 3.5, 1e9] for _ in range(8)]                                   # -34 each
    f = hp.kernel_forms(_particle(0.5, big), w)
    assert f["sign_ok"] and not f["fast"] and f["elo"] <= -hp.EXP_BUDGET
    big[0][2] = 1.0
    assert hp.kernel_forms(_particle(0.5, big), w)["fast"]
    assert not hp.kernel_forms(_particle(0.5, [[100 * h, 3.5, 1e305]]), w)["fast"]   # al >= 1e300
    f = hp.kernel_forms(_particle(1.0, [[100 * h, 3.5, 5e-324]]), w)                 # 0 < al, 1/al overflows
    assert f["sign_ok"] and f["edge"]
    assert not hp.kernel_forms(_particle(1.0, [[100 * h, 3.5, 1e-300]]), w)["edge"]


def test_kernel_forms_recurrence_clauses():
    w, h = _forms_grid()
    lane_step = hp.grid_analysis(w)[2]
    for r in (0.5, 0.0):                                                             # (independent of the pair form)
        under = hp.kernel_forms(_particle(r, [[300 * h, 3.5, 1.0], [lane_step * (1 + 1e-9), 3.2, 1.0]]), w)
        over = hp.kernel_forms(_particle(r, [[300 * h, 3.5, 1.0], [-lane_step * (1 - 1e-9), 3.2, 1.0]]), w)
        assert under["rec"] and 0 < under["rec_margin"] < 1e-8 and under["d"] < 2.0
        assert not over["rec"] and -1e-8 < over["rec_margin"] < 0 and over["d"] > 2.0
        assert under["fast"] == (r == 0.5)
    x = _particle(0.5, [[300 * h, 3.5, 1.0]])
    assert hp.kernel_forms(x, w)["rec"] and hp.kernel_forms(x, w[::-1].copy())["rec"]
    s = np.linspace(0.0, 1.0, w.size)
    f = hp.kernel_forms(x, 3.0 + s + 0.35 * s * s)                                   # a non-uniform grid
    assert not f["rec"] and f["rec_margin"] == -math.inf and f["fast"]
    assert not hp.kernel_forms(x, np.linspace(3.0, 4.0, 1023))["rec"]                # N = 1023 against 1024
    assert hp.kernel_forms(_particle(0.5, [[300.0 / 1023, 3.5, 1.0]]), np.linspace(3.0, 4.0, 1024))["rec"]
    # the grid's departure from the line: |it| grid_dev 11e10 <= 1
    bent = w.copy()
    bent[500] += 0.5e-6 * h
    dev = hp.grid_analysis(bent)[3]
    wide, narrow = 2.0 * dev * hp.REC_DEVK * 1.01, 2.0 * dev * hp.REC_DEVK * 0.99
    assert narrow > 64 * h                                                           # (|d| <= 2 holds for both)
    assert hp.kernel_forms(_particle(0.5, [[wide, 3.5, 1.0]]), bent)["rec"]
    assert not hp.kernel_forms(_particle(0.5, [[narrow, 3.5, 1.0]]), bent)["rec"]


# ---- residual rows: the float64 references inside the plain bound, planted errors outside ---------------------------------

def _reference_rows(X, w, u, v, wt):
    """{channel: rows} of the float64 references: the C oracle (real) and tests/lsq_im_support.py (imaginary, both modes)."""
    from oracle import c_oracle
    from tests import lsq_im_support as M
    return {"re": c_oracle.residual_batch(X, w, u, v, wt)[0], "im1": M.residual_rows(X, w, u, v, wt, 1)[1],
            "im2": M.residual_rows(X, w, u, v, wt, 2)[1]}


def _check_reference(worst, key, X, w, u, v, wt, j):
    from tests import rows_support as RS
    rows = _reference_rows(X, w, u, v, wt)
    for s, x in enumerate(X):
        t = RS.truth(key + (j, X.shape[1], s), x, w, u, v, j)
        for ch, R in rows.items():
            RS.check_point(worst[ch], R[s, j], t, ch, wt[j], (j, (X.shape[1] - 4) // 3, s))


def _report(worst):
    fails = []
    for wo in worst.values():
        fails += wo.report()
    return fails


@pytest.mark.parametrize("kind", ["uniform", "descending", "nonuniform", "unsorted"])
def test_float64_references_of_the_rows_at_the_switches_stay_inside_the_plain_bound(kind):
    """The cases of tests/test_gpu_rows_pointwise.py test_rows_at_the_switches, at the probes 0, 64, 511, 512 and N - 1,
    every peak count (65 and 130 at two of the probes), the P = 0 row, the same weights: what the bound asks of the
    device it grants a plain float64 evaluation with room to spare.  Worst err/tol measured over the four grids: real rows
    (C oracle) 0.0614 (nonuniform, point 64, P = 9, row 0; 0.037 on the other grids), imaginary rows (numpy, scipy's
    dawsn) 0.0102 in either mode (unsorted, point 0, the P = 0 row)."""
    from tests import rows_support as RS
    w, u, v = RS.make_grid(kind)
    N = w.size
    js = RS.switch_probes(N)
    wt, _ = RS.hostile_weights(N, js, seed=5)
    worst = {ch: hp.Worst("reference rows/%s/%s" % (kind, ch)) for ch in RS.CHANNELS}
    for n, j in enumerate(js):
        if j not in (0, 64, 511, 512, N - 1):
            continue
        for P, X in RS.switch_stacks(w, n, j).items():
            _check_reference(worst, (kind, N), X, w, u, v, wt, j)
        _check_reference(worst, (kind, N), RS.X_NO_PEAK, w, u, v, wt, j)
    fails = _report(worst)
    assert not fails, fails[:5]


@pytest.mark.parametrize("cls", ["pair_rec", "pair", "general_rec", "general", "budget_rec"])
def test_float64_references_of_class_rows_stay_inside_the_plain_bound(cls):
    """Every form class of tests/test_gpu_pointwise_forms.py on uniform1101: one probe in the full chunk, one in the
    ragged tail (the grid's last point), every peak count.  The *_rec classes included: a plain evaluation has no
    recurrence, and neither have the row kernels.  Worst err/tol measured over the five classes: real rows 0.0119,
    imaginary rows 0.0119 (both general_rec, point 512)."""
    from tests import rows_support as RS
    grid = "uniform1101"
    w, u, v = RS.class_grid(grid)
    N = w.size
    frame = hp.grid_analysis(w)
    chunks, large = RS.class_probes(N, cls)
    probes = [j for _, _, p in chunks for _, j in p]
    wt, _ = RS.hostile_weights(N, probes, seed=9)
    worst = {ch: hp.Worst("reference rows/%s/%s/%s" % (grid, cls, ch)) for ch in RS.CHANNELS}
    for kind, c, p in chunks:
        stacks = RS.class_stacks(w, c, cls, frame)
        j = [j for _, j in p if j in large][0]
        for P, X in stacks.items():
            _check_reference(worst, (grid, kind, cls), X, w, u, v, wt, j)
    fails = _report(worst)
    assert not fails, fails[:5]


def _ratio(got, t, ch, wj):
    from tests import rows_support as RS
    val, tol = RS.CHANNELS[ch]
    return abs(got - wj * t[val]) / (abs(wj) * t[tol])


def test_planted_errors_in_a_row_leave_the_bound():
    """The GPU test's comparison discriminates: a float64 row passes, the same row with one planted error does not.
        (a) one peak's Lorentzian amplitude off by a relative 1e-12, read at the peak's centre;
        (b) the Gaussian of a general-form particle (r = 0) dropped at a point just inside its window's edge
            (1 - 1e-6 of 3.97 widths), on data that is zero there -- with data of order one the value at the edge, 2^-63 of
            the amplitude, lies below the bound by design of the window; dropped at three widths it is flagged in noise;
        (c) the row shifted by one grid point (a store index off by one);
        (d) the weight's sign lost, read at the point whose weight is negative."""
    from tests import rows_support as RS
    from tests.test_gpu_pointwise import features
    w, u, v = RS.make_grid("uniform")
    N = w.size
    js = RS.switch_probes(N)
    wt, _ = RS.hostile_weights(N, js, seed=5)
    j = 64
    # (a) the t = 0 feature alone, with a Lorentzian part (the builder's row has r = 0)
    x = RS.particles(w, j)[1][0].copy()
    x[2] = 0.37
    assert x[5] == w[j]
    t = hp.point(x, w, u, v, j)
    row = _reference_rows(x[None, :], w, u, v, wt)["re"][0]
    AL = x[6] * x[2] * 2.0 / (math.pi * x[4])
    assert _ratio(row[j], t, "re", wt[j]) < 1.0
    assert _ratio(row[j] - wt[j] * AL * 1e-12, t, "re", wt[j]) > 1.0
    # (b) features 2 (the window's edge, inside by 1e-6) and 8 (three widths)
    feats = features(w, j)
    z = np.zeros(N)
    for k, uu, vv in ((2, z, z), (8, u, v)):
        width, loc, a, kind = feats[k]
        assert kind == "gauss"
        assert abs(abs(w[j] - loc) / width - ((1 - 1e-6) * 3.9686269665968861 if k == 2 else 3.0)) < 1e-9
        x = np.array([0.0, 0.0, 0.0, 0.0, width, loc, a])
        assert not hp.kernel_forms(x, w)["fast"]                        # r = 0: the general form
        t = hp.point(x, w, uu, vv, j)
        row = _reference_rows(x[None, :], w, uu, vv, wt)["re"][0]
        G = row[j] - wt[j] * t["V"]                                      # the model's part of the row: -weights G
        assert G != 0.0
        assert _ratio(row[j], t, "re", wt[j]) < 1.0
        assert _ratio(row[j] - G, t, "re", wt[j]) > 1.0, k
    # (c), (d) a stack of the sweep, all three channels
    X = RS.particles(w, j)[9]
    rows = _reference_rows(X, w, u, v, wt)
    neg = [q for q in js if wt[q] < 0]
    assert len(neg) == 1
    Xn = RS.particles(w, neg[0])[9]
    rows_n = _reference_rows(Xn, w, u, v, wt)
    for ch in RS.CHANNELS:
        for s, x in enumerate(X):
            t = RS.truth(("uniform", N, j, X.shape[1], s), x, w, u, v, j)
            assert _ratio(rows[ch][s, j], t, ch, wt[j]) < 1.0
            for shift in (1, -1):
                assert _ratio(np.roll(rows[ch][s], shift)[j], t, ch, wt[j]) > 1.0, (ch, s, shift)
        for s, x in enumerate(Xn):
            t = hp.point(x, w, u, v, neg[0])
            assert _ratio(rows_n[ch][s, neg[0]], t, ch, wt[neg[0]]) < 1.0
            assert _ratio(-rows_n[ch][s, neg[0]], t, ch, wt[neg[0]]) > 1.0, (ch, s)

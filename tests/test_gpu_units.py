"""
GPU tier: every kernel held to its values in other units than the suite's own (an axis on [3, 4.35], intensities of
order 1).  tests/units_support.py states the law and the systems; tests/test_units_cpu.py shows that every reference
used here keeps the law by itself.

    exact        a change of units by powers of two (E1 = (2^7, 1), E2 = (2^14, 4^14), E3 = (2^-10, 4^-12), the descending
                 twin (-2^7, 1)) commutes with every operation of the chain, so the device's outputs in both systems are
                 compared BIT FOR BIT: the objective and the residual rows of every kernel variant, imaginary mode and
                 launch form, the weights, the swarms, the device batch (four fits in four systems side by side), the
                 reconstruction, the residual statistics, the noise, the weights' build and the normal equations.
                 Every exact case asserts its preconditions on its own inputs first: the same form flags
                 (hp_truth.kernel_forms) in both systems and no value outside [2^-900, 2^900].
    by truth     where the system flips a form flag (E3 takes the pair form from amplitudes of order 1: c = 4^-12 raises
                 the sum of eight exponents by 192) and in the physical systems P1 (ppm, descending from 185, x 3.7e8), P2
                 (Hz at 2.5e4 to 4.9e4, x 2.1e6), P3 (1e-3 (3 + s), x 1e-7): check_objective and check_recon of
                 tests/test_gpu_pointwise.py, unchanged, with hp_truth's own bound.

A swarm is not compared across the descending twin: a box swaps its ends under a negative column scale and
lb + rand (ub - lb) is not symmetric under the swap (tests/test_units_cpu.py shows it on the host mirror).  The batch's
descending fit is held to its own lone run, and to the law through what is evaluated at given positions.

Phase correction and peak picking are NOT covariant, by the reference's own constants: ACME adds 1000 x a penalty that is
quadratic in the intensities to an entropy that is free of them; peakutils' baseline iterates from a coefficient of 1.0
to a relative tolerance and thresholds are absolute.  For these the existing host comparisons are re-run on spectra
x 3.7e8 and x 2^-30 instead.

FARFIELD32 is held to the law inside its documented domain (fp32's: E1, the descending twin and F7 = (2^7, 4^7)); it
keeps it exactly there, no flush threshold was met.

Every case prints ``units:`` lines (recorded in profiles/r15/units.txt).
"""
import math

import numpy as np
import pytest

from nmrfit_amd import _cabi, lsq, noise, quality, synth, utils
from nmrfit_amd.equations import Evaluator
from tests import hp_truth as hp
from tests import units_support as us
from tests.test_gpu_pair_waves import _env
from tests.test_gpu_pointwise import (MODES, check_objective, check_recon, chunk_of, make_grid, particles,
                                      recon_x, sample_points)

pytestmark = pytest.mark.gpu

F7 = us.Exact("F7", 2.0 ** 7, 4.0 ** 7)                # the far end of FARFIELD32's documented domain
LAW = {s.name: s for s in (us.E1, us.E2, us.DESC, F7)}
PROBES = (64, 2048 + 511, 4172)                        # a first row, a last row of a full chunk, the ragged tail's end


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    assert _cabi.device_count() >= 1


def wide_lines(w, P, n, seed):
    """n particles of P lines 90 to 300 grid steps wide with small positive areas and 0 < r < 1: the pair form, and on a
    uniform grid the Gaussian recurrence; the exponent sums stay inside the budget under c = 4^14 as well."""
    rng = np.random.default_rng(seed)
    span = float(w.max() - w.min())
    h = span / (w.size - 1)
    X = np.empty((n, 4 + 3 * P))
    X[:, 0] = rng.uniform(-1.0, 1.0, n)
    X[:, 1] = rng.uniform(-30.0, 30.0, n)
    X[:, 2] = rng.uniform(0.2, 0.9, n)
    X[:, 3] = rng.uniform(-1e-3, 1e-3, n)
    X[:, 4::3] = h * np.exp(rng.uniform(math.log(90.0), math.log(300.0), (n, P)))
    X[:, 5::3] = rng.uniform(w.min(), w.max(), (n, P))
    X[:, 6::3] = rng.uniform(0.003, 0.01, (n, P))
    return X


def stacks(w):
    """{name: X}: the particles of test_gpu_pointwise at three probes, and wide lines."""
    out = {}
    for j in PROBES:
        for P, X in particles(w, j, with_large=False).items():
            out["probe%d/P%d" % (j, P)] = X
    for P in (3, 9, 17):
        out["wide/P%d" % P] = wide_lines(w, P, 6, seed=P)
    return out


def tile(X, S):
    return np.ascontiguousarray(np.tile(X, (-(-S // len(X)), 1))[:S])


def modes_of(ev, var, X):
    """The imaginary modes the variant has (FARFIELD32: the real channel alone)."""
    ev.set_variant(var)
    out = []
    for mode in MODES:
        try:
            ev.objective_batch(X[:1], fit_im=mode)
            out.append(mode)
        except _cabi.NmrfitError as e:
            if "error %d" % _cabi.E_UNSUPPORTED not in str(e):
                raise
    return out


def variants_for(sys_):
    """FARFIELD32 inside its documented domain: fp32's, i.e. not under c = 4^14."""
    return [v for v in _cabi.available_variants() if v != _cabi.VARIANT_FARFIELD32 or sys_.c <= F7.c]


def preconditions(sys_, w, u, v, X, w2, u2, v2, X2):
    """The rows of X whose form flags agree in both systems (every value in range is asserted); the flags."""
    assert us.in_range(w, u, v, X) and us.in_range(w2, u2, v2, X2)
    return us.same_forms(X, w, X2, w2)


# ---- the objective and the rows ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(LAW))
@pytest.mark.parametrize("kind", ["uniform", "nonuniform"])
def test_objective_and_rows_keep_the_law(kind, name):
    """f' == c f and R' == c R, bit for bit, for every particle whose form flags agree in both systems.  A particle whose
    flag flips (E2 and F7 take the pair form from some of the probes' 8- and 9-peak particles: amplitudes of order 1
    times c leave the exponent budget) is NOT compared by bits: it is held, in the other system, to the truth at its
    probe (check_objective of tests/test_gpu_pointwise.py); in the suite's units that file holds it already."""
    sys_ = LAW[name]
    w, u, v = make_grid(kind)
    N = w.size
    wt = np.random.default_rng(5).uniform(0.5, 2.0, N)
    wt[[7, 600, 4000]] = 0.0
    w2, u2, v2 = sys_.spectrum(w, u, v)
    tally = us.Tally("objective+rows/%s/%s" % (kind, name), system=sys_)
    worst = hp.Worst("objective+rows/%s/%s: flipped particles by truth" % (kind, name))
    nfast = nrec = nflip = 0
    flipped = []
    with Evaluator(w, u, v, wt) as a, Evaluator(w2, u2, v2, wt) as b:
        for tag, X in stacks(w).items():
            X2 = sys_.params(X)
            same, f1, _ = preconditions(sys_, w, u, v, X, w2, u2, v2, X2)
            if tag.startswith("wide"):
                assert same.all() and all(f for f, _ in f1) and all(r for _, r in f1) == (kind == "uniform"), (tag, f1)
            else:
                assert same.any(), tag
            if not same.all():
                flipped.append((int(tag[5:tag.index("/")]), X2[~same]))
                nflip += int((~same).sum())
            X, X2 = X[same], X2[same]
            nfast += sum(f for (f, _), k in zip(f1, same) if k)
            nrec += sum(r for (_, r), k in zip(f1, same) if k)
            for var in variants_for(sys_):
                for mode in modes_of(a, var, X):
                    b.set_variant(var)
                    tally.equal(b.objective_batch(X2, fit_im=mode), sys_.c * a.objective_batch(X, fit_im=mode),
                                (tag, var, mode))
                Ra, fa = a.residual_batch(X, return_f=True)
                Rb, fb = b.residual_batch(X2, return_f=True)
                tally.equal(Rb, sys_.c * Ra, (tag, var, "rows"))
                tally.equal(fb, sys_.c * fa, (tag, var, "rows f"))
            a.set_variant(_cabi.VARIANT_DEFAULT)
            b.set_variant(_cabi.VARIANT_DEFAULT)
            for mode in (True, "sum"):
                for got, want in zip(b.residual_batch_im(X2, mode), a.residual_batch_im(X, mode)):
                    tally.equal(got, sys_.c * want, (tag, "rows_im", mode))
        wc, _ = hp.grid_frame(w2)
        for j, X2 in flipped:
            one = np.zeros(N)
            one[j] = 1.0
            b.set_weights(one)
            lo, hi = chunk_of(w2, j)
            check_objective(b, X2, w2, u2, v2, j, worst, (lo - wc, hi - wc))
    tally.fields.update(pair_form=nfast, recurrence=nrec, flipped_held_by_truth=nflip,
                        flipped_worst_err_over_bound="%.3g" % worst.ratio)
    bad = tally.done() + worst.report()
    assert not bad, bad[:5]


LAUNCHES = (("eight segments", 204, None, None, 8), ("four segments", 516, None, None, 4),
            ("four segments, pair form", 516, 1, None, 4), ("a wave per particle", 300, None, 1, 1))


@pytest.mark.parametrize("name", ["E1", "E2", "DESC"])
def test_objective_law_in_every_launch_form(name):
    """N = 4096: eight blocks of one chunk, so that a swarm of 204 takes the eight-wave workgroup, one of 516 four
    segments (with NMRFIT_PAIR_WAVES=1 the pair form: two particles per workgroup) and NMRFIT_TARGET_WAVES=1 a wave per
    particle; the knobs are read when the context is made."""
    sys_ = LAW[name]
    w, u, v = make_grid("uniform", N=4096)
    wt = np.random.default_rng(6).uniform(0.5, 2.0, w.size)
    w2, u2, v2 = sys_.spectrum(w, u, v)
    general = wide_lines(w, 9, 8, seed=2)
    general[:, 6 + 3 * np.arange(8)] *= -1.0              # one negative area each: the general form, in every system
    pool = np.concatenate([wide_lines(w, 9, 40, seed=1), general])
    tally = us.Tally("launch forms/%s" % name, system=sys_)
    seen = []
    for what, S, pair, target, segments in LAUNCHES:
        X = tile(pool, S)
        X2 = sys_.params(X)
        same, f1, _ = preconditions(sys_, w, u, v, X, w2, u2, v2, X2)
        assert same.all() and any(f for f, _ in f1) and not all(f for f, _ in f1)      # (pairs of both forms)
        with _env(NMRFIT_PAIR_WAVES=pair, NMRFIT_TARGET_WAVES=target):
            a, b = Evaluator(w, u, v, wt), Evaluator(w2, u2, v2, wt)
        with a, b:
            for var in variants_for(sys_):
                for mode in modes_of(a, var, X):
                    b.set_variant(var)
                    fa = a.objective_batch(X, fit_im=mode)
                    ll = a.last_launch()
                    if mode is False and var == _cabi.VARIANT_DEFAULT:
                        assert ll["segments"] == segments, (what, ll)
                        seen.append((what, ll["segments"], ll["waves_per_workgroup"], ll["waves"]))
                    tally.equal(b.objective_batch(X2, fit_im=mode), sys_.c * fa, (what, var, mode))
    tally.fields.update(launches=seen)
    bad = tally.done()
    assert not bad, bad[:5]


def test_weights_times_a_power_of_two():
    w, u, v = make_grid("uniform")
    wt = np.random.default_rng(7).uniform(0.5, 2.0, w.size)
    X = np.concatenate([wide_lines(w, 9, 6, seed=2), particles(w, 64, with_large=False)[9]])
    tally = us.Tally("weights 2^k", k=(-20, 7, 40))
    with Evaluator(w, u, v, wt) as ev:
        for var in _cabi.available_variants():
            for mode in modes_of(ev, var, X):
                ev.set_weights(wt)
                f = ev.objective_batch(X, fit_im=mode)
                R = ev.residual_batch(X)
                for k in (-20, 7, 40):
                    ev.set_weights(wt * 2.0 ** k)
                    tally.equal(ev.objective_batch(X, fit_im=mode), f * 2.0 ** k, (var, mode, k))
                    tally.equal(ev.residual_batch(X), R * 2.0 ** k, (var, "rows", k))
    bad = tally.done()
    assert not bad, bad[:5]


# ---- truth in physical units, and where a form flips -------------------------------------------------------------------

def truth_probes(N):
    return (0, 63, 512, 2048 + 448 + 31, N - N % hp.CHUNK, N - 1)


@pytest.mark.parametrize("name", [s.name for s in us.PHYSICAL])
@pytest.mark.parametrize("kind", ["uniform", "nonuniform"])
def test_objective_truth_in_physical_units(kind, name):
    """check_objective of tests/test_gpu_pointwise.py, unchanged, on a grid and data in physical units: the particles are
    built on that grid (peaks at the kernels' switches around the probe), their amplitudes scaled like the data."""
    sys_ = {s.name: s for s in us.PHYSICAL}[name]
    w0_, u0_, v0_ = make_grid(kind)
    w, u, v = sys_.spectrum(w0_, u0_, v0_)
    N = w.size
    worst = hp.Worst("objective truth %s/%s" % (kind, name))
    n = 0
    with Evaluator(w, u, v, np.ones(N)) as ev:
        for j in truth_probes(N):
            wt = np.zeros(N)
            wt[j] = 1.0
            ev.set_weights(wt)
            wc, _ = hp.grid_frame(w)
            lo, hi = chunk_of(w, j)
            for P, X in particles(w, j, with_large=False).items():
                X = sys_.amplitudes(X)
                assert us.in_range(w, u, v, X)
                check_objective(ev, X, w, u, v, j, worst, (lo - wc, hi - wc))
                n += X.shape[0] * P
    fails = worst.report()
    us.record("objective truth/%s/%s" % (kind, name), system=sys_, peak_points=n, worst_err_over_bound="%.3g" % worst.ratio)
    assert not fails, fails[:5]


def test_objective_truth_where_e3_flips_the_form():
    """Wide lines with areas of order 1e-2 take the pair form in the suite's units and the general form under E3: the two
    systems are not compared by bits but each with the truth (the recurrence's term where the probe's chunk is full)."""
    w, u, v = make_grid("uniform")
    N = w.size
    X = wide_lines(w, 9, 3, seed=29)
    w2, u2, v2 = us.E3.spectrum(w, u, v)
    X2 = us.E3.params(X)
    same, f1, f2 = preconditions(us.E3, w, u, v, X, w2, u2, v2, X2)
    assert not same.any() and all(f for f, _ in f1) and not any(f for f, _ in f2) and all(r for _, r in f1 + f2)
    worst = {}
    for tag, (gw, gu, gv, gX) in (("suite units", (w, u, v, X)), ("E3", (w2, u2, v2, X2))):
        worst[tag] = hp.Worst("E3 flip: %s" % tag)
        _, _, lane_step, grid_dev = hp.grid_analysis(gw)
        with Evaluator(gw, gu, gv, np.ones(N)) as ev:
            for j in truth_probes(N):
                wt = np.zeros(N)
                wt[j] = 1.0
                ev.set_weights(wt)
                wc, _ = hp.grid_frame(gw)
                lo, hi = chunk_of(gw, j)
                full = (j // hp.CHUNK + 1) * hp.CHUNK <= N
                rec = (lane_step, grid_dev, np.ones(len(gX), dtype=bool)) if full else None
                check_objective(ev, gX, gw, gu, gv, j, worst[tag], (lo - wc, hi - wc), rec=rec)
    fails = [f for t in worst.values() for f in t.report()]
    us.record("objective truth/E3 flip", forms="%s -> %s" % (f1[0], f2[0]),
              worst_err_over_bound="%.3g / %.3g" % (worst["suite units"].ratio, worst["E3"].ratio))
    assert not fails, fails[:5]


@pytest.mark.parametrize("name", [s.name for s in us.PHYSICAL] + ["E3"])
def test_reconstruction_truth_in_other_units(name):
    """check_recon of tests/test_gpu_pointwise.py, unchanged, on the fit's own and on a foreign output grid."""
    sys_ = dict({s.name: s for s in us.PHYSICAL}, E3=us.E3)[name]
    w, u, v = sys_.spectrum(*make_grid("uniform", N=1500))
    N = w.size
    w0, wspan = hp.grid_frame(w)
    worst = hp.Worst("reconstruction truth %s" % name)
    n = 0
    with Evaluator(w, u, v, np.ones(N)) as ev:
        for P in (0, 9, 257):
            x = recon_x(w, P, seed=P + 3)
            x = sys_.amplitudes(x)          # (built on this system's grid: the axis is in place, the intensities are not)
            m = min(60, max(8, 3000 // max(P, 1)))
            wout = np.linspace(w.min(), w.max(), int(1.5 * N))
            for grid in (None, wout):
                g = w if grid is None else grid
                real, imag, fit, data = ev.generate_result(x, grid)
                r2, i2 = ev.contributions(x, grid)
                np.testing.assert_array_equal(real, r2)
                np.testing.assert_array_equal(imag, i2)
                js = sample_points(g.size, m, seed=P)
                check_recon(worst, (P, grid is None), x, w, u, v, g, real, imag, fit, data, js,
                            sample_points(N, 20, seed=P + 1), w0, wspan)
                n += len(js) * max(P, 1)
    fails = worst.report()
    us.record("reconstruction truth/%s" % name, system=sys_, peak_points=n, worst_err_over_bound="%.3g" % worst.ratio)
    assert not fails, fails[:5]


# ---- the swarm -----------------------------------------------------------------------------------------------------------

def swarm_run(sp, sys_, S, variant, minfunc, gens=8):
    """The whole state after ``gens`` generations in the system sys_."""
    from nmrfit_amd.pso import DeviceSwarm
    w, u, v, wt = sys_.spectrum(sp["w"], sp["u"], sp["v"], sp["weights"])
    lo, up = sys_.box(sp["lower"], sp["upper"])
    with Evaluator(w, u, v, wt) as ev:
        ev.set_variant(variant)
        sw = DeviceSwarm(ev, lo, up, swarmsize=S, seed=5, minstep=-1.0, minfunc=minfunc * sys_.c)
        sw.run(maxiter=gens, check_every=1)
        out = dict(sw.state(), best=sw.best(), status=sw.status(), launches=sw.last_launches())
        sw.close()
    return out


@pytest.mark.parametrize("minfunc", [2.0 ** -8, -1.0], ids=["stops", "runs"])
@pytest.mark.parametrize("S, N", [(64, 4096), (516, 4173)])
def test_swarm_keeps_the_law(S, N, minfunc):
    """Eight generations -- S = 64 on 4096 points: eight-wave workgroups, one launch a generation, the fold deferred;
    S = 516 on 4173 points (nine blocks): per-block sums and the select kernel -- with minstep = -1 (the step norm mixes
    units: pyswarm's own rule) and minfunc scaled by c; armed, it stops the swarm before the eighth generation (the
    host mirror of tests/swarm_support.py does)."""
    sp = synth.make_spectrum(N, 9, seed=3, physical=True)
    for var in (_cabi.VARIANT_DEFAULT, _cabi.VARIANT_FARFIELD):
        a = swarm_run(sp, us.IDENTITY, S, var, minfunc)
        assert (a["status"]["stop"] == 1 and a["status"]["iteration"] < 8) == (minfunc > 0), a["status"]
        assert (a["launches"] == 1) == (S == 64), a["launches"]
        for sys_ in (us.E1, us.E2):
            tally = us.Tally("swarm/S%d/%s/variant %d/%s" % (S, "stops" if minfunc > 0 else "runs", var, sys_.name),
                             system=sys_, stop=a["status"]["stop"], generation=a["status"]["iteration"],
                             launches=a["launches"])
            w2, u2, v2 = sys_.spectrum(sp["w"], sp["u"], sp["v"])
            same, f1, _ = preconditions(sys_, sp["w"], sp["u"], sp["v"], a["x"], w2, u2, v2, sys_.params(a["x"]))
            assert same.all()
            tally.fields.update(pair_form="%d of %d" % (sum(f for f, _ in f1), len(f1)))
            b = swarm_run(sp, sys_, S, var, minfunc)
            for key in ("x", "v", "p"):
                tally.equal(sys_.un_params(b[key]), a[key], key)
            for key in ("fx", "fp"):
                tally.equal(sys_.un_inten(b[key]), a[key], key)
            tally.equal(sys_.un_params(b["best"][0]), a["best"][0], "best x")
            tally.equal(b["best"][1] / sys_.c, a["best"][1], "best f")
            tally.equal([b["status"]["stop"], b["status"]["iteration"], b["status"]["fg"] / sys_.c],
                        [a["status"]["stop"], a["status"]["iteration"], a["status"]["fg"]], "status")
            bad = tally.done()
            assert not bad, bad[:5]


# ---- the device batch ----------------------------------------------------------------------------------------------------

BATCH_SYSTEMS = (us.IDENTITY, us.E1, us.E2, us.DESC)
SIGMA = (0.004, 0.002)


def batch_fits(ragged):
    """Four base fits of ragged (or equal) lengths and of different peak counts, in the suite's units, with their
    regions and noise seeds."""
    out = []
    for k, (N, P) in enumerate(((1500, 3), (2113, 6), (2726, 2), (3339, 5))):
        N = N if ragged else 1900              # (four blocks, the last ragged: what the workgroup geometry takes)
        sp = synth.make_spectrum(N, P, seed=30 + k, physical=True)
        sp["regions"] = [(float(l - 2 * d), float(l + 2 * d)) for l, d in zip(sp["x_true"][5::3], sp["x_true"][4::3])][:2]
        sp["noise_seed"] = 900 + k
        out.append(sp)
    return out


def lone_fit(sp, sys_, mode, gens=8):
    """The fit alone, in the system sys_: the noise replica (noise.replicas), a DeviceSwarm on it, the reconstruction
    and the residual statistics at its best position."""
    from nmrfit_amd.pso import DeviceSwarm
    w, u, v, wt = sys_.spectrum(sp["w"], sp["u"], sp["v"], sp["weights"])
    lo, up = sys_.box(sp["lower"], sp["upper"])
    (un, vn), = noise.replicas([u], [v], sys_.sigma(SIGMA[0]), sys_.sigma(SIGMA[1]), [sp["noise_seed"]])
    with Evaluator(w, un, vn, wt) as ev:
        ev.set_fit_im(mode)
        sw = DeviceSwarm(ev, lo, up, swarmsize=96, seed=sp["noise_seed"] + 1, minstep=-1.0, minfunc=-1.0)
        sw.run(maxiter=gens, check_every=4)
        out = dict(sw.state(), best=sw.best(), spectrum=(un, vn))
        sw.close()
        real, imag, fit, data = ev.generate_result(out["best"][0])
    out["generate"] = dict(real=real, imag=imag, V=fit[0], I=fit[1], u=fit[2], v=fit[3], data_V=data[0], data_I=data[1])
    out["quality"] = quality.residual_stats(w, un, vn, out["best"][0], sys_.regions(sp["regions"])).rows
    return out


@pytest.mark.parametrize("ragged, geometry, mode", [(True, "wave", False), (False, "wave", False),
                                                    (False, "workgroup", False), (True, None, "sum")])
def test_device_batch_of_four_unit_systems(ragged, geometry, mode):
    """One FitBatch, fit k in system k (identity, E1, E2, descending): per fit, unscaled, bit for bit the lone run in the
    suite's units -- so no fit's scale leaks into a neighbour's descriptor record.  The descending fit's swarm is held
    to its own lone run (see the module docstring) and to the law at the identity run's best position.  Fits of
    different lengths run in the wave geometry alone (the library refuses the other), so the workgroup geometry has
    fits of one length; ``geometry`` None: the library's own choice, recorded."""
    from nmrfit_amd.batch import FitBatch
    fits = batch_fits(ragged)
    specs, lows, ups = [], [], []
    for sp, sys_ in zip(fits, BATCH_SYSTEMS):
        specs.append(sys_.spectrum(sp["w"], sp["u"], sp["v"], sp["weights"]))
        lo, up = sys_.box(sp["lower"], sp["upper"])
        lows.append(lo)
        ups.append(up)
    lone = [lone_fit(sp, us.IDENTITY, mode) for sp in fits]
    lone_desc = lone_fit(fits[3], us.DESC, mode)
    with FitBatch(specs, lows, ups, swarmsize=96, seeds=[sp["noise_seed"] + 1 for sp in fits], minstep=-1.0, minfunc=-1.0,
                  fit_im=mode) as b:
        if geometry is not None:
            b.set_geometry(geometry)
        b.add_noise([s.sigma(SIGMA[0]) for s in BATCH_SYSTEMS], [s.sigma(SIGMA[1]) for s in BATCH_SYSTEMS],
                    [sp["noise_seed"] for sp in fits])
        spectra = [b.spectrum(k) for k in range(4)]
        b.run(8, 4)
        ran = b.geometry()["mode"]
        assert geometry in (None, ran)
        states = [b.state(k) for k in range(4)]
        best = b.best()
        gen = b.generate()
        qual = b.residual_stats(regions=[s.regions(sp["regions"]) for s, sp in zip(BATCH_SYSTEMS, fits)])
        at = [s.params(l["best"][0]) for s, l in zip(BATCH_SYSTEMS, lone)]
        qual_at = b.residual_stats(X=at, regions=[s.regions(sp["regions"]) for s, sp in zip(BATCH_SYSTEMS, fits)])
    for k, (sys_, sp) in enumerate(zip(BATCH_SYSTEMS, fits)):
        tally = us.Tally("batch/%s/%s/fit_im=%s/fit %d" % ("ragged" if ragged else "equal", ran, mode, k), system=sys_,
                         N=sp["w"].size)
        ref = lone[k]
        tally.equal(sys_.un_inten(spectra[k][0]), ref["spectrum"][0], "spectrum u")
        tally.equal(sys_.un_inten(spectra[k][1]), ref["spectrum"][1], "spectrum v")
        tally.equal(sys_.un_quality(qual_at[k].rows), ref["quality"], "residual_stats at the identity run's best")
        if sys_ is us.DESC:
            ref, un_p, un_i, un_q = lone_desc, (lambda a: a), (lambda a: a), (lambda a: a)
        else:
            un_p, un_i, un_q = sys_.un_params, sys_.un_inten, sys_.un_quality
            w2, u2, v2 = sys_.spectrum(sp["w"], sp["u"], sp["v"])
            same, _, _ = preconditions(sys_, sp["w"], sp["u"], sp["v"], ref["x"], w2, u2, v2, sys_.params(ref["x"]))
            assert same.all()
        for key in ("x", "v", "p"):
            tally.equal(un_p(states[k][key]), ref[key], "state " + key)
        for key in ("fx", "fp"):
            tally.equal(un_i(states[k][key]), ref[key], "state " + key)
        tally.equal(un_p(best[k][0]), ref["best"][0], "best x")
        tally.equal(un_i(best[k][1]), ref["best"][1], "best f")
        for key, arr in ref["generate"].items():
            tally.equal(un_i(gen[k][key]), arr, "generate " + key)
        tally.equal(un_q(qual[k].rows), ref["quality"], "residual_stats")
        bad = tally.done()
        assert not bad, (k, bad[:5])


# ---- the lone entry points -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["E1", "E2", "E3", "DESC"])
def test_reconstruction_keeps_the_law(name):
    sys_ = dict(LAW, E3=us.E3)[name]
    w, u, v = make_grid("uniform", N=1500)
    w2, u2, v2 = sys_.spectrum(w, u, v)
    wout = np.linspace(w.min(), w.max(), 2250)
    tally = us.Tally("generate_result+contributions/%s" % name, system=sys_, P=(0, 9, 257))
    with Evaluator(w, u, v, np.ones(w.size)) as a, Evaluator(w2, u2, v2, np.ones(w.size)) as b:
        for P in (0, 9, 257):
            x = recon_x(w, P, seed=P + 3)
            x2 = sys_.params(x)
            assert us.in_range(w, u, v, x) and us.in_range(w2, u2, v2, x2)
            for grid in (None, wout):
                g2 = None if grid is None else sys_.grid(grid)
                for got, want in zip(b.generate_result(x2, g2), a.generate_result(x, grid)):
                    tally.equal(got, sys_.c * want, (P, grid is None, "generate_result"))
                for got, want in zip(b.contributions(x2, g2), a.contributions(x, grid)):
                    tally.equal(got, sys_.c * want, (P, grid is None, "contributions"))
    bad = tally.done()
    assert not bad, bad[:5]


def test_quality_noise_and_weights_keep_the_law():
    """residual_stats_many, replicas and compute_weights_many: one call holds the same spectrum in six systems (any
    power of two here: none of these kernels takes a square root of an intensity)."""
    systems = (us.IDENTITY, us.E1, us.E2, us.E3, us.DESC, us.Exact("odd", 2.0 ** -9, 2.0 ** 33))
    sp = synth.make_spectrum(2113, 6, seed=8, physical=True)
    x = synth.make_swarm(sp["lower"], sp["upper"], 2, seed=9)[1]
    reg = [(float(l - 2 * d), float(l + 3 * d)) for l, d in zip(sp["x_true"][5::3], sp["x_true"][4::3])][:4]
    tally = us.Tally("quality+noise+weights", systems=[s.name for s in systems])
    got = quality.residual_stats_many([s.spectrum(sp["w"], sp["u"], sp["v"]) for s in systems],
                                      [s.params(x) for s in systems], [s.regions(reg) for s in systems])
    assert np.all(got[0].rows[:-1, 0] > 0)
    for s, q in zip(systems, got):
        tally.equal(s.un_quality(q.rows), got[0].rows, ("residual_stats_many", s.name))
    rep = noise.replicas([s.inten(sp["u"]) for s in systems], [s.inten(sp["v"]) for s in systems],
                         [float(s.sigma(0.01)) for s in systems], [float(s.sigma(0.003)) for s in systems],
                         [77] * len(systems))
    for s, (un, vn) in zip(systems, rep):
        tally.equal(s.un_inten(un), rep[0][0], ("replicas u", s.name))
        tally.equal(s.un_inten(vn), rep[0][1], ("replicas v", s.name))

    def peaks(s):
        import types
        return [types.SimpleNamespace(bounds=(lo * s.ax, hi * s.ax), height=pk.height * s.c / abs(s.ax))
                for pk, (lo, hi) in zip(sp["peaks"], [(p.loc - 2 * p.width, p.loc + 3 * p.width) for p in sp["peaks"]])]
    wts, pairs = utils.compute_weights_many([s.grid(sp["w"]) for s in systems], [peaks(s) for s in systems],
                                            return_pairs=True)
    assert wts[0].min() < wts[0].max()
    tally.equal(wts[0], utils.compute_weights(sp["w"], peaks(us.IDENTITY)), "compute_weights_many against the host")
    for s, wk, pk in zip(systems, wts, pairs):
        tally.equal(wk, wts[0], ("compute_weights_many", s.name))
        tally.equal(pk, pairs[0], ("first and last", s.name))
    bad = tally.done()
    assert not bad, bad[:5]


E3M = us.Exact("E3m", 2.0 ** -10, 4.0 ** -3)        # E3's axis with an intensity factor that keeps the pair form


@pytest.mark.parametrize("name", ["E1", "E2", "E3m", "DESC"])
def test_normal_equations_keep_the_law(name):
    """Evaluator.jacobian(rows, c, s, normal=True) with transformed rows and factors, D = 76 and N = 700:
    A'_ik = A_ik c^2/(sigma_i sigma_k) and g' likewise, exactly; J and r too.  The rows are written by an instantiation
    of the objective kernel, form switch included: under E3 itself this particle leaves the pair form (its rows then
    differ by roundings, as test_objective_truth_where_e3_flips_the_form holds them), so E3's axis goes with 4^-3."""
    sys_ = dict(LAW, E3m=E3M)[name]
    sp = synth.make_spectrum(700, 24, seed=12, physical=True)
    x = synth.make_swarm(sp["lower"], sp["upper"], 2, seed=13)[1]
    assert x.size == 76
    rows, h = lsq.forward_rows(x, sp["lower"], sp["upper"])
    s = 1.0 / math.sqrt(700.0)
    w2, u2, v2, wt2 = sys_.spectrum(sp["w"], sp["u"], sp["v"], sp["weights"])
    rows2 = sys_.params(rows)
    same, f1, _ = preconditions(sys_, sp["w"], sp["u"], sp["v"], rows, w2, u2, v2, rows2)
    assert same.all() and all(f for f, _ in f1)
    assert not us.same_forms(rows, sp["w"], us.E3.params(rows), us.E3.grid(sp["w"]))[0].any()
    tally = us.Tally("normal equations/%s" % name, system=sys_, D=76, N=700)
    with Evaluator(sp["w"], sp["u"], sp["v"], sp["weights"]) as a, Evaluator(w2, u2, v2, wt2) as b:
        A = a.jacobian(rows, s / h, s, J=True, r=True, normal=True)
        B = b.jacobian(rows2, sys_.lsq_factors(s / h), s, J=True, r=True, normal=True)
    Au, gu = sys_.un_normal(B["A"], B["g"])
    tally.equal(Au, A["A"], "A")
    tally.equal(gu, A["g"], "g")
    tally.equal(B["J"], A["J"] * (sys_.c / sys_.pscale(76)), "J")
    tally.equal(B["r"], A["r"] * sys_.c, "r")
    tally.equal(B["f"], A["f"] * sys_.c, "f")
    bad = tally.done()
    assert not bad, bad[:5]


# ---- phase correction and peak picking: not covariant; the host comparisons at other intensities ------------------------

INTENSITIES = (3.7e8, 2.0 ** -30)


@pytest.mark.parametrize("c", INTENSITIES, ids=["x3.7e8", "x2^-30"])
def test_phase_scores_match_the_host_at_other_intensities(c):
    """The host comparisons of tests/test_gpu_phase.py on scaled spectra: ACME and peak minima at rtol 1e-12 (the
    absolute floor of the peak-minima comparison scaled with the data), brute exact, the device Nelder-Mead's nfev and
    nit equal to scipy.optimize.fmin's."""
    import scipy.optimize
    from nmrfit_amd import proc_autophase
    from tests.test_gpu_phase import _ragged
    zs = [c * z for z in _ragged((63, 64, 65, 3000, 4096))]
    ph = np.random.default_rng(11).uniform(-1e3, 1e3, (len(zs), 4, 2))
    ph[:, 0] = 0.0
    got = proc_autophase.phase_scores(zs, ph, "acme")
    want = np.array([[proc_autophase._ps_acme_score(p, z) for p in phk] for z, phk in zip(zs, ph)])
    rel = np.abs(got - want) / np.maximum(np.abs(want), 1e-300)
    print("units: phase/acme x%g: worst relative difference from the host %.3g" % (c, rel.max()))
    assert np.all((got == want) | (rel <= 1e-12)), rel.max()
    long_ = [c * z for z in _ragged((2000, 4096, 1000), seed=3)]
    ph = np.random.default_rng(5).uniform(-40, 40, (len(long_), 4, 2))
    got = proc_autophase.phase_scores(long_, ph, "peak_minima")
    want = np.array([[proc_autophase._ps_peak_minima_score(p, z) for p in phk] for z, phk in zip(long_, ph)])
    np.testing.assert_allclose(got, want, rtol=1e-12, atol=1e-15 * min(c, 1.0))
    angles = np.arange(-np.pi, np.pi, np.pi / 45)
    lev = proc_autophase.brute_levels([z.real for z in zs], [z.imag for z in zs], angles)
    for k, z in enumerate(zs):
        u, v = z.real.copy(), z.imag.copy()
        n = max(1, int(len(u) / 5000))
        for m, a in enumerate(angles):
            V, _ = proc_autophase.ps2(u, v, a, 0.0)
            err = np.sqrt((V[:n].mean() - V[-n:].mean()) ** 2)
            if np.max(V) > abs(np.min(V)):
                assert lev[k, m] == err, (k, m, lev[k, m], err)
            else:
                assert np.isnan(lev[k, m])
    long_ = [c * z for z in _ragged((4096, 3000), seed=31)]
    for fn, p0, p1 in (("acme", 0.0, 0.0), ("peak_minima", 5.0, -3.0)):
        x, f, nfev, nit = proc_autophase.estimate_many(long_, fn, p0, p1)
        for k, z in enumerate(long_):
            xs, fs, its, fev, _ = scipy.optimize.fmin(proc_autophase._SCORES[fn], [p0, p1], args=(z,), disp=False,
                                                      full_output=True)
            assert nfev[k] == fev and nit[k] == its, (fn, k, nfev[k], fev, nit[k], its)
            np.testing.assert_allclose(x[k], xs, rtol=0, atol=1e-8)
        print("units: phase/%s x%g: nfev %s nit %s equal fmin's" % (fn, c, [int(n) for n in nfev], [int(n) for n in nit]))


@pytest.mark.parametrize("c", INTENSITIES, ids=["x3.7e8", "x2^-30"])
def test_peak_sums_against_the_exact_truth_at_other_intensities(c):
    """One exactly-summed comparison of tests/peaks_support.py ("even count inside") with the intensities and ``thresh``
    scaled, that file's convergence-margin assertion kept."""
    from nmrfit_amd import peaks
    from tests import peaks_support
    from tests.test_gpu_peaks_edges import quiet, within
    case = peaks_support.BY_NAME["even count inside"]
    w, u, thresh, window = peaks_support.case_inputs(case)
    u, thresh = c * u, c * thresh
    em = quiet(peaks_support.emulate, w, u, thresh, window)
    assert peaks_support.all_margins_ok(em, thresh)
    got, base = quiet(peaks.find_peaks_many, [w], [u], thresh=thresh, window=window, return_baseline=True)
    got, base = got[0], base[0]
    ok = [within("x%g global baseline" % c, base, em.B, em.trace.err)]
    assert len(got) == len(em.peaks) > 0
    for g, p in zip(got, em.peaks):
        assert g.i == p["i"] and g.idx[0][0] == p["lo"] and g.idx[0][-1] == p["hi"] and g.width == p["width"]
        at = "x%g peak at %d, n = %d: " % (c, p["i"], p["n"])
        ok.append(within(at + "baseline", g.baseline, p["baseline"], p["base_err"]))
        ok.append(within(at + "height", g.height, p["height"], p["height_err"]))
        ok.append(within(at + "area", g.area, p["area"], p["area_err"]))
    us.record("peaks/x%g" % c, peaks=len(got), within_bounds=all(ok))
    assert all(ok)

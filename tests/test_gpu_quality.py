"""
GPU tier of the residual statistics (csrc/quality.hip, include/nmrfit_amd_quality.h; nmrfit_amd/quality.py,
FitBatch.residual_stats, FitUtility.residual_stats, fit_many(quality=True)): the device rows against the numpy mirror
applied to the reconstruction's own arrays, bit for bit; one function of (spectrum, x, regions) whatever the way in;
the sums against exactly summed high-precision truth; the edges; the state rule and the swarms left alone; the whole call.
"""
from fractions import Fraction

import numpy as np
import pytest

import nmrfit_amd
from nmrfit_amd import _cabi, quality, synth, utils
from nmrfit_amd.batch import FitBatch
from tests import hp_truth as hp

pytestmark = pytest.mark.gpu

NS, PS = (700, 257, 1), (3, 2, 1)


def region_kinds(w):
    """Five regions on a grid of 700 points: a single point, the pairs across a wave's and a tile's start, a reversed one
    that overlaps the pair before it, and one whose far edge lies beyond the grid's end."""
    h = w[1] - w[0]
    return [(w[100], w[100] + 0.2 * h), (w[63], w[64]), (w[255], w[256]), (w[300], w[250]), (w[690], 1.0e9)]


KIND_PAIRS = [(100, 100), (63, 64), (255, 256), (250, 300), (690, 699)]


@pytest.fixture(scope="module")
def three():
    """The three ragged fits after 12 generations in one batch: spectra, regions, best positions, the batch's own
    reconstruction and its rows (read-only: shared between the tests)."""
    specs = [synth.make_spectrum(n, p, seed=30 + k, physical=True) for k, (n, p) in enumerate(zip(NS, PS))]
    regions = [region_kinds(specs[0]["w"]), [], [(2.0, 5.0)]]          # R = 5 / 0 / 1 (the whole one-point grid)
    with make_batch(specs) as fb:
        fb.run(12, 4)
        X = [x for x, _ in fb.best()]
        gen = fb.generate()
        rows = [q.rows.copy() for q in fb.residual_stats(regions=regions)]
        again = [q.rows.copy() for q in fb.residual_stats(regions=regions)]
        given = [q.rows.copy() for q in fb.residual_stats(X, regions)]
    for a in X + rows:
        a.setflags(write=False)
    return dict(specs=specs, regions=regions, X=X, gen=gen, rows=rows, again=again, given=given)


def make_batch(specs, seeds=None):
    return FitBatch([(s["w"], s["u"], s["v"], s["weights"]) for s in specs], [s["lower"] for s in specs],
                    [s["upper"] for s in specs], swarmsize=16, seeds=seeds or [201 + k for k in range(len(specs))])


def same(a, b):
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


def finished(spec, x):
    """A FitUtility as a finished lone fit leaves it, at the parameters x."""
    f = utils.FitUtility(synth.SynthData(spec["w"], spec["u"], spec["v"], spec["peaks"]), list(spec["lower"]), list(spec["upper"]),
                         summary=False)
    f.params, f.error = np.array(x), 0.0
    return f


def reconstruction(spec, x):
    """(V, data_V) of the lone reconstruction (nmrfit_generate_result)."""
    f = finished(spec, x)
    f.generate_result()
    return np.array(f.V), np.array(f.data.V)


def test_bit_for_bit_against_the_mirror(three):
    """FitBatch.residual_stats() == residual_stats_host of that batch's own generate() arrays, all 8 quantities: e_j is
    the reconstruction's bits, the order is the header's."""
    assert [tuple(r) for r in quality.region_indices(three["specs"][0]["w"], three["regions"][0])] == KIND_PAIRS
    for k, (sp, reg) in enumerate(zip(three["specs"], three["regions"])):
        g = three["gen"][k]
        want = quality.residual_stats_host(g["V"], g["data_V"], sp["w"], reg)
        got = three["rows"][k]
        assert got.shape == (len(reg) + 2, 8)
        assert np.array_equal(got, want), (k, got, want)
        assert got[-2][0] == NS[k]
    assert [r[0] for r in three["rows"][0]] == [1, 2, 2, 51, 10, 700, 700 - 1 - 2 - 51 - 10]     # (region 2 lies in region 3)
    assert three["rows"][0][0][3] == 0.0                                     # a single point has no pair
    assert three["rows"][2][1][0] == 1 and three["rows"][2][2][0] == 0       # N = 1: the region is the grid, nothing left


def test_one_function_of_spectrum_x_and_regions(three):
    """The same rows from a batch of 3, batches of 1 (X given, before generation 0), nmrfit_quality_stats from host
    arrays (together and alone), FitUtility.residual_stats, and a second call."""
    specs, regions, X, rows = three["specs"], three["regions"], three["X"], three["rows"]
    for k in range(3):
        assert same(three["again"][k], rows[k]) and same(three["given"][k], rows[k])
        with make_batch([specs[k]], seeds=[77]) as one:
            assert same(one.residual_stats([X[k]], [regions[k]])[0].rows, rows[k])
    many = quality.residual_stats_many([(s["w"], s["u"], s["v"]) for s in specs], X, regions)
    for k, sp in enumerate(specs):
        assert same(many[k].rows, rows[k]) and many[k].nparams == 4 + 3 * PS[k]
        assert same(quality.residual_stats(sp["w"], sp["u"], sp["v"], X[k], regions[k]).rows, rows[k])
        f = finished(sp, X[k])
        assert same(f.residual_stats(regions[k]).rows, rows[k]) and f.quality.rows is not None
    # the default regions of a finished fit: its peaks' bounds
    f = finished(specs[0], X[0])
    bounds = [tuple(p.bounds) for p in specs[0]["peaks"]]
    assert same(f.residual_stats().rows, quality.residual_stats(specs[0]["w"], specs[0]["u"], specs[0]["v"], X[0], bounds).rows)
    with pytest.raises(AttributeError):
        utils.FitUtility(f.data, f.lower, f.upper, summary=False).residual_stats()


def test_descending_grid(three):
    """w descending: the regions are those of the reversed grid by the same argmin rule, and the rows are the mirror's
    of that problem's own reconstruction."""
    sp, x, reg = three["specs"][0], three["X"][0], three["regions"][0]
    back = dict(sp, w=sp["w"][::-1].copy())
    N = NS[0]
    assert [tuple(r) for r in quality.region_indices(back["w"], reg)] == [(N - 1 - b, N - 1 - a) for a, b in KIND_PAIRS]
    V, dV = reconstruction(back, x)
    got = quality.residual_stats(back["w"], back["u"], back["v"], x, reg).rows
    assert np.array_equal(got, quality.residual_stats_host(V, dV, back["w"], reg))
    assert [r[0] for r in got[:5]] == [1, 2, 2, 51, 10]


def test_truth():
    """One fit, N = 320, P = 2, two regions, phases of order 1: the rows against exact sums (Fraction) of the
    high-precision truth of every point.  With tau_j = tol_j(V) + tol_j(d), hp_truth's first-order bounds:
    sum e within sum tau + n eps sum|e|;  sum e^2 within sum(2|e| tau + tau^2) + n eps sum e^2;  sum d, sum d^2 likewise
    with tol_j(d);  sum (e_j - e_{j-1})^2 likewise with tau_j + tau_{j-1};  the maximum within max tau.  No constant but
    hp_truth's.  Worst used fraction of each bound, measured on the MI355X: sum e 5.8e-4, sum e^2 4.0e-3,
    sum step^2 3.2e-3, sum d 1.8e-3, sum d^2 1.5e-3, max 4.0e-3."""
    N, P = 320, 2
    sp = synth.make_spectrum(N, P, seed=41, physical=True)
    x = sp["x_true"].copy()
    x[0], x[1] = 1.1, -0.7
    x[4::3] *= 1.07
    w, u, v = sp["w"], sp["u"], sp["v"]
    regions = [tuple(sp["peaks"][0].bounds), (w[150], w[290])]
    rows = quality.residual_stats(w, u, v, x, regions).rows
    w0, wspan = hp.grid_frame(w)
    e, d, tau, told = [], [], [], []
    for j in range(N):
        t = hp.point(x, w, u, v, j, w0=w0, wspan=wspan, n_steps=0, imag=False)
        td = hp.C * hp.EPS * (abs(u[j]) + abs(v[j])) * (1 + abs(x[0]) + abs(x[1]))
        e.append(Fraction(t["Vf"]) - Fraction(t["V"]))
        d.append(Fraction(t["V"]))
        told.append(td)
        tau.append(t["tol_Vf"] + td)
    fl = quality.region_indices(w, regions)
    held = set()
    members = []
    for a, b in fl:
        members.append(list(range(a, b + 1)))
        held.update(members[-1])
    members += [list(range(N)), [j for j in range(N) if j not in held]]
    used = dict(sum_e=0.0, sum_e2=0.0, sum_step2=0.0, sum_d=0.0, sum_d2=0.0, max=0.0)

    def check(name, got, want, bound):
        err = abs(Fraction(float(got)) - want)
        assert err <= bound, (name, float(got), float(want), float(err), float(bound))
        used[name] = max(used[name], float(err / bound) if bound else 0.0)
    eps = Fraction(hp.EPS)
    for row, idx in zip(rows, members):
        n = len(idx)
        assert row[0] == n and n > 0
        T = [Fraction(tau[j]) for j in idx]
        E = [e[j] for j in idx]
        D = [d[j] for j in idx]
        TD = [Fraction(told[j]) for j in idx]
        check("sum_e", row[1], sum(E), sum(T) + n * eps * sum(abs(q) for q in E))
        check("sum_e2", row[2], sum(q * q for q in E), sum(2 * abs(q) * t + t * t for q, t in zip(E, T)) + n * eps * sum(q * q for q in E))
        in_row = set(idx)
        pairs = [j for j in idx if j - 1 in in_row]
        S = [e[j] - e[j - 1] for j in pairs]
        TS = [Fraction(tau[j]) + Fraction(tau[j - 1]) for j in pairs]
        check("sum_step2", row[3], sum(q * q for q in S), sum(2 * abs(q) * t + t * t for q, t in zip(S, TS)) + n * eps * sum(q * q for q in S))
        check("sum_d", row[4], sum(D), sum(TD) + n * eps * sum(abs(q) for q in D))
        check("sum_d2", row[5], sum(q * q for q in D), sum(2 * abs(q) * t + t * t for q, t in zip(D, TD)) + n * eps * sum(q * q for q in D))
        check("max", row[6], max(abs(q) for q in E), max(T))
        assert abs(e[int(row[7])]) >= max(abs(q) for q in E) - 2 * max(T) and int(row[7]) in in_row
    print("residual statistics against exact sums, worst used fraction of each bound: "
          + ", ".join("%s %.3g" % kv for kv in used.items()))


def test_edges():
    """N = 1, 256 and 257; 64 regions on one fit; a region equal to the whole grid; infinite edges; one NaN in u -- each
    against the mirror of the fit's own reconstruction, and by what the rows must say."""
    rng = np.random.default_rng(5)
    specs = [synth.make_spectrum(n, 2, seed=50 + k, physical=True) for k, n in enumerate((1, 256, 257, 600, 300, 300, 520))]
    X = [sp["lower"] + rng.random(sp["lower"].size) * (sp["upper"] - sp["lower"]) for sp in specs]
    w3, w4 = specs[3]["w"], specs[4]["w"]
    lo64 = rng.uniform(w3[0], w3[-1], 64)
    regions = [[(0.0, 9.0)],
               [(specs[1]["w"][0], specs[1]["w"][-1])],                       # the whole grid: the complement is empty
               [(specs[2]["w"][255], specs[2]["w"][256]), (specs[2]["w"][256], specs[2]["w"][256])],
               [(a, a + rng.uniform(0.0, 0.05)) for a in lo64],               # R = 64
               [(-np.inf, np.inf), (np.inf, w4[10]), (w4[20], -np.inf)],      # every distance infinite: index 0
               [],
               [(specs[6]["w"][60], specs[6]["w"][80]), (specs[6]["w"][100], specs[6]["w"][120])]]
    bad = dict(specs[6], u=specs[6]["u"].copy())
    bad["u"][70] = np.nan
    specs[6] = bad
    got = quality.residual_stats_many([(s["w"], s["u"], s["v"]) for s in specs], X, regions)
    for k, (sp, x, reg) in enumerate(zip(specs, X, regions)):
        V, dV = reconstruction(sp, x)
        want = quality.residual_stats_host(V, dV, sp["w"], reg)
        assert np.array_equal(got[k].rows, want, equal_nan=True), (k, got[k].rows, want)
    r = got[0].rows                                                          # N = 1
    assert list(r[:, 0]) == [1, 1, 0] and list(r[:, 3]) == [0, 0, 0] and list(r[:, 7]) == [0, 0, -1] and r[2][6] == 0
    r = got[1].rows                                                          # N = 256: one tile, the region is the grid
    assert list(r[:, 0]) == [256, 256, 0] and same(r[0], r[1]) and list(r[2]) == [0, 0, 0, 0, 0, 0, 0, -1]
    assert np.isnan(got[1].outside.rms[0]) and np.isnan(got[1].sigma_outside)
    r = got[2].rows                                                          # N = 257: the last point alone in its tile
    assert list(r[:, 0]) == [2, 1, 257, 255] and r[1][3] == 0 and r[0][3] > 0 and r[1][7] == 256
    assert got[3].rows.shape == (66, 8) and np.all(got[3].rows[:64, 0] >= 1)
    r = got[4].rows                                                          # infinite edges
    assert list(r[:, 0]) == [1, 11, 21, 300, 300 - 21]
    assert same(got[5].rows[0], got[5].rows[1])                              # R = 0: the complement is the whole grid
    r = got[6].rows                                                          # a NaN at point 70
    assert np.isnan(r[0][1:6]).all() and np.isnan(r[2][1:6]).all() and not np.isnan(r[1]).any() and not np.isnan(r[3]).any()
    assert list(r[:, 0]) == [21, 21, 520, 520 - 42] and r[0][7] != 70 and 60 <= r[0][7] <= 80 and r[0][6] > 0


def test_state_rule_and_the_swarms_left_alone(three):
    """X=None before generation 0 raises with the state code, X given works there; statistics taken between two runs
    of 5 generations leave best() and state() as those of an untouched twin run for 10 generations, bit for bit."""
    specs, regions = three["specs"], three["regions"]
    with make_batch(specs) as a, make_batch(specs) as b:
        with pytest.raises(_cabi.NmrfitError) as ei:
            a.residual_stats(regions=regions)
        assert ei.value.code == _cabi.E_STATE
        assert len(a.residual_stats(three["X"], regions)) == 3
        a.run(5, 64)
        mid = a.residual_stats(regions=regions)
        assert all(q.rows.shape == (len(r) + 2, 8) for q, r in zip(mid, regions))
        a.run(5, 64)
        b.run(10, 64)
        for (xa, fa), (xb, fb) in zip(a.best(), b.best()):
            assert np.array_equal(xa, xb) and fa == fb
        for k in range(3):
            sa, sb = a.state(k), b.state(k)
            assert all(np.array_equal(sa[name], sb[name]) for name in sa)
        assert [s["iteration"] for s in a.status()] == [s["iteration"] for s in b.status()]


def test_fit_many_quality():
    """fit_many(jobs, quality=True): four small jobs -- one of another length, one polished in the batch, one that runs
    alone -- each fit.quality == residual_stats(w, u, v, fit.params, bounds); params and error as without the keyword."""
    def jobs():
        out = []
        for k, (n, p) in enumerate(((512, 2), (512, 3), (700, 2), (512, 2))):
            sp = synth.make_spectrum(n, p, seed=60 + k, physical=True)
            opts = dict(swarmsize=16, maxiter=15, seed=300 + k)
            if k == 1:
                opts["polish"] = True
            if k == 3:
                opts["variant"] = "norec"                                      # (not batchable: runs alone)
            out.append(dict(data=synth.SynthData(sp["w"], sp["u"], sp["v"], sp["peaks"]), lower=list(sp["lower"]),
                            upper=list(sp["upper"]), options=opts))
        return out
    with_q = nmrfit_amd.fit_many(jobs(), batch_polish=True, quality=True)
    without = nmrfit_amd.fit_many(jobs(), batch_polish=True)
    for f, g in zip(with_q, without):
        assert np.array_equal(f.params, g.params) and f.error == g.error
        assert "quality" not in vars(g)
        bounds = [tuple(p.bounds) for p in f.data.peaks]
        want = nmrfit_amd.residual_stats(f.data.w, f.data.u, f.data.v, f.params, bounds)
        assert isinstance(f.quality, nmrfit_amd.FitQuality) and f.quality.nparams == len(f.lower)
        assert np.array_equal(f.quality.rows, want.rows)
        assert f.quality.rows.shape == (len(bounds) + 2, 8) and f.quality.sigma_outside > 0

"""
GPU tier: the residual ROWS, R[b, j] = weights[j] (data - model) of both channels, read one grid point at a time against
the high-precision truth (tests/hp_truth.py) at the kernels' switches.

Every least-squares product starts from these rows -- J and r are tied to them bit for bit, A = J^T J and g = J^T r to
exactly summed truth OF them -- and they are written by instantiations of the objective kernel of their own
(objective_kernel.h, WRITE_R): other machine code than the objective launches that tests/test_gpu_pointwise.py and
tests/test_gpu_pointwise_forms.py read through one-hot weights, with a row store that has its own index arithmetic and
ragged-tail predicate, and WITHOUT the Gaussian recurrence.  The particles are those two files' own (peaks at the
Gaussian window's edge, the Dawson table's boundaries, the far-field switch, needles, widths below the floor, negative
widths, r outside [0, 1]; the five classes of the two per-particle form switches), the bound is hp_truth's plain one
-- never the recurrence's term, particles of the *_rec classes included -- times |weights[j]|.  One launch returns every
point of a row, so no one-hot weights are needed: the weights are uniform(0.5, 2) with exact zeros and one negative value
at a probed point (tests/rows_support.py).

    rows at the switches     four grids, 15 probes, P = 0, 1, 8, 9, 32, 33 (65, 130 at every fourth probe); every variant
                             that writes rows (real), the DEFAULT kernel's rows of both channels in both modes, FARFIELD32
                             = FARFIELD bit for bit, the refusals of the other variants
    every form class         uniform1101 and uniform8781, full chunks (first and second of a phase block) and the ragged
                             tail, rows 0 to 7 of a lane, the a-priori assertions of class and placement kept
    the launch form          one segment, workgroup = particle, partial sums + finalize: the same bits
    f                        every returned RMSE against the exactly summed squares of its own returned row
    the batch                FitBatch.normal_equations at hostile points, ragged in N and P, against lone contexts bit for bit

Each test prints its worst err/tol ratios (recorded in profiles/r09/rows_pointwise.txt).
"""
import math

import numpy as np
import pytest

from nmrfit_amd import _cabi, lsq
from nmrfit_amd.equations import Evaluator
from tests import hp_truth as hp
from tests import lsq_support as S
from tests import rows_support as RS

pytestmark = pytest.mark.gpu

MODE_ARG = {1: True, 2: "sum"}
IM_CHANNEL = {1: "im1", 2: "im2"}


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    assert _cabi.device_count() >= 1


def row_variants():
    """The kernels that write rows: DEFAULT, FARFIELD, NOREC and the A/B forms of an A/B build (a context set to
    FARFIELD32 runs FARFIELD's)."""
    out = [var for var in _cabi.available_variants() if var != _cabi.VARIANT_FARFIELD32]
    assert {_cabi.VARIANT_DEFAULT, _cabi.VARIANT_FARFIELD, _cabi.VARIANT_NOREC} <= set(out)
    return out


def worsts(name):
    return {ch: hp.Worst("%s/%s" % (name, ch)) for ch in RS.CHANNELS}


def report(worst):
    fails = []
    for wo in worst.values():
        fails += wo.report()
    return fails


def refused(ev, X):
    for mode in (1, 2):
        with pytest.raises(_cabi.NmrfitError) as ei:
            ev.residual_batch_im(X, MODE_ARG[mode])
        assert ei.value.code == _cabi.E_UNSUPPORTED, ei.value


def check_stack(ev, X, points, wt, zeros, worst, tag):
    """One residual_batch call per variant for the stack X (and the DEFAULT kernel's call for both channels per mode),
    read at ``points``: [(j, [truth of row s at j])]."""
    P = (X.shape[1] - 4) // 3

    def read(R, ch, what):
        assert R.shape == (X.shape[0], wt.size)
        assert not R[:, zeros].any(), tag + (what,)          # a weight of zero: a residual of zero, exactly
        for j, truths in points:
            for s, t in enumerate(truths):
                RS.check_point(worst[ch], R[s, j], t, ch, wt[j], tag + (what, j, P, s))

    rows = {}
    for var in row_variants():
        ev.set_variant(var)
        R = ev.residual_batch(X)
        read(R, "re", var)
        rows[var] = R
        # both channels: the DEFAULT kernel alone (every other variant of the context is refused)
        if var != _cabi.VARIANT_DEFAULT:
            refused(ev, X)
            np.testing.assert_array_equal(ev.residual_batch(X), R, err_msg="after the refusal: %s" % (tag + (var,),))
    ev.set_variant(_cabi.VARIANT_FARFIELD32)
    np.testing.assert_array_equal(ev.residual_batch(X), rows[_cabi.VARIANT_FARFIELD], err_msg=str(tag))
    refused(ev, X)
    ev.set_variant(_cabi.VARIANT_DEFAULT)
    for mode in (1, 2):
        R_re, R_im, _ = ev.residual_batch_im(X, MODE_ARG[mode])
        np.testing.assert_array_equal(R_re, rows[_cabi.VARIANT_DEFAULT], err_msg="real rows, mode %d, %s" % (mode, tag))
        read(R_re, "re", "both%d" % mode)
        read(R_im, IM_CHANNEL[mode], "both%d" % mode)


@pytest.mark.parametrize("kind", RS.SWITCH_KINDS)
def test_rows_at_the_switches(kind):
    w, u, v = RS.make_grid(kind)
    N = w.size
    js = RS.switch_probes(N)
    wt, zeros = RS.hostile_weights(N, js, seed=5)
    assert sum(wt[j] < 0 for j in js) == 1 and zeros.size == 5
    worst = worsts("rows/switches/%s" % kind)
    with Evaluator(w, u, v, wt) as ev:
        for n, j in enumerate(js):
            for P, X in RS.switch_stacks(w, n, j).items():
                truths = [RS.truth((kind, N, j, X.shape[1], s), x, w, u, v, j) for s, x in enumerate(X)]
                check_stack(ev, X, [(j, truths)], wt, zeros, worst, (kind,))
        # no peak: the row is weights V, the rotated data, at every probe
        X = RS.X_NO_PEAK
        check_stack(ev, X, [(j, [RS.truth((kind, N, j, 4, 0), X[0], w, u, v, j)]) for j in js], wt, zeros, worst, (kind,))
    fails = report(worst)
    assert not fails, fails[:5]


@pytest.mark.parametrize("grid,cls", [(g, c) for g in RS.CLASS_GRIDS for c in RS.CLASSES])
def test_rows_of_every_form_class(grid, cls):
    w, u, v = RS.class_grid(grid)
    N = w.size
    frame = hp.grid_analysis(w)
    assert frame[2] != 0.0                                     # a uniform grid: the objective WOULD take the recurrence
    chunks, large = RS.class_probes(N, cls)
    for kind, c, p in chunks:
        full = (c + 1) * hp.CHUNK <= N
        assert full == (kind != "tail")
        assert [q for q, _ in p] == list(range(hp.ROWS if full else (N - 1 - c * hp.CHUNK) // hp.WAVE + 1)), (kind, p)
    assert {k for k, _, _ in chunks} == ({"first", "second", "tail"} if hp.block_len(N) > hp.CHUNK else {"first", "tail"})
    wt, zeros = RS.hostile_weights(N, [j for _, _, p in chunks for _, j in p], seed=9)
    worst = worsts("rows/forms/%s/%s" % (grid, cls))
    with Evaluator(w, u, v, wt) as ev:
        for kind, c, p in chunks:
            for P, X in RS.class_stacks(w, c, cls, frame).items():
                points = [(j, [RS.truth((grid, kind, cls, j, X.shape[1], s), x, w, u, v, j) for s, x in enumerate(X)])
                          for _, j in p if P not in RS.P_ROW or j in large]
                if points:
                    check_stack(ev, X, points, wt, zeros, worst, (grid, kind, cls))
    fails = report(worst)
    assert not fails, fails[:5]


# ---- the launch form --------------------------------------------------------------------------------------------------

FORM_GRIDS = (2 * hp.CHUNK + 77, 3 * hp.CHUNK + 77, 17 * hp.CHUNK + 77)     # 3, 4 and 18 chunks, the last one ragged
ROWS_BYTES = 40e6                                                          # of rows per call, at most


def launch_form(g):
    return "one" if g["segments"] == 1 else "workgroup" if g["segments"] == g["waves_per_workgroup"] else "partial"


def test_rows_do_not_depend_on_the_launch_form():
    """The hostile stacks of one probe per grid, alone and tiled to as many rows as 40 MB hold: the launch names its form
    (one segment; the workgroup holds the particle; partial sums + finalize), every row and RMSE of the large call is the
    small call's, bit for bit, in both channels.  The truth is checked on the small call; the bits carry it."""
    assert hp.block_len(FORM_GRIDS[2]) == 2 * hp.CHUNK and all(N % hp.CHUNK == 77 for N in FORM_GRIDS)
    seen = {"re": {}, 1: {}, 2: {}}
    worst = worsts("rows/launch forms")
    for N, j in zip(FORM_GRIDS, (64, hp.CHUNK + 64 + 12, FORM_GRIDS[2] - 1)):
        w, u, v = RS.make_grid("uniform", N, seed=N)
        wt, zeros = RS.hostile_weights(N, [j], seed=N)
        Xs = RS.particles(w, j, with_large=False)
        with Evaluator(w, u, v, wt) as ev:
            for P in (1, 9, 33):
                X = Xs[P]
                n = X.shape[0]
                truths = [RS.truth(("forms", N, j, X.shape[1], s), x, w, u, v, j) for s, x in enumerate(X)]
                check_stack(ev, X, [(j, truths)], wt, zeros, worst, (N,))
                R, f = ev.residual_batch(X, return_f=True)
                seen["re"].setdefault(launch_form(ev.last_launch()), []).append((N, n))
                big = int(ROWS_BYTES / (8 * N))
                RL, fL = ev.residual_batch(np.resize(X, (big, X.shape[1])), return_f=True)
                seen["re"].setdefault(launch_form(ev.last_launch()), []).append((N, big))
                np.testing.assert_array_equal(RL, np.resize(R, RL.shape), err_msg="real rows %s" % ((N, P, big),))
                np.testing.assert_array_equal(fL, np.resize(f, fL.shape), err_msg="f %s" % ((N, P, big),))
                del RL
                for mode in (1, 2):
                    R_re, R_im, f2 = ev.residual_batch_im(X, MODE_ARG[mode])
                    seen[mode].setdefault(launch_form(ev.last_launch()), []).append((N, n))
                    np.testing.assert_array_equal(R_re, R)
                    np.testing.assert_array_equal(f2[:, 0], f)
                    big = int(ROWS_BYTES / (16 * N))
                    L_re, L_im, L2 = ev.residual_batch_im(np.resize(X, (big, X.shape[1])), MODE_ARG[mode])
                    seen[mode].setdefault(launch_form(ev.last_launch()), []).append((N, big))
                    np.testing.assert_array_equal(L_re, np.resize(R, L_re.shape), err_msg="real rows %s" % ((N, P, mode, big),))
                    np.testing.assert_array_equal(L_im, np.resize(R_im, L_im.shape), err_msg="imaginary rows %s" % ((N, P, mode, big),))
                    np.testing.assert_array_equal(L2, np.resize(f2, L2.shape), err_msg="f2 %s" % ((N, P, mode, big),))
                    del L_re, L_im
    for key, forms in seen.items():
        print("rows/launch forms: %s: %s" % (key, "; ".join("%s at (N, rows) = %s" % (k, sorted(set(q))) for k, q in sorted(forms.items()))))
        assert set(forms) == {"one", "workgroup", "partial"}, (key, forms)
    fails = report(worst)
    assert not fails, fails[:5]


# ---- f --------------------------------------------------------------------------------------------------------------------

def exact_rms(row):
    """sqrt(sum_j row_j^2 / N) from the EXACT sum of the exact squares, rounded once (lsq_support.two_product, fsum)."""
    p, e = S.two_product(row, row)
    return math.sqrt(math.fsum(np.concatenate((p, e)).tolist()) / row.size)


@pytest.mark.parametrize("kind", ["uniform", "unsorted"])
def test_f_is_the_rms_of_the_returned_rows(kind):
    """Every RMSE a rows call returns -- f of residual_batch(return_f=True) in every variant, both columns of f2 -- against
    the exactly summed squares of its own returned row, within f (sum_bound(N, 1) + 4 u): two sums of the same N squares,
    each within sum_bound of the exact one, a division and a root each.  The hostile rows span many orders of magnitude
    (a needle's peak beside noise): a dropped or doubled block sum is not diluted."""
    w, u, v = RS.make_grid(kind)
    N = w.size
    js = RS.switch_probes(N)
    wt, _ = RS.hostile_weights(N, js, seed=5)
    worst = hp.Worst("rows/f/%s" % kind)
    spread = 0.0
    with Evaluator(w, u, v, wt) as ev:
        for n, j in enumerate(js):
            if j not in (0, 64, 2048, N - 1):
                continue
            for P, X in list(RS.switch_stacks(w, n, j).items()) + [(0, RS.X_NO_PEAK)]:
                for var in row_variants():
                    ev.set_variant(var)
                    R, f = ev.residual_batch(X, return_f=True)
                    assert np.isfinite(R).all() and np.isfinite(f).all()
                    for s in range(X.shape[0]):
                        worst.check(f[s], exact_rms(R[s]), f[s] * (S.sum_bound(N, 1.0) + 4 * S.U), (var, "f", j, P, s))
                spread = max(spread, float(np.max(np.abs(R).max(axis=1) / f)))
                ev.set_variant(_cabi.VARIANT_DEFAULT)
                for mode in (1, 2):
                    R_re, R_im, f2 = ev.residual_batch_im(X, MODE_ARG[mode])
                    assert np.isfinite(R_im).all() and np.isfinite(f2).all()
                    for ch, Rc in enumerate((R_re, R_im)):
                        for s in range(X.shape[0]):
                            worst.check(f2[s, ch], exact_rms(Rc[s]), f2[s, ch] * (S.sum_bound(N, 1.0) + 4 * S.U),
                                        ("f2", mode, ch, j, P, s))
    print("rows/f/%s: largest max|R| / f of a row %.3g (sqrt(N) = %.3g: one point carries the sum)" % (kind, spread, math.sqrt(N)))
    fails = worst.report()
    assert not fails, fails[:5]


# ---- the batch ------------------------------------------------------------------------------------------------------------

BATCH_FITS = ((hp.CHUNK, 1, "uniform", 511, 22), (700, 8, "unsorted", 699, 3), (16 * hp.CHUNK + 8, 9, "descending", 8 * hp.CHUNK + 64, 0))
BATCH_ORDER = (0, 1, 2, 0, 1, 2, 1)      # seven fits: two parts (a batch splits from K = 6), the fits recur across the boundary


@pytest.fixture(scope="module")
def hostile_fits():
    """Three fits -- N of one chunk, 700 and 17 chunks; P = 1, 8, 9 -- each with hostile weights, a hostile point of the
    switch builders (a needle narrower than a grid step; the group with the needles, the line wider than the span, the
    width below the floor and the negative width; the centred peak with the Gaussian window's edges) and a box drawn
    round the point.  Fit 1 sits on its upper bound: every forward step flips."""
    fits = []
    for k, (N, P, kind, j, row) in enumerate(BATCH_FITS):
        w, u, v = RS.make_grid(kind, N, seed=20 + k)
        wt, _ = RS.hostile_weights(N, [j], seed=30 + k)
        x = RS.particles(w, j, with_large=False)[P][row].copy()
        d = 0.01 * np.abs(x) + 1e-6
        lower, upper = x - d, (x.copy() if k == 1 else x + d)
        rows, h = lsq.forward_rows(x, lower, upper)
        assert np.all(h < 0) if k == 1 else np.all(h > 0)
        fits.append(dict(spec=(w, u, v, wt), x=x, lower=lower, upper=upper))
    assert [hp.block_len(f["spec"][0].size) // hp.CHUNK for f in fits] == [1, 1, 2]
    return fits


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_batch_rows_at_hostile_points(hostile_fits, mode, monkeypatch):
    from nmrfit_amd.batch import FitBatch
    fits = hostile_fits
    lone = []
    for f in fits:
        with Evaluator(*f["spec"]) as ev:
            m = lsq.ResidualModel(ev, f["lower"], f["upper"], fit_im=MODE_ARG[mode] if mode else 0)
            q = dict(combined=m.normal_equations(f["x"]))
            if mode:
                rows, h = lsq.forward_rows(f["x"], f["lower"], f["upper"])
                s = 1.0 / np.sqrt(f["spec"][0].size)
                q["channels"] = ev.jacobian_im(rows, s / h, s, MODE_ARG[mode], normal=True)
            lone.append(q)
        A, g, fk = q["combined"]
        assert np.isfinite(A).all() and np.isfinite(g).all() and np.isfinite(fk) and A.any() and g.any()
    order = BATCH_ORDER
    X = [fits[k]["x"] for k in order]
    with FitBatch([fits[k]["spec"] for k in order], [fits[k]["lower"] for k in order], [fits[k]["upper"] for k in order],
                  swarmsize=8, seeds=list(range(1, len(order) + 1)), fit_im=MODE_ARG[mode] if mode else False) as fb:
        for budget in (None, "1"):
            if budget:
                monkeypatch.setenv("NMRFIT_LSQ_WORKSPACE_MB", budget)
            got = fb.normal_equations(X, channels="both" if mode else "real")
            for i, ((A, g, fk), k) in enumerate(zip(got, order)):
                A0, g0, f0 = lone[k]["combined"]
                np.testing.assert_array_equal(A, A0, err_msg="A of fit %d (position %d), budget %s" % (k, i, budget))
                np.testing.assert_array_equal(g, g0, err_msg="g of fit %d (position %d), budget %s" % (k, i, budget))
                assert fk == f0, (k, i, budget)
            if mode:
                from tests.test_gpu_lsq_im import _raw_batch_call
                for i, ((A, g, f2), k) in enumerate(zip(_raw_batch_call(fb, X), order)):
                    q = lone[k]["channels"]
                    np.testing.assert_array_equal(A, q["A"], err_msg="A per channel of fit %d (position %d), budget %s" % (k, i, budget))
                    np.testing.assert_array_equal(g, q["g"], err_msg="g per channel of fit %d (position %d), budget %s" % (k, i, budget))
                    np.testing.assert_array_equal(f2, q["f2"], err_msg="f2 of fit %d (position %d), budget %s" % (k, i, budget))

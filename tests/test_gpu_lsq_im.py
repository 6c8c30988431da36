"""
GPU tier of least squares on both channels (include/nmrfit_amd_lsq_im.h; csrc/objective_rows_im.hip, lsq.hip, batch_lsq.hip).

Rows: the real rows and rho_re of the new call against nmrfit_residual_batch bit for bit, (rho_re + rho_im)/2 against
nmrfit_objective_batch, rho_im against the RMS of the returned imaginary rows, and the imaginary rows point by point
against the mpmath truth of tests/hp_truth.py (its own first-order bound, C = 32) -- in every geometry a residual launch
takes (one segment, workgroup = particle, partial sums + finalize).  J and r per channel bit for bit against the host
expressions of the returned rows; A and g per channel within the derived bound of exactly summed truth, the same bits on a
second call, in any batch and under any workspace grouping; FitBatch.normal_equations / polish(channels="both") and
fit_many(batch_polish="both"); the refusals.

Shapes, the smallest that cross each boundary: N = 1, 63, 64, 65 (the LSQ tile of 64, full and ragged), 511, 512, 513 (the
512-point chunk), 1537 (four chunks = four blocks: the workgroup holds the particle), N_MULTI (blocks of two chunks,
hp_truth.block_len); P = 1, 2, 3 everywhere, P = 24 (D = 76, the reduction kernel's largest) and P = 25 (beyond it) once.

What this file covers of the rows, and what it does not: synth spectra at three parameter rows (inside the box, one needle,
one centred peak) with at most three peaks -- never a second group of eight, the Gaussian window's edge from outside the
chunk, the Dawson table's boundaries, a width below the floor, a negative width or r outside [0, 1].  Those, P up to 130,
the five classes of the kernel's form switches, weights with zeros and a negative value, and the real rows against the same
truth (here they are tied to nmrfit_residual_batch bit for bit, no more) are in tests/test_gpu_rows_pointwise.py; so is
the batch at such points.
"""
import math

import numpy as np
import pytest

from nmrfit_amd import _cabi, lsq, synth
from tests import hp_truth as hp
from tests import lsq_im_support as M
from tests import lsq_support as S

pytestmark = pytest.mark.gpu

NS = (1, 63, 64, 65, 511, 512, 513, 1537)
N_MULTI = 16 * hp.CHUNK + 8             # 17 chunks: blocks of two chunks, nine blocks, a ragged last chunk of 8 points
assert hp.block_len(N_MULTI) == 2 * hp.CHUNK
PS = (1, 2, 3)
SHAPES = [(N, P) for N in NS + (N_MULTI,) for P in PS]
MODE_ARG = {1: True, 2: "sum"}


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    assert _cabi.device_count() >= 1


_SPECTRA = {}


def _spectrum(N, P):
    if (N, P) not in _SPECTRA:
        _SPECTRA[(N, P)] = synth.make_spectrum(N, P, seed=200 + N % 89 + P, physical=True)
    return _SPECTRA[(N, P)]


def _interior(sp, seed=7):
    return synth.make_swarm(sp["lower"], sp["upper"], 2, seed=seed)[1]


def _step(w):
    return float(w[1] - w[0]) if w.size > 1 else 1e-3


def _probe_rows(sp):
    """Three parameter rows: inside the box; peak 0 a needle narrower than a grid step; peak 0 centred on a grid point."""
    w = sp["w"]
    N = w.size
    x = _interior(sp)
    jc = int(np.argmin(np.abs(w - x[5])))
    needle, centred = x.copy(), x.copy()
    needle[4] = 0.01 * _step(w)
    needle[5] = w[jc] + 0.3 * _step(w)
    centred[5] = w[jc]
    return np.stack([x, needle, centred]), jc


def _sample(N, jc):
    """Every point up to N = 65; beyond, chunk and block edges, the tile edges of the first chunk, the last point, the
    centre of peak 0 and its neighbours."""
    if N <= 65:
        return list(range(N))
    bl = hp.block_len(N)
    js = {0, 1, 63, 64, 65, N - 1, N - 2, jc - 1, jc, jc + 1}
    for c in range(0, N, hp.CHUNK):
        js.update((c - 1, c, c + 1))
    for b in range(0, N, bl):
        js.update((b - 1, b))
    return sorted(j for j in js if 0 <= j < N)


_TRUTH = {}


def _truth(N, P, b, j, x, sp):
    key = (N, P, b, j)
    if key not in _TRUTH:
        _TRUTH[key] = hp.point(x, sp["w"], sp["u"], sp["v"], j)
    return _TRUTH[key]


def _evaluator(sp):
    from nmrfit_amd.equations import Evaluator
    return Evaluator(*S.spectrum_tuple(sp))


@pytest.mark.parametrize("N, P", SHAPES)
def test_rows_of_both_channels(N, P):
    sp = _spectrum(N, P)
    X, jc = _probe_rows(sp)
    wt = sp["weights"]
    worst = hp.Worst("R_im N %d P %d" % (N, P))
    with _evaluator(sp) as ev:
        R, f = ev.residual_batch(X, return_f=True)
        for mode in M.MODES:
            R_re, R_im, f2 = ev.residual_batch_im(X, MODE_ARG[mode])
            geom = ev.last_launch()
            np.testing.assert_array_equal(R_re, R, err_msg="real rows, mode %d" % mode)
            np.testing.assert_array_equal(f2[:, 0], f, err_msg="rho_re, mode %d" % mode)
            fo = ev.objective_batch(X, fit_im=MODE_ARG[mode])
            mean = 0.5 * (f2[:, 0] + f2[:, 1])
            print("N %d P %d mode %d (%d segments): (rho_re + rho_im)/2 %s  objective_batch %s  max relative difference %.3g"
                  % (N, P, mode, geom["segments"], mean, fo, np.max(np.abs(mean - fo) / fo)))
            np.testing.assert_array_equal(mean, fo, err_msg="mean of the two RMSEs against nmrfit_objective_batch, mode %d" % mode)
            # rho_im against the RMS of the returned rows: two sums of the same N squares, each within sum_bound of the
            # exact one -- together twice the bound on the sum, once on its root -- and a division and a root each: 4 u
            rms = np.sqrt(np.mean(R_im * R_im, axis=1))
            tol = f2[:, 1] * (S.sum_bound(N, 1.0) + 4 * S.U)
            assert np.all(np.abs(rms - f2[:, 1]) <= tol), (rms, f2[:, 1], tol)
            for b, x in enumerate(X):
                for j in _sample(N, jc):
                    t = _truth(N, P, b, j, x, sp)
                    want, bar = (t["dI1"], t["tol_I1"]) if mode == 1 else (t["dI2"], t["tol_I2"])
                    worst.check(R_im[b, j], wt[j] * want, wt[j] * bar, (mode, b, j))
    fails = worst.report()
    assert not fails, fails[:5]


def test_rows_in_every_geometry():
    """The three forms a residual launch takes, named by the launch itself: one segment (many rows), the workgroup holds
    the particle (as many segments as waves), partial sums + finalize.  Rows and RMSEs do not depend on the form: the rows
    of a large call equal the same rows in a small one."""
    for N, B, want in ((1537, 3, "workgroup"), (513, 3, "partial"), (513, 4100, "one"), (N_MULTI, 3, "partial")):
        sp = _spectrum(N, 1)
        X = synth.make_swarm(sp["lower"], sp["upper"], B, seed=5)
        with _evaluator(sp) as ev:
            for mode in M.MODES:
                R_re, R_im, f2 = ev.residual_batch_im(X, MODE_ARG[mode])
                g = ev.last_launch()
                form = "one" if g["segments"] == 1 else "workgroup" if g["segments"] == g["waves_per_workgroup"] else "partial"
                assert form == want, (N, B, g)
                R, f = ev.residual_batch(X, return_f=True)
                np.testing.assert_array_equal(R_re, R)
                np.testing.assert_array_equal(f2[:, 0], f)
                np.testing.assert_array_equal(0.5 * (f2[:, 0] + f2[:, 1]), ev.objective_batch(X, fit_im=MODE_ARG[mode]))
                if B > 3:
                    a_re, a_im, a2 = ev.residual_batch_im(X[:3], MODE_ARG[mode])
                    np.testing.assert_array_equal(R_im[:3], a_im)
                    np.testing.assert_array_equal(f2[:3], a2)


def _jacobian_case(N, P, mode, exact=True):
    sp = _spectrum(N, P)
    D = 4 + 3 * P
    s = 1.0 / np.sqrt(N)
    with _evaluator(sp) as ev:
        m = lsq.ResidualModel(ev, sp["lower"], sp["upper"], fit_im=MODE_ARG[mode])
        for where, x in (("interior", _interior(sp)), ("upper bound", np.array(sp["upper"], dtype=float))):
            rows, h = m.rows(x)
            c = s / h
            R_re, R_im, f2 = ev.residual_batch_im(rows, MODE_ARG[mode])
            out = ev.jacobian_im(rows, c, s, MODE_ARG[mode], J=True, r=True, normal=True)
            assert out["J"].shape == (2, N, D)
            np.testing.assert_array_equal(out["f2"], f2[0])
            for ch, R in enumerate((R_re, R_im)):
                J_host = np.ascontiguousarray(((R[1:] - R[0]) * (s / h[:, None])).T)
                r_host = R[0] * s
                np.testing.assert_array_equal(out["J"][ch], J_host, err_msg="J, channel %d, %s" % (ch, where))
                np.testing.assert_array_equal(out["r"][ch], r_host, err_msg="r, channel %d, %s" % (ch, where))
                A, g = out["A"][ch], out["g"][ch]
                np.testing.assert_array_equal(A, A.T)
                if exact and (where == "interior" or D < 76):
                    Ax, gx, absA, absg = S.exact_normal_equations(J_host, r_host)
                    with np.errstate(invalid="ignore", divide="ignore"):     # (an entry that is exactly zero: 0 / 0)
                        print("N %d P %d mode %d channel %d %s: max |A - exact| / bound %.3g, g %.3g" % (
                            N, P, mode, ch, where, np.nanmax(np.abs(A - Ax) / S.sum_bound(N, absA)),
                            np.nanmax(np.abs(g - gx) / S.sum_bound(N, absg))))
                    assert np.all(np.abs(A - Ax) <= S.sum_bound(N, absA))
                    assert np.all(np.abs(g - gx) <= S.sum_bound(N, absg))
            # the real channel is nmrfit_jacobian's, bit for bit
            one = ev.jacobian(rows, c, s, J=True, r=True, normal=True)
            for key in ("J", "r", "A", "g"):
                np.testing.assert_array_equal(out[key][0], one[key], err_msg="real channel against nmrfit_jacobian: " + key)
            assert out["f2"][0] == one["f"]
            again = ev.jacobian_im(rows, c, s, MODE_ARG[mode], J=True, r=True, normal=True)
            for key in ("J", "r", "A", "g", "f2"):
                np.testing.assert_array_equal(again[key], out[key], err_msg="second call: " + key)
            # what scipy receives, and the combined triple
            np.testing.assert_array_equal(m.jac(x), out["J"].reshape(2 * N, D))
            np.testing.assert_array_equal(m.fun(x), out["r"].reshape(2 * N))
            H, grad, fc = m.normal_equations(x)
            H0, g0, f0 = lsq.combine_channels([(out["A"][ch], out["g"][ch], out["f2"][ch]) for ch in (0, 1)])
            np.testing.assert_array_equal(H, H0)
            np.testing.assert_array_equal(grad, g0)
            assert fc == f0 == 0.5 * (out["f2"][0] + out["f2"][1])


@pytest.mark.parametrize("mode", M.MODES)
@pytest.mark.parametrize("N, P", SHAPES)
def test_jacobian_bits_and_normal_equations_per_channel(N, P, mode):
    _jacobian_case(N, P, mode)


@pytest.mark.parametrize("mode", M.MODES)
def test_largest_D(mode):
    """P = 24 (D = 76), N = 513: the ragged last tile at the reduction kernel's largest D."""
    _jacobian_case(513, 24, mode)


@pytest.mark.parametrize("mode", M.MODES)
def test_beyond_the_normal_equations_limit(mode):
    """P = 25: A and g are refused (UNSUPPORTED); J and r of both channels still come back, bit for bit."""
    from nmrfit_amd.equations import NmrfitError
    N = 513
    sp = _spectrum(N, 25)
    s = 1.0 / np.sqrt(N)
    with _evaluator(sp) as ev:
        m = lsq.ResidualModel(ev, sp["lower"], sp["upper"], fit_im=MODE_ARG[mode])
        x = _interior(sp)
        rows, h = m.rows(x)
        R_re, R_im, _ = ev.residual_batch_im(rows, MODE_ARG[mode])
        out = ev.jacobian_im(rows, s / h, s, MODE_ARG[mode], J=True, r=True)
        for ch, R in enumerate((R_re, R_im)):
            np.testing.assert_array_equal(out["J"][ch], np.ascontiguousarray(((R[1:] - R[0]) * (s / h[:, None])).T))
            np.testing.assert_array_equal(out["r"][ch], R[0] * s)
        with pytest.raises(NmrfitError) as ei:
            m.normal_equations(x)
        assert ei.value.code == _cabi.E_UNSUPPORTED and "D = 4 + 3 P <= 76" in str(ei.value)
        np.testing.assert_array_equal(m.jac(x), out["J"].reshape(2 * N, -1))     # usable after the refusal


RAGGED = [(512, 1), (1537, 3), (N_MULTI, 2)]


@pytest.fixture(scope="module")
def ragged():
    """Three fits of different N and P, their points (one on its upper bound), and per mode each fit's per-channel normal
    equations on a lone context."""
    specs = [_spectrum(N, P) for N, P in RAGGED]
    X = [_interior(sp, seed=11 + k) for k, sp in enumerate(specs)]
    X[1] = np.array(specs[1]["upper"], dtype=float)
    lone = {}
    for mode in M.MODES:
        lone[mode] = []
        for sp, x in zip(specs, X):
            with _evaluator(sp) as ev:
                rows, h = lsq.forward_rows(x, sp["lower"], sp["upper"])
                s = 1.0 / np.sqrt(len(sp["w"]))
                lone[mode].append(ev.jacobian_im(rows, s / h, s, MODE_ARG[mode], normal=True))
    return specs, X, lone


def _batch(specs, order, mode, **kw):
    from nmrfit_amd.batch import FitBatch
    return FitBatch([S.spectrum_tuple(specs[k]) for k in order], [specs[k]["lower"] for k in order],
                    [specs[k]["upper"] for k in order], swarmsize=8, seeds=list(range(1, len(order) + 1)),
                    fit_im=MODE_ARG[mode] if mode else False, **kw)


def _raw_batch_call(fb, X):
    """nmrfit_batch_normal_equations_im itself: per fit (A [2, D, D], g [2, D], f2 [2])."""
    rows, cs = [], []
    s = 1.0 / np.sqrt(fb.Ns.astype(np.float64))
    for k, x in enumerate(X):
        r, h = lsq.forward_rows(_cabi.f64(x), fb.lowers[k], fb.uppers[k])
        rows.append(r.ravel())
        cs.append(s[k] / h)
    rows, cs = np.concatenate(rows), np.concatenate(cs)
    D = np.asarray(fb.D, dtype=np.int64)
    aoff = np.concatenate(([0], np.cumsum(D * D)))
    A, g, f2 = np.empty(2 * int(aoff[-1])), np.empty(2 * int(fb.offsets[-1])), np.empty(2 * fb.K)
    _cabi.check(_cabi.lib().nmrfit_batch_normal_equations_im(fb._h, _cabi.ptr(rows), _cabi.ptr(cs), _cabi.ptr(s), _cabi.ptr(A),
                                                             _cabi.ptr(g), _cabi.ptr(f2)))
    return [(A[2 * aoff[k]:2 * aoff[k + 1]].reshape(2, D[k], D[k]), g[2 * fb.offsets[k]:2 * fb.offsets[k + 1]].reshape(2, D[k]),
             f2[2 * k:2 * k + 2]) for k in range(fb.K)]


@pytest.mark.parametrize("mode", M.MODES)
@pytest.mark.parametrize("order", [(0,), (0, 1, 2), (0, 2, 1), (0, 1, 2, 0, 1, 2, 1)])
def test_batch_equals_lone_contexts_bit_for_bit(ragged, order, mode, monkeypatch):
    """K = 1 and K = 3, ragged in N and P.  Under a workspace budget of 1 MiB the order (0, 2, 1) makes every fit a group of
    its own (fit 2's doubled rows alone exceed it; fits 0 and 1 are not neighbours), the order (0, 1, 2) groups fits 0
    and 1: not a bit changes either way.  The swarms are untouched by the calls.  K = 7 is two parts of 3 + 4 (a batch
    splits from K = 6): the call walks per-part offsets into every array, doubled for the two channels; the part boundary
    lies between fits that differ in N and P, and the fits recur, so that a wrong offset lands on another fit's block."""
    specs, X, lone = ragged
    with _batch(specs, order, mode) as fb:
        fb.run(3, 1)
        before = fb.best()
        for budget in (None, "1"):
            if budget:
                monkeypatch.setenv("NMRFIT_LSQ_WORKSPACE_MB", budget)
            for (A, g, f2), k in zip(_raw_batch_call(fb, [X[k] for k in order]), order):
                np.testing.assert_array_equal(A, lone[mode][k]["A"], err_msg="A of fit %d" % k)
                np.testing.assert_array_equal(g, lone[mode][k]["g"], err_msg="g of fit %d" % k)
                np.testing.assert_array_equal(f2, lone[mode][k]["f2"], err_msg="f2 of fit %d" % k)
            for (H, grad, f), k in zip(fb.normal_equations([X[k] for k in order], channels="both"), order):
                q = lone[mode][k]
                H0, g0, f0 = lsq.combine_channels([(q["A"][ch], q["g"][ch], q["f2"][ch]) for ch in (0, 1)])
                np.testing.assert_array_equal(H, H0)
                np.testing.assert_array_equal(grad, g0)
                assert f == f0
        after = fb.best()
        for (xa, fa), (xb, fb_) in zip(before, after):
            np.testing.assert_array_equal(xa, xb)
            assert fa == fb_


@pytest.fixture(scope="module")
def five():
    return [synth.make_spectrum(2048, 2 + k % 2, seed=30 + k, physical=True) for k in range(5)]


@pytest.mark.parametrize("mode", M.MODES)
def test_batch_polish_on_both_channels(five, mode):
    """From the batch's own swarm result: the lock-step polish on both channels never ends above its start, ends within the
    CPU-measured bar (lsq_im_support.FINAL_F_BAR_IM) of the host loop -- lsq.lm_polish over lsq.rows_provider_im on the
    closed-form residual of tests/lsq_im_support.py, same start, same settings -- and no higher, beyond the same bar, than
    the real-only polish (lsq.polish(..., fit_im=mode)) in the objective both are judged by."""
    from nmrfit_amd.batch import FitBatch
    specs = five
    with FitBatch([S.spectrum_tuple(sp) for sp in specs], [sp["lower"] for sp in specs], [sp["upper"] for sp in specs],
                  swarmsize=64, seeds=[3 + k for k in range(5)], fit_im=MODE_ARG[mode]) as fb:
        fb.run(100, 10)
        start = fb.best()
        budget = 100 * max(fb.D)
        res = fb.polish(max_launches=budget, channels="both")
        info = fb.last_polish
        assert fb.polish(which=[], channels="both")[0][1] == start[0][1]
    bar = M.FINAL_F_BAR_IM
    for k, (sp, (xs, fs), (x, f)) in enumerate(zip(specs, start, res)):
        hist = info["history"][k]
        assert all(b <= a for a, b in zip(hist, hist[1:]))
        assert f <= fs, (k, f, fs)
        assert np.all(x >= sp["lower"]) and np.all(x <= sp["upper"])
        assert f == pytest.approx(M.objective(x, sp, mode), rel=1e-9)
        Xh, fh, ih = lsq.lm_polish(M.host_provider([sp], mode), [xs], [sp["lower"]], [sp["upper"]], max_launches=budget)
        with _evaluator(sp) as ev:
            xp, fp, _ = lsq.polish(ev, xs, sp["lower"], sp["upper"], fit_im=MODE_ARG[mode], **S.TRF_TOL)
            fdev = float(ev.objective_batch(x, fit_im=MODE_ARG[mode])[0])
        gap = abs(f - fh[0]) / fh[0]
        print("mode %d fit %d: swarm %.9g  both channels %.17g (%s, %d accepted)  host loop %.17g (gap %.3g)  real-only polish %.17g"
              "  objective_batch at x %.17g" % (mode, k, fs, f, info["stop"][k], info["accepted"][k], fh[0], gap, fp, fdev))
        assert gap <= bar, (k, gap, bar)
        assert f <= fp * (1 + bar), (k, f, fp)


@pytest.mark.parametrize("fit_im", [True, "sum"])
def test_fit_many_batch_polish_both(five, fit_im):
    import nmrfit_amd
    specs = five + [synth.make_spectrum(2048, 2, seed=36, physical=True)]

    def jobs(polish=True):
        out = []
        for k, sp in enumerate(specs):
            out.append(dict(data=synth.SynthData(sp["w"], sp["u"], sp["v"], sp["peaks"]), lower=list(sp["lower"]),
                            upper=list(sp["upper"]), fit_im=fit_im,
                            options={"swarmsize": 64, "maxiter": 100, "seed": 3 + k, "polish": polish and k not in (1, 4)}))
        return out
    plain = nmrfit_amd.fit_many(jobs(polish=False), generate=True)
    base = nmrfit_amd.fit_many(jobs(), generate=True, threads=2)
    flag = nmrfit_amd.fit_many(jobs(), generate=True, threads=2, batch_polish=True)
    both = nmrfit_amd.fit_many(jobs(), generate=True, threads=2, batch_polish="both")
    for k, (a, b, t, c) in enumerate(zip(plain, base, flag, both)):
        # batch_polish=True leaves fit_im jobs to the per-fit path: bit for bit the unflagged call
        np.testing.assert_array_equal(t.params, b.params)
        assert t.error == b.error
        np.testing.assert_array_equal(t.V, b.V)
        np.testing.assert_array_equal(t.imag_contribs, b.imag_contribs)
        if k in (1, 4):                        # no options['polish']: "both" changes nothing either
            np.testing.assert_array_equal(c.params, b.params)
            assert c.error == b.error
            np.testing.assert_array_equal(c.V, b.V)
            np.testing.assert_array_equal(c.I, b.I)
            np.testing.assert_array_equal(c.real_contribs, b.real_contribs)
            np.testing.assert_array_equal(c.imag_contribs, b.imag_contribs)
            continue
        print("fit_im %r job %d: swarm %.12g  per-fit polish %.12g  both channels %.12g" % (fit_im, k, a.error, b.error, c.error))
        assert c.error <= a.error, (k, c.error, a.error)
        assert np.all(c.params >= c.lower) and np.all(c.params <= c.upper)
        lone = nmrfit_amd.utils.FitUtility(jobs()[k]["data"], jobs()[k]["lower"], jobs()[k]["upper"], fit_im=fit_im, summary=False)
        lone.params = np.array(c.params)
        lone.generate_result()
        for name in ("V", "I", "u", "v", "real_contribs", "imag_contribs"):
            np.testing.assert_array_equal(getattr(c, name), getattr(lone, name), err_msg=name)


def test_refusals(ragged):
    """Every refusal of the three entry points with its code and message, and a normal call after each group.  (The
    NMRFIT_E_STATE of a reconstruction in flight cannot be reached from a test: the reconstruction begins and ends inside
    one call of the library -- as for nmrfit_batch_normal_equations.)"""
    specs, X, lone = ragged
    L = _cabi.lib()
    sp, x = specs[0], X[0]
    D, N = len(x), len(sp["w"])
    s = 1.0 / np.sqrt(N)
    with _evaluator(sp) as ev:
        rows, h = lsq.forward_rows(x, sp["lower"], sp["upper"])
        c = s / h
        A = np.empty((2, D, D))
        R = np.empty((2, D + 1, N))
        pr, pc, pA, pR = _cabi.ptr(rows), _cabi.ptr(c), _cabi.ptr(A), _cabi.ptr(R)
        for args, code, text in (((ev.handle, 1, None, pc, s, 1), _cabi.E_INVALID, b"null rows or c"),
                                 ((ev.handle, 1, pr, None, s, 1), _cabi.E_INVALID, b"null rows or c"),
                                 ((ev.handle, -1, pr, pc, s, 1), _cabi.E_INVALID, b"negative"),
                                 ((ev.handle, 1 << 20, pr, pc, s, 2), _cabi.E_INVALID, b"exceeds the supported maximum"),
                                 ((ev.handle, 1, pr, pc, s, 0), _cabi.E_INVALID, b"fit_im must be 1"),
                                 ((ev.handle, 1, pr, pc, s, 3), _cabi.E_INVALID, b"fit_im must be 1")):
            assert L.nmrfit_jacobian_im(*args, None, None, pA, None, None) == code, args
            assert text in L.nmrfit_last_error()
        for args, text in (((ev.handle, D + 1, 1, pr, 0, pR), b"fit_im must be 1"), ((ev.handle, D + 1, 1, pr, 3, pR), b"fit_im must be 1"),
                           ((ev.handle, D + 1, 1, None, 1, pR), b"null parameter/output pointer"),
                           ((ev.handle, D + 1, 1, pr, 1, None), b"null parameter/output pointer"),
                           ((ev.handle, D + 1, -1, pr, 1, pR), b"negative"), ((ev.handle, -1, 1, pr, 1, pR), b"negative")):
            assert L.nmrfit_residual_batch_im(*args, None) == _cabi.E_INVALID, args
            assert text in L.nmrfit_last_error()
        # the rows of both channels exist in the DEFAULT kernel alone
        ev.set_variant(_cabi.VARIANT_FARFIELD)
        assert L.nmrfit_jacobian_im(ev.handle, 1, pr, pc, s, 1, None, None, pA, None, None) == _cabi.E_UNSUPPORTED
        assert b"DEFAULT kernel variant only" in L.nmrfit_last_error()
        ev.set_variant(_cabi.VARIANT_DEFAULT)
        out = ev.jacobian_im(rows, c, s, True, normal=True)                # after the refused calls a normal one succeeds
        np.testing.assert_array_equal(out["A"], lone[1][0]["A"])
    with _batch(specs, (0, 1, 2), 1) as fb:
        good = fb.normal_equations(X, channels="both")
        rows = np.concatenate([lsq.forward_rows(x, q["lower"], q["upper"])[0].ravel() for x, q in zip(X, specs)])
        cs = np.ones(int(fb.offsets[-1]))
        ss = np.ones(3)
        f2 = np.empty(6)
        for args in ((None, _cabi.ptr(cs), _cabi.ptr(ss)), (_cabi.ptr(rows), None, _cabi.ptr(ss)), (_cabi.ptr(rows), _cabi.ptr(cs), None)):
            assert L.nmrfit_batch_normal_equations_im(fb._h, *args, None, None, _cabi.ptr(f2)) == _cabi.E_INVALID
            assert b"null rows, c or s" in L.nmrfit_last_error()
        with pytest.raises(ValueError):
            fb.normal_equations(X[:2], channels="both")
        with pytest.raises(ValueError):
            fb.normal_equations(X, channels="imaginary")
        for (H, g, fk), (H0, g0, f0) in zip(fb.normal_equations(X, channels="both"), good):
            np.testing.assert_array_equal(H, H0)
            assert fk == f0
    # a batch created with fit_im = 0 has no imaginary channel to refine
    with _batch(specs, (0, 1, 2), 0) as fb:
        with pytest.raises(_cabi.NmrfitError) as ei:
            fb.normal_equations(X, channels="both")
        assert ei.value.code == _cabi.E_INVALID and "fit_im = 0" in str(ei.value)
        assert len(fb.normal_equations(X)) == 3                             # the batch is usable: the real channel's call
        fb.run(3, 1)
        assert len(fb.best()) == 3
    # one fit beyond D = 76 in the batch: refused, and the batch goes on fitting
    big = [specs[0], _spectrum(513, 25)]
    with _batch(big, (0, 1), 2) as fb:
        with pytest.raises(_cabi.NmrfitError) as ei:
            fb.normal_equations([X[0], _interior(big[1])], channels="both")
        assert ei.value.code == _cabi.E_UNSUPPORTED
        fb.run(3, 1)
        assert len(fb.best()) == 2

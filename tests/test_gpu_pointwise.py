"""
GPU tier: the hot path read one grid point at a time against the high-precision truth (tests/hp_truth.py).

One-hot weights (1 at the probe point j, 0 elsewhere) turn the objective into a pointwise readout of the kernel itself:
f sqrt(N) = |dV_j| (fit_im off) or (|dV_j| + |dI_j|)/2 (fit_im True / "sum").  Unlike the parity tests on f -- an RMS
over N points, where an error at a handful of points is diluted by k/N -- every probe is held to the first-order fp64
bound of that one point.  The particles are built around the probe so that, at the probe, the peaks sit at the kernels'
switches: t = 0, the Gaussian window's edge (3.97 widths) from outside the probe's chunk, the Dawson table's quarter
intervals and its |x| = 7 and 16 boundaries, the far-field switch rho = 0.1 relative to the probe's chunk (both sides),
needles narrower than a grid step, lines wider than the span, widths below the floor, r outside [0, 1], phases to 1e3.
The swarm step and device batches are read the same way through their fx, the reconstruction point by point.

What this file covers of the objective kernel, and what it does not: the probes sit at in-chunk positions 0, 1, 63, 64,
76 and 511, i.e. rows 0, 1 and 7 of a lane's eight (a point is row * 64 + lane), in swarms of at most 25 particles (the
launch that leaves per-block sums to finalize_kernel).  The features above include a negative width and negative
amplitudes, which put every particle with 32 peaks or more, and most smaller ones, on the kernel's GENERAL forms: the
Lorentzian group form and the point-by-point Gaussian.  The two-operation pair form and the Gaussian recurrence
(objective_kernel.h fast_all / rec_all), rows 2 to 6, peak counts 0, 2 to 7 and 10 to 15, the other launch forms and
the swarm / batch boxes that reach the recurrence are held to truth in tests/test_gpu_pointwise_forms.py.  One-hot weights
reach the objective launches alone: the residual ROWS (nmrfit_residual_batch, the rows of both channels, the batch's
normal equations) are written by instantiations of their own -- a row store, no Gaussian recurrence -- and are held to
truth, at the particles built here and under weights that are not ones, in tests/test_gpu_rows_pointwise.py.

Each test prints its worst err/tol ratio.
"""
import math

import numpy as np
import pytest

from nmrfit_amd import _cabi
from nmrfit_amd.equations import Evaluator
from tests import hp_truth as hp

pytestmark = pytest.mark.gpu

KGW = 3.9686269665968861          # csrc/objective_math.h kGaussWindow (widths)
SQLN2 = math.sqrt(math.log(2.0))
MODES = (False, True, "sum")
R_SWEEP = (0.0, 0.37, 1.0, -0.2, 1.2)
PHASES = ((0.0, 0.0), (0.5, 900.0), (-1000.0, 7.0), (3.0, -640.0))


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    assert _cabi.device_count() >= 1


def make_grid(kind, N=4096 + 77, seed=11):
    rng = np.random.default_rng(seed)
    s = np.linspace(0.0, 1.0, N)
    if kind == "uniform":
        w = 3.0 + s
    elif kind == "descending":
        w = 4.0 - s
    elif kind == "nonuniform":
        w = 3.0 + s + 0.35 * s * s
    elif kind == "unsorted":
        w = rng.permutation(3.0 + s)
    elif kind == "c3":
        w = np.linspace(3.0, 4.0, 65536)
    else:
        raise ValueError(kind)
    u, v = rng.standard_normal(w.size), rng.standard_normal(w.size)
    return w, u, v


def probe_points(N):
    bl = hp.block_len(N)
    js = {0, 1, 63, 64, 511, 512, N - 1}
    for b in range(0, N, bl):
        js.update((b, min(b + bl, N) - 1))
    if N % hp.CHUNK:
        js.add(N - N % hp.CHUNK)
    return sorted(j for j in js if 0 <= j < N)


def chunk_of(w, j):
    c = j // hp.CHUNK
    seg = w[c * hp.CHUNK:(c + 1) * hp.CHUNK]
    return float(seg.min()), float(seg.max())


def features(w, j):
    """Peaks (width, loc, amplitude, kind) placed relative to probe j: each sits at one of the kernels' switches."""
    N = w.size
    span = float(w.max() - w.min())
    h = span / (N - 1)
    wj = float(w[j])
    lo, hi = chunk_of(w, j)
    # the side of the probe that lies outside its chunk (a peak there leaves the chunk's window from the probe on)
    sgn = -1.0 if wj == lo else 1.0 if wj == hi else (-1.0 if j % 2 else 1.0)
    out = []
    W = 10 * h
    out.append((W, wj, 1.0, "any"))                                          # t = 0
    for f in (1 - 1e-6, 1 + 1e-6, 3.5 / KGW, 3.0 / KGW):                    # the Gaussian window's edge
        out.append((8 * h, wj + sgn * f * KGW * 8 * h, 1.3, "gauss"))
        out.append((8 * h, wj - sgn * f * KGW * 8 * h, 0.7, "gauss"))
    for x in (7.0, 16.0):                                                   # Dawson: table / asymptotic, far-field form
        for f in (1 - 1e-9, 1 + 1e-9):
            out.append((W, wj - sgn * f * x / SQLN2 * W / 2, 0.9, "gauss"))
    for m in (1, 5, 27, 63):                                                # quarter-interval boundaries
        out.append((W, wj + sgn * (0.25 * m + 1e-12) / SQLN2 * W / 2, 1.1, "gauss"))
    if hi > lo:                                                              # the far-field switch, rho = |hk|/sqrt(1+tc^2)
        Wf = (hi - lo) / 4.0
        hk = 4.0
        for rho in (0.09, 0.1 * (1 - 1e-7), 0.1 * (1 + 1e-7), 0.11, 0.18):
            tc = math.sqrt(hk * hk / (rho * rho) - 1.0)
            out.append((Wf, 0.5 * (lo + hi) + sgn * tc * Wf / 2, 1.0, "lor"))
    out.append((0.01 * h, wj + sgn * 0.3 * h, 1.0, "any"))                   # needles narrower than a step
    out.append((0.01 * h, wj - 3.3 * h, 0.8, "any"))
    out.append((10.0 * span, wj + 0.2 * span, 1.0, "any"))                   # wider than the span
    out.append((1e-21 * span, wj - sgn * 5 * h, 1.0, "any"))                 # below the width floor
    out.append((-20 * h, wj + 2 * h, 0.6, "any"))                            # a negative width
    return out


def fillers(w, n, seed):
    rng = np.random.default_rng(seed)
    span = float(w.max() - w.min())
    h = span / (w.size - 1)
    return [(h * 10 ** rng.uniform(0.5, 2.0), rng.uniform(w.min() - 0.1 * span, w.max() + 0.1 * span),
             rng.uniform(-0.5, 1.0), "any") for _ in range(n)]


def particles(w, j, with_large=True):
    """{P: X[S, 4 + 3P]} built around probe j."""
    feats = features(w, j)
    rng = np.random.default_rng(j)
    out = {}

    def row(peaks, i):
        kinds = {k for *_, k in peaks}
        r = R_SWEEP[i % len(R_SWEEP)]
        if kinds == {"lor"}:
            r = (1.0, 1.2, 0.37)[i % 3]
        elif kinds == {"gauss"}:
            r = (0.0, 0.37, -0.2)[i % 3]
        p0, p1 = PHASES[i % len(PHASES)]
        return np.concatenate([[p0, p1, r, rng.uniform(-1e-3, 1e-3)], np.ravel([p[:3] for p in peaks])])
    out[1] = np.stack([row([f], i) for i, f in enumerate(feats)])
    for P in (8, 9):
        groups = [feats[i:i + P] for i in range(0, len(feats), P)]
        groups[-1] = groups[-1] + fillers(w, P - len(groups[-1]), j + P)
        out[P] = np.stack([row(g, i) for i, g in enumerate(groups)])
    for P in ((32, 33, 65, 130) if with_large else (32, 33)):
        peaks = (feats + fillers(w, max(P - len(feats), 0), j + P))[:P]
        out[P] = np.stack([row(peaks, i) for i in range(2)])
    return out


def variants_modes():
    for var in _cabi.available_variants():
        for mode in MODES:
            yield var, mode


REC_VARIANTS = (_cabi.VARIANT_DEFAULT, _cabi.VARIANT_FARFIELD, _cabi.VARIANT_FARFIELD32)   # objective_kernel.h kRec


def check_objective(ev, X, w, u, v, j, worst, chunk, rec=None):
    """``rec``: None, or (lane_step, grid_dev, mask) for a probe in a FULL chunk of a uniform grid -- particle s, where
    mask[s] says that the Gaussian recurrence runs for it, is held to the bound with the recurrence's term by the
    variants that have the recurrence, and to the plain bound by every other variant."""
    N = w.size
    truths = [hp.point(x, w, u, v, j, chunk=chunk, rec=rec[:2] if rec is not None and rec[2][s] else None)
              for s, x in enumerate(X)]
    for var, mode in variants_modes():
        ev.set_variant(var)
        try:
            f = ev.objective_batch(X, fit_im=mode)
        except _cabi.NmrfitError as e:
            if "error %d" % _cabi.E_UNSUPPORTED in str(e):   # (FARFIELD32: no imaginary channel)
                continue
            raise
        for s, t in enumerate(truths):
            want, tol = hp.objective_probe(t if var in REC_VARIANTS else hp.plain_bounds(t), mode)
            if var == _cabi.VARIANT_FARFIELD32:
                tol += t["far32"]
            worst.check(f[s] * math.sqrt(N), want, tol, (var, mode, j, X.shape[1], s))


@pytest.mark.parametrize("kind", ["uniform", "descending", "nonuniform", "unsorted", "c3"])
def test_objective_pointwise(kind):
    w, u, v = make_grid(kind)
    N = w.size
    worst = hp.Worst("objective/%s" % kind)
    js = probe_points(N)
    with Evaluator(w, u, v, np.ones(N)) as ev:
        for n, j in enumerate(js):
            wt = np.zeros(N)
            wt[j] = 1.0
            ev.set_weights(wt)
            w0, _ = hp.grid_frame(w)
            lo, hi = chunk_of(w, j)
            for P, X in particles(w, j, with_large=(n % 4 == 0)).items():
                check_objective(ev, X, w, u, v, j, worst, (lo - w0, hi - w0))
    fails = worst.report()
    assert not fails, fails[:5]


def test_needle_below_width_floor():
    """A width below the floor (2e-18 of the span) is the line of the floor width in BOTH channels: its dispersion tail
    a/(pi (w - loc)) is exact, whatever the width (up to round 6 the imaginary line was scaled by (2/width)/cap: 200x
    here).  Through contributions, generate_result and the objective's imaginary channel."""
    N = 1024
    w = np.linspace(0.0, 1.0, N)
    rng = np.random.default_rng(3)
    u, v = rng.standard_normal(N), rng.standard_normal(N)
    w0, wspan = hp.grid_frame(w)
    for width in (1e-20, -3e-25, 1e-300):
        x = np.array([0.0, 0.0, 1.0, 0.0, width, 0.5 + 1e-7, 1.0])
        assert hp.capped(width, x[5], w0, wspan)
        with Evaluator(w, u, v, np.ones(N)) as ev:
            real, imag = ev.contributions(x)
            for j in (0, 100, 511, 513, 900, N - 1):
                dw = w[j] - x[5]
                assert imag[0, j] == pytest.approx(1.0 / (math.pi * dw), rel=1e-12), (width, j)
                t = hp.point(x, w, u, v, j)
                assert abs(real[0, j] - t["real"][0]) <= t["tol_real"][0], (width, j)
                assert abs(imag[0, j] - t["imag"][0]) <= t["tol_imag"][0], (width, j)
                wt = np.zeros(N)
                wt[j] = 1.0
                ev.set_weights(wt)
                for mode in (True, "sum"):
                    want, tol = hp.objective_probe(t, mode)
                    assert abs(ev.objective_batch(x, fit_im=mode)[0] * math.sqrt(N) - want) <= tol, (width, j, mode)


# ---- the swarm step and the device batch ----------------------------------------------------------------------------

def hostile_box(w, P, kind, seed):
    """Bounds that land particles in one hostile regime: needles, wide lines, lines beyond the grid, r outside [0, 1]."""
    rng = np.random.default_rng(seed)
    span = float(w.max() - w.min())
    h = span / (w.size - 1)
    lo = [-2.0, -900.0, -0.3, -1e-3]
    up = [2.0, 900.0, 1.3, 1e-3]
    for k in range(P):
        c = rng.uniform(w.min(), w.max())
        if kind == "needle":
            lo += [1e-3 * h, c - 2 * h, 0.5]
            up += [0.3 * h, c + 2 * h, 1.5]
        elif kind == "wide":
            lo += [0.5 * span, c - 0.1, 0.5]
            up += [20 * span, c + 0.1, 1.5]
        elif kind == "beyond":
            lo += [5 * h, w.max() + 0.01 * span, 0.5]
            up += [50 * h, w.max() + 0.5 * span, 1.5]
        elif kind in ("fine", "fine_neg"):     # lines the Gaussian recurrence takes (|d| <= 128/90), 0 < r < 1
            neg = kind == "fine_neg" and k == P // 2
            lo += [90 * h, c - 0.05, -1.5 if neg else 0.5]
            up += [300 * h, c + 0.05, -0.5 if neg else 1.5]
        else:
            lo += [2 * h, c - 0.05, 0.5]
            up += [40 * h, c + 0.05, 1.5]
    if kind in ("fine", "fine_neg"):           # "fine": the pair form; "fine_neg": one amplitude negative, the general form
        lo[2], up[2] = 0.2, 0.9
    return np.array(lo), np.array(up)


def check_state(x, fx, w, u, v, j, mode, worst, tag, n=24, rec=None, forms=None):
    """``rec``: None, or (lane_step, grid_dev) when j lies in a full chunk and the kernel variant has the Gaussian
    recurrence: a sampled row for which the mirror says it runs takes the recurrence's term.  ``forms``: the (pair form,
    recurrence) class every sampled row must be in, by the mirror."""
    N = w.size
    idx = np.unique(np.linspace(0, x.shape[0] - 1, min(n, x.shape[0])).astype(int))
    for s in idx:
        if rec is not None or forms is not None:
            kf = hp.kernel_forms(x[s], w)
            if forms is not None:
                assert (kf["fast"], kf["rec"]) == tuple(forms), (tag, int(s), kf)
        t = hp.point(x[s], w, u, v, j, rec=rec if rec is not None and kf["rec"] else None)
        want, tol = hp.objective_probe(t, mode)
        worst.check(fx[s] * math.sqrt(N), want, tol, tag + (int(s),))


@pytest.mark.parametrize("S", [204, 4099])
def test_swarm_step_pointwise(S):
    from nmrfit_amd.pso import DeviceSwarm
    w, u, v = make_grid("uniform")
    N = w.size
    worst = hp.Worst("swarm S=%d" % S)
    for i, (kind, P, mode, var) in enumerate((("needle", 3, False, _cabi.VARIANT_DEFAULT),
                                              ("wide", 8, "sum", _cabi.VARIANT_FARFIELD),
                                              ("beyond", 9, True, _cabi.VARIANT_DEFAULT),
                                              ("normal", 33, False, _cabi.VARIANT_FARFIELD))):
        j = (0, 511, 2048, N - 1)[i]
        wt = np.zeros(N)
        wt[j] = 1.0
        lo, up = hostile_box(w, P, kind, seed=i)
        with Evaluator(w, u, v, wt) as ev:
            ev.set_variant(var)
            ev.set_fit_im(mode)
            sw = DeviceSwarm(ev, lo, up, swarmsize=S, seed=17 + i)
            sw.run(maxiter=2, check_every=1)
            st = sw.state()
            sw.close()
        check_state(st["x"], st["fx"], w, u, v, j, mode, worst, (kind, P, str(mode), var))
    fails = worst.report()
    assert not fails, fails[:5]


@pytest.mark.parametrize("ragged", [False, True])
@pytest.mark.parametrize("mode", MODES)
def test_device_batch_pointwise(ragged, mode):
    from nmrfit_amd.batch import FitBatch
    worst = hp.Worst("batch ragged=%s fit_im=%s" % (ragged, mode))
    for variant in ("default", "farfield"):
        specs, lows, ups, probes = [], [], [], []
        for k, (kind, P) in enumerate((("needle", 2), ("wide", 7), ("beyond", 12), ("normal", 5))):
            w, u, v = make_grid("uniform" if k % 2 == 0 else "nonuniform", N=(1500 + 613 * k) if ragged else 3000, seed=k)
            j = (7, 512, 1499, 64)[k]
            wt = np.zeros(w.size)
            wt[j] = 1.0
            lo, up = hostile_box(w, P, kind, seed=40 + k)
            specs.append((w, u, v, wt))
            lows.append(lo)
            ups.append(up)
            probes.append(j)
        with FitBatch(specs, lows, ups, swarmsize=96, seeds=[1, 2, 3, 4], variant=variant, fit_im=mode) as b:
            b.run(2, 1)
            states = [b.state(k) for k in range(len(specs))]
        for k, st in enumerate(states):
            w, u, v, _ = specs[k]
            check_state(st["x"], st["fx"], w, u, v, probes[k], mode, worst, (variant, k), n=12)
    fails = worst.report()
    assert not fails, fails[:5]


# ---- the reconstruction -----------------------------------------------------------------------------------------------

def recon_x(w, P, seed):
    rng = np.random.default_rng(seed)
    span = float(w.max() - w.min())
    h = span / (w.size - 1)
    x = [rng.uniform(-1000, 1000), rng.uniform(-1000, 1000), rng.choice(R_SWEEP), rng.uniform(-1e-3, 1e-3)]
    for k in range(P):
        c = k % 4
        width = (0.01 * h, 10 * h, 5 * span, 1e-21 * span)[c] if k % 7 else 30 * h
        x += [width, rng.uniform(w.min() - 0.2 * span, w.max() + 0.2 * span), rng.uniform(-0.5, 1.5)]
    return np.array(x)


def check_recon(worst, tag, x, w, u, v, wout, real, imag, fit, data, js_out, js_data, w0, wspan):
    Nout = wout.size
    for j in js_out:
        t = hp.point(x, wout, np.zeros(Nout), np.zeros(Nout), j, w0=w0, wspan=wspan, n_steps=0)
        for k in range(real.shape[0]):
            worst.check(real[k, j], t["real"][k], t["tol_real"][k], tag + ("real", k, j))
            worst.check(imag[k, j], t["imag"][k], t["tol_imag"][k], tag + ("imag", k, j))
        if fit is not None:
            worst.check(fit[0][j], t["Vf"], t["tol_Vf"], tag + ("V", j))
            worst.check(fit[1][j], t["If2"], t["tol_If"], tag + ("I", j))
            # u_fit + i v_fit = (V + i I) exp(-i phi_j), phi_j over the output grid's index
            phi = hp.mp.mpf(x[0]) + hp.mp.mpf(x[1]) * j / Nout
            cs, sn = hp.mp.cos(phi), hp.mp.sin(phi)
            Vf, If = hp.mp.mpf(t["Vf"]), hp.mp.mpf(t["If2"])
            tol = t["tol_Vf"] + t["tol_If"] + hp.C * hp.EPS * (abs(t["Vf"]) + abs(t["If2"])) * (1 + abs(float(phi)))
            worst.check(fit[2][j], float(cs * Vf + sn * If), tol, tag + ("u_fit", j))
            worst.check(fit[3][j], float(cs * If - sn * Vf), tol, tag + ("v_fit", j))
    if data is not None:
        for j in js_data:
            t = hp.point(x[:4], w, u, v, j, w0=w0, wspan=wspan, n_steps=0, imag=False)
            tol = hp.C * hp.EPS * (abs(u[j]) + abs(v[j])) * (1 + abs(x[0]) + abs(x[1]))
            worst.check(data[0][j], t["V"], tol, tag + ("data_V", j))
            worst.check(data[1][j], t["I"], tol, tag + ("data_I", j))


def sample_points(n, m=200, seed=0):
    rng = np.random.default_rng(seed)
    js = {0, n - 1, min(255, n - 1), min(256, n - 1)}
    js.update(rng.integers(0, n, m - len(js)).tolist())
    return sorted(js)


@pytest.mark.parametrize("kind", ["uniform", "descending", "nonuniform", "unsorted"])
def test_reconstruction_pointwise(kind):
    w, u, v = make_grid(kind, N=1500)
    N = w.size
    w0, wspan = hp.grid_frame(w)
    worst = hp.Worst("reconstruction/%s" % kind)
    with Evaluator(w, u, v, np.ones(N)) as ev:
        for P, scale in ((0, 1.5), (1, 2.5), (255, 1.5), (256, 1.0), (257, 2.5), (600, 1.0)):
            x = recon_x(w, P, seed=P + 3)
            m = min(200, max(8, 6000 // max(P, 1)))             # (about 6000 (point, peak) truths per case)
            wout = np.linspace(w.min(), w.max(), int(scale * N))
            for grid in (None, wout):
                g = w if grid is None else grid
                real, imag = ev.contributions(x, grid)
                r2, i2, fit, data = ev.generate_result(x, grid)
                np.testing.assert_array_equal(real, r2)
                np.testing.assert_array_equal(imag, i2)
                check_recon(worst, (P, scale, grid is None), x, w, u, v, g, real, imag, fit, data,
                            sample_points(g.size, m, seed=P), sample_points(N, 40, seed=P + 1), w0, wspan)
    fails = worst.report()
    assert not fails, fails[:5]


def test_batch_generate_pointwise():
    from nmrfit_amd.batch import FitBatch
    worst = hp.Worst("FitBatch.generate")
    specs, lows, ups = [], [], []
    for k, (kind, P) in enumerate((("needle", 3), ("wide", 6), ("beyond", 1), ("normal", 9))):
        w, u, v = make_grid(("uniform", "descending", "nonuniform", "unsorted")[k], N=900 + 301 * k, seed=k + 5)
        lo, up = hostile_box(w, P, kind, seed=60 + k)
        specs.append((w, u, v, np.ones(w.size)))
        lows.append(lo)
        ups.append(up)
    with FitBatch(specs, lows, ups, swarmsize=64, seeds=[5, 6, 7, 8], fit_im="sum") as b:
        b.run(2, 1)
        best = b.best()
        outs = [b.generate(), b.generate(scale=1.5)]
    for out in outs:
        for k, (r, (x, _)) in enumerate(zip(out, best)):
            w, u, v, _ = specs[k]
            w0, wspan = hp.grid_frame(w)
            g = w if r["w"] is None else r["w"]
            fit = (r["V"], r["I"], r["u"], r["v"])
            check_recon(worst, ("batch", k, r["w"] is None), x, w, u, v, g, r["real"], r["imag"], fit,
                        (r["data_V"], r["data_I"]), sample_points(g.size, 60, seed=k), sample_points(w.size, 30), w0, wspan)
    fails = worst.report()
    assert not fails, fails[:5]

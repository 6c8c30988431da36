"""
What the tests of the polynomial baselines share (NOT part of the nmrfit_amd package): the case list, the exact truth,
and the driver of the poisoned-allocation children,

    python -m tests.baseline_support poison OUT.npz

THE TRUTH.  The least-squares polynomial of degree d over the masked points is unique whatever basis it is written in.
Here it is computed exactly: the fp64 inputs are rationals, the normal equations in powers of (w - w_first) are formed
in integers and solved in ``fractions.Fraction``; the polynomial is evaluated exactly at every w_j and rounded once.
sigma comes from the exact residuals: S2 / n is a rational, its square root is taken by mpmath at 200 bits.

THE CASE LIST.  N in {1, 63, 64, 65, 255, 256, 257, 320, 1000} x d in {0, 1, 2, 4, 8} x three masks (one interval, the
complement of two regions, the whole grid) x four grids (ascending on [3, 4], descending, shuffled with duplicates, with
a NaN in it); y with a NaN inside the mask and with one outside it; +-inf edges; exactly d + 1 masked points
(interpolation), d masked points (status 2), an empty mask (status 1), all masked w equal, R at the interval limit.
"""
import math
import os
import sys
from fractions import Fraction

import numpy as np

NS = (1, 63, 64, 65, 255, 256, 257, 320, 1000)
DEGS = (0, 1, 2, 4, 8)
MASKS = ("interval", "outside2", "whole")
GRIDS = ("ascending", "descending", "shuffled", "nan_w")
EPS = 2.0 ** -52
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the bound on the baseline's error against the exact polynomial, in units of 2^-52 max|y| over the mask: twice the worst
# error of the numpy mirror over the case list (5.06; tests/test_baseline_cpu.py prints it), rounded up
BOUND_E = 11.0


class Case:
    def __init__(self, name, w, y, deg, intervals, complement):
        self.name, self.w, self.y, self.deg = name, np.asarray(w, dtype=np.float64), np.asarray(y, dtype=np.float64), int(deg)
        self.intervals, self.complement = [tuple(map(float, iv)) for iv in intervals], bool(complement)

    def mask(self):
        from nmrfit_amd import baseline
        return baseline.mask_of(self.w, self.intervals, self.complement)

    def has_truth(self):
        """The exact polynomial exists and is unique, and every input that enters it is finite."""
        m = self.mask()
        return (len(np.unique(self.w[m])) >= self.deg + 1 and np.all(np.isfinite(self.y[m])) and np.all(np.isfinite(self.w[m])))


def _grid(kind, N, rng):
    w = np.linspace(3.0, 4.0, N) if N > 1 else np.array([3.5])
    if kind == "descending":
        w = w[::-1].copy()
    elif kind == "shuffled":
        w = w.copy()
        if N >= 8:
            w[rng.integers(0, N, N // 8)] = w[rng.integers(0, N, N // 8)]      # duplicates
        rng.shuffle(w)
    elif kind == "nan_w":
        w = w.copy()
        w[N // 2] = np.nan
    return w


def _signal(w, rng):
    """Unit noise on a roll of a few sigma: what a noise stretch and a finished fit's residual look like.  (The bound on
    sigma in tests/test_baseline_cpu.py is that of the sums' rounding alone, so the data are of the residual's own
    scale: on a pedestal of 300 sigma every fp64 evaluation of b_j carries ulp(300) per point, and the same mirror used
    1.49 of that bound.)"""
    x = np.where(np.isnan(w), 3.5, w)
    return 2.0 + 1.5 * (x - 3.4) - 6.0 * (x - 3.5) ** 2 + 0.5 * np.sin(7.0 * x) + rng.standard_normal(len(w))


def _mask_args(kind):
    if kind == "interval":
        return [(3.2, 3.9)], False
    if kind == "outside2":
        return [(3.3, 3.45), (3.7, 3.6)], True      # (the second pair reversed: swapped by the definition)
    return [], True


def cases():
    """The case list, in a fixed order (every array from a generator seeded by the case's place)."""
    from nmrfit_amd import baseline
    out = []
    for gi, grid in enumerate(GRIDS):
        for N in NS:
            for mi, mask in enumerate(MASKS):
                rng = np.random.default_rng(1000 * gi + 10 * N + mi)
                w = _grid(grid, N, rng)
                y = _signal(w, rng)
                iv, comp = _mask_args(mask)
                for d in DEGS:
                    out.append(Case("%s/N%d/%s/d%d" % (grid, N, mask, d), w, y, d, iv, comp))
    rng = np.random.default_rng(7)
    for N in (257, 1000):
        w = _grid("ascending", N, rng)
        for mask in MASKS:
            iv, comp = _mask_args(mask)
            m = baseline.mask_of(w, iv, comp)
            for d in DEGS:
                y = _signal(w, rng)
                y[np.flatnonzero(m)[len(np.flatnonzero(m)) // 3]] = np.nan
                out.append(Case("y_nan_inside/N%d/%s/d%d" % (N, mask, d), w, y, d, iv, comp))
                if not m.all():
                    y = _signal(w, rng)
                    y[np.flatnonzero(~m)[0]] = np.nan
                    out.append(Case("y_nan_outside/N%d/%s/d%d" % (N, mask, d), w, y, d, iv, comp))
    w = _grid("ascending", 320, rng)
    y = _signal(w, rng)
    for d in DEGS:
        out.append(Case("inf_edges/in/d%d" % d, w, y, d, [(-np.inf, 3.5)], False))
        out.append(Case("inf_edges/all/d%d" % d, w, y, d, [(np.inf, -np.inf)], False))
        out.append(Case("inf_edges/out/d%d" % d, w, y, d, [(3.6, np.inf)], True))
        # exactly d + 1 masked points (the polynomial interpolates), and d of them (rank)
        step = w[1] - w[0]
        out.append(Case("interpolates/d%d" % d, w, y, d, [(w[100] - step / 4, w[100 + d] + step / 4)], False))
        out.append(Case("one_short/d%d" % d, w, y, d, [(w[100] - step / 4, w[100 + d - 1] + step / 4)] if d else [(5.0, 6.0)], False))
        out.append(Case("empty/d%d" % d, w, y, d, [(5.0, 6.0)], False))
        out.append(Case("empty_complement/d%d" % d, w, y, d, [(0.0, 10.0)], True))
        ws = np.full(70, 3.25)
        ws[:3] = (3.0, 3.1, 3.9)
        out.append(Case("all_equal/d%d" % d, ws, _signal(ws, rng), d, [(3.2, 3.3)], False))
        # R at the limit: many slivers that miss every point, and one interval that holds a stretch
        slivers = [(w[k % 319] + step / 4, w[k % 319] + step / 2) for k in range(baseline.MAX_INTERVALS - 1)]
        out.append(Case("r_limit/d%d" % d, w, y, d, slivers + [(3.4, 3.8)], False))
    return out


# ---- the exact least-squares polynomial ----------------------------------------------------------------------------------

def exact_fit(case):
    """(values, sigma): the exact least-squares polynomial of the case at every w_j, rounded once (NaN where w_j is),
    and sigma = sqrt(sum_mask (r_j - rbar)^2 / n) of the exact residuals, rounded once from 200 bits."""
    import mpmath
    m = case.mask()
    d = case.deg
    idx = np.flatnonzero(m)
    w0 = Fraction(float(case.w[idx[0]]))
    xs = [Fraction(float(case.w[j])) - w0 for j in idx]
    ys = [Fraction(float(case.y[j])) for j in idx]
    sx = max(x.denominator.bit_length() - 1 for x in xs)
    X = [int(x * (1 << sx)) for x in xs]           # x = X / 2^sx
    sy = max(y.denominator.bit_length() - 1 for y in ys)
    Y = [int(y * (1 << sy)) for y in ys]
    pw = [[1] * len(X)]
    for _ in range(2 * d):
        pw.append([p * x for p, x in zip(pw[-1], X)])
    mom = [sum(p) for p in pw]                                              # sum X^k
    rhs = [sum(p * y for p, y in zip(pw[k], Y)) for k in range(d + 1)]      # sum X^k Y
    A = [[Fraction(mom[i + k]) for k in range(d + 1)] + [Fraction(rhs[i])] for i in range(d + 1)]
    for i in range(d + 1):                                                  # Gauss-Jordan in rationals
        p = next(r for r in range(i, d + 1) if A[r][i] != 0)
        A[i], A[p] = A[p], A[i]
        inv = 1 / A[i][i]
        A[i] = [v * inv for v in A[i]]
        for r in range(d + 1):
            if r != i and A[r][i] != 0:
                f = A[r][i]
                A[r] = [vr - f * vi for vr, vi in zip(A[r], A[i])]
    coef = [A[i][d + 1] for i in range(d + 1)]      # in powers of X, values scaled by 2^sy
    den = 1
    for c in coef:
        den = den * c.denominator // math.gcd(den, c.denominator)
    cint = [int(c * den) for c in coef]             # the polynomial is sum cint_k X^k / (den 2^sy)
    values = np.full(len(case.w), np.nan)
    exact = {}
    for j in range(len(case.w)):
        if np.isnan(case.w[j]) or np.isinf(case.w[j]):
            continue
        xj = (Fraction(float(case.w[j])) - w0) * (1 << sx)
        if xj.denominator == 1:
            xi = int(xj)
            acc = 0
            for c in reversed(cint):
                acc = acc * xi + c
            v = Fraction(acc, den << sy)
        else:
            acc = Fraction(0)
            for c in reversed(cint):
                acc = acc * xj + c
            v = acc / (den << sy)
        exact[j] = v
        values[j] = float(v)
    res = [Fraction(float(case.y[j])) - exact[j] for j in idx]
    n = len(res)
    mean = sum(res) / n
    var = sum((r - mean) ** 2 for r in res) / n
    with mpmath.workprec(200):
        sigma = float(mpmath.sqrt(mpmath.mpf(var.numerator) / mpmath.mpf(var.denominator)))
    return values, sigma


def domain_t(case):
    """t_j of every grid point as the definition forms it (NaN where w is), for the |t| <= 1 selection."""
    m = case.mask()
    a, b = case.w[m].min(), case.w[m].max()
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.zeros_like(case.w) if b == a else ((case.w - a) - (b - case.w)) / (b - a)


def baseline_error(case, got, truth):
    """The worst |got - truth| over the masked points and over all points with |t| <= 1, in units of
    2^-52 max|y| over the mask."""
    m = case.mask()
    with np.errstate(invalid="ignore"):
        sel = (m | (np.abs(domain_t(case)) <= 1.0)) & ~np.isnan(truth)
    unit = EPS * np.abs(case.y[m]).max()
    return float(np.abs(got[sel] - truth[sel]).max() / unit)


def polyfit_baseline(case):
    """np.polyfit on the raw w of the masked points, the method of peaks.sample_noise, evaluated at every w."""
    import warnings
    m = case.mask()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        p = np.polyfit(case.w[m], case.y[m], case.deg)
    with np.errstate(invalid="ignore"):
        return np.polyval(p, case.w)


def device_fits(case_list, device=0, return_baseline=True):
    """One ``baseline.fit_many`` call over the cases."""
    from nmrfit_amd import baseline
    return baseline.fit_many([c.w for c in case_list], [c.y for c in case_list], deg=[c.deg for c in case_list],
                             intervals=[c.intervals for c in case_list], complement=[c.complement for c in case_list],
                             device=device, return_baseline=return_baseline)


def same_bits(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def same_row(a, b):
    """Rows equal bit for bit, any NaN equal to any NaN (the payload of a NaN is not part of the definition)."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(np.all((a == b) & (np.signbit(a) == np.signbit(b)) | (np.isnan(a) & np.isnan(b))))


# ---- the poison driver -------------------------------------------------------------------------------------------------

def resident_problem(seed=3):
    """3 fits, S = 8, N in {320, 1000}, P = 2: the spectra, boxes and intervals of the resident-batch tests."""
    from nmrfit_amd import synth
    sps = [synth.make_spectrum(N, 2, seed=seed + k) for k, N in enumerate((320, 1000, 320))]
    intervals = [[tuple(p.bounds) for p in sp["peaks"]] for sp in sps]
    return sps, intervals


def make_batch(sps, seed=11):
    from nmrfit_amd.batch import FitBatch
    return FitBatch([(sp["w"], sp["u"], sp["v"], sp["weights"]) for sp in sps], [sp["lower"] for sp in sps],
                    [sp["upper"] for sp in sps], swarmsize=8, seeds=[seed + k for k in range(len(sps))], minfunc=-1.0, minstep=-1.0)


def poison_run(out):
    """Every piece of the two entry points' device blocks: the whole case list through nmrfit_baseline_fit (rows and
    baselines, one and two channels), and a resident batch through nmrfit_batch_residual_baseline at X and at the best
    positions.  Host outputs start as NaN (np.empty is filled), so a copy that came up short shows."""
    from nmrfit_amd import baseline
    from tests import poison_support
    arrays = {}
    with poison_support.nan_outputs():
        cl = cases()
        got = device_fits(cl)
        arrays["rows"] = np.array([f.row for f in got])
        arrays["baselines"] = np.concatenate([f.baseline for f in got])
        two = baseline.fit_many([c.w for c in cl[:40]], [np.array([c.y, c.y[::-1]]) for c in cl[:40]], deg=[c.deg for c in cl[:40]],
                                intervals=[c.intervals for c in cl[:40]], complement=[c.complement for c in cl[:40]])
        arrays["rows2"] = np.array([[f.row for f in pair] for pair in two])
        arrays["baselines2"] = np.concatenate([f.baseline for pair in two for f in pair])
        sps, intervals = resident_problem()
        with make_batch(sps) as fb:
            X = [0.5 * (sp["lower"] + sp["upper"]) for sp in sps]
            at_x = fb.residual_baseline(X, deg=[1, 2, 4], intervals=intervals, return_baseline=True)
            fb.run(5, 5)
            best = fb.residual_baseline(None, deg=1, intervals=intervals, return_baseline=True)
            rows_only = fb.residual_baseline(None, deg=1, intervals=intervals)
        arrays["resident_x_rows"] = np.array([f.row for f in at_x])
        arrays["resident_x_baselines"] = np.concatenate([f.baseline for f in at_x])
        arrays["resident_best_rows"] = np.array([f.row for f in best])
        arrays["resident_best_baselines"] = np.concatenate([f.baseline for f in best])
        assert all(same_row(a.row, b.row) for a, b in zip(best, rows_only))
    # a status-0 job leaves no NaN the driver put there; a refused job's NaN is the definition's
    for f in got:
        assert (f.status == 0 and np.isfinite(f.row[1:4]).all()) or f.status in (1, 2) or np.isnan(f.row[4]), f
    arrays["__poison__"] = np.array(os.environ.get("NMRFIT_POISON_ALLOC", ""))
    np.savez(out, **arrays)


if __name__ == "__main__":
    if len(sys.argv) != 3 or sys.argv[1] != "poison":
        sys.exit("usage: python -m tests.baseline_support poison OUT.npz")
    poison_run(sys.argv[2])

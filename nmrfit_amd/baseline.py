"""
Least-squares polynomial baselines and noise levels of many spectra on the device (include/nmrfit_amd_baseline.h,
csrc/baseline.hip).

The reference estimates a noise level with a quadratic fit over a signal-free stretch (``utils.sample_noise``:
``np.polyfit`` on raw ppm values) and models the baseline of a fit by one constant, ``yoff``.  Here one device primitive
fits, over a masked part of a grid, a polynomial of degree <= 8 in the Chebyshev basis of the masked points' own domain
-- well conditioned where powers of ppm values near 3.5 are not -- sums the normal equations in a fixed order and
returns the coefficients, the baseline at every grid point and the spread of what is left over the mask.  A job's
numbers are the same bits alone, in any batch and from call to call; ``fit_host`` is the numpy mirror, order and solve
included.

    fit_many(ws, ys, deg, intervals, complement)      K spectra (one or two channels each), one library call
    sample_noise_many(ws, ys, regions)                utils.sample_noise for many: degree 2, one interval, the sigmas
    fit_host(w, y, deg, intervals, complement)        the numpy mirror of one job
    FitBatch.residual_baseline(X, deg, intervals)     the baseline of data_V - V of a device batch's fits, resident
    fit_many(jobs, residual_baseline=1)               every fit carries ``fit.residual_baseline``
    correct_baseline_many(datas, deg, exclude)        subtract a fitted baseline from V, I (and u, v) of many Data
    subtract_rotated(u, v, b, p0, p1)                 u, v with a real-channel baseline b taken out at phase (p0, p1)

The documented recipe for a baseline seen in a fit's residual: ``fits = fit_many(jobs, residual_baseline=1)``, then
``u, v = subtract_rotated(d.u, d.v, fit.residual_baseline(d.w), fit.params[0], fit.params[1])`` per spectrum and a second
``fit_many`` on the corrected data.  Nothing refits by itself.
"""
import numpy as np

from . import _cabi

MAX_DEG = 8              # NMRFIT_BASELINE_MAX_DEG
ROW = 17                 # doubles per row (NMRFIT_BASELINE_ROW)
MAX_INTERVALS = 1024     # per spectrum (NMRFIT_BASELINE_MAX_INTERVALS)
TILE, WAVE = 256, 64     # the summation order's units: point j is lane j % 64 of wave (j % 256) / 64
OK, EMPTY, RANK = 0, 1, 2


def _chebyshev(t, kmax):
    """[T_0(t) .. T_kmax(t)] by T_k = (2 t) T_{k-1} - T_{k-2}, every operation rounded once."""
    T = [np.ones_like(t), t]
    t2 = 2.0 * t
    for _ in range(2, kmax + 1):
        T.append(t2 * T[-1] - T[-2])
    return T[:kmax + 1]


class BaselineFit:
    """One job's row.

    status : 0 fitted, 1 empty mask, 2 rank (fewer masked points than coefficients, or a pivot not > 0)
    n : masked points;  domain : (a, b), the smallest and largest masked w
    coef : c_0 .. c_d in the Chebyshev basis of t = ((w - a) - (b - w)) / (b - a)
    sigma : sqrt(S2 / n), the standard deviation (ddof 0) of y - baseline over the mask -- ``utils.sample_noise``'s number
    rcond : the smallest pivot of the solve over the largest (small: a thin mask for this degree)
    baseline : the polynomial at every grid point of the job, or None when it was not asked for
    row : the 17 doubles as the library returns them
    Calling the object, ``fit(w)``, evaluates the polynomial at any w by the recurrence the device uses."""

    def __init__(self, row, baseline=None):
        self.row = np.array(row, dtype=np.float64).reshape(ROW)
        self.status, self.n, self.deg = int(self.row[0]), int(self.row[1]), int(self.row[7])
        self.domain = (float(self.row[2]), float(self.row[3]))
        self.S1, self.S2, self.rcond = float(self.row[4]), float(self.row[5]), float(self.row[6])
        self.coef = self.row[8:9 + self.deg].copy()
        with np.errstate(invalid="ignore"):
            self.sigma = float(np.sqrt(self.S2 / self.n)) if self.n else float("nan")
        self.baseline = baseline

    def __call__(self, w):
        w = np.asarray(w, dtype=np.float64)
        a, b = np.float64(self.domain[0]), np.float64(self.domain[1])
        with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
            t = np.zeros_like(w) if b == a else ((w - a) - (b - w)) / (b - a)
            T = _chebyshev(t, self.deg)
            out = np.full_like(w, self.coef[0])
            for i in range(1, self.deg + 1):
                out = out + self.coef[i] * T[i]
        return out

    def __repr__(self):
        return "BaselineFit(status %d, deg %d, n %d, sigma %.6g)" % (self.status, self.deg, self.n, self.sigma)


# -- the numpy mirror --------------------------------------------------------------------------------------------

def _ordered_sums(terms):
    """The sums of the rows of ``terms`` (S, N; +0.0 already where a point does not count) in the device's order: a
    lane's running sum over the tiles in ascending order, the wave tree, the four waves in order."""
    S, n = terms.shape
    tiles = max(1, -(-n // TILE))
    a = np.zeros((S, tiles * TILE))
    a[:, :n] = terms
    a = a.reshape(S, tiles, TILE)
    run = np.zeros((S, TILE))
    for tile in range(tiles):
        run = run + a[:, tile]
    x = run.reshape(S, TILE // WAVE, WAVE)
    x = x[:, :, :32] + x[:, :, 32:]
    for half in (16, 8, 4, 2, 1):
        x = x[:, :, :half] + x[:, :, half:]
    x = x[:, :, 0]
    s = x[:, 0]
    for wv in range(1, TILE // WAVE):
        s = s + x[:, wv]
    return s


def mask_of(w, intervals, complement):
    """The definition's mask: by value, reversed edges swapped, a NaN w never in it."""
    w = np.asarray(w, dtype=np.float64)
    held = np.zeros(len(w), dtype=bool)
    with np.errstate(invalid="ignore"):
        for lo, hi in (intervals if intervals is not None else ()):
            lo, hi = (lo, hi) if lo <= hi else (hi, lo)
            held |= (lo <= w) & (w <= hi)
    return ~np.isnan(w) & (~held if complement else held)


def fit_host(w, y, deg=2, intervals=None, complement=False):
    """The numpy mirror of one job (include/nmrfit_amd_baseline.h), summation order and solve included: the
    ``BaselineFit`` the device gives for the same job, bit for bit, with ``baseline`` at every grid point."""
    w, y, d = _cabi.f64(w).ravel(), _cabi.f64(y).ravel(), int(deg)
    if not 0 <= d <= MAX_DEG:
        raise ValueError("baseline: the degree is 0 .. %d" % MAX_DEG)
    if len(w) != len(y) or len(w) == 0:
        raise ValueError("baseline: w and y have the same non-zero length")
    m = mask_of(w, intervals, complement)
    n = int(m.sum())
    nan = float("nan")
    row = np.zeros(ROW)
    row[7] = d
    row[1] = n
    if n < d + 1:
        row[0] = EMPTY if n == 0 else RANK
        row[2:4] = (w[m].min(), w[m].max()) if n else (nan, nan)
        row[4:7] = nan
        row[8:9 + d] = nan
        return BaselineFit(row, np.full(len(w), nan))
    a, b = w[m].min(), w[m].max()
    zero = np.zeros_like(w)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        t = zero.copy() if b == a else ((w - a) - (b - w)) / (b - a)
        T = _chebyshev(t, max(2 * d, 1))
        terms = [np.where(m, T[k], zero) for k in range(2 * d + 1)] + [np.where(m, T[i] * y, zero) for i in range(d + 1)]
        sums = _ordered_sums(np.array(terms))
        mu, g = sums[:2 * d + 1], sums[2 * d + 1:]
        G = np.array([[0.5 * (mu[i + k] + mu[abs(i - k)]) for k in range(d + 1)] for i in range(d + 1)])
        L, D, ok = np.zeros((d + 1, d + 1)), np.zeros(d + 1), True
        for j in range(d + 1):
            v = [L[j, k] * D[k] for k in range(j)]
            s = G[j, j]
            for k in range(j):
                s = s - L[j, k] * v[k]
            D[j] = s
            if not s > 0.0:
                ok = False
                break
            for i in range(j + 1, d + 1):
                r = G[i, j]
                for k in range(j):
                    r = r - L[i, k] * v[k]
                L[i, j] = r / s
        if not ok:
            row[0] = RANK
            row[2:4] = a, b
            row[4:7] = nan
            row[8:9 + d] = nan
            return BaselineFit(row, np.full(len(w), nan))
        z = np.zeros(d + 1)
        for i in range(d + 1):
            r = g[i]
            for k in range(i):
                r = r - L[i, k] * z[k]
            z[i] = r
        for i in range(d + 1):
            z[i] = z[i] / D[i]
        c = np.zeros(d + 1)
        for i in range(d, -1, -1):
            r = z[i]
            for k in range(i + 1, d + 1):
                r = r - L[k, i] * c[k]
            c[i] = r
        base = np.full_like(w, c[0])
        for i in range(1, d + 1):
            base = base + c[i] * T[i]
        res = y - base
        S1 = _ordered_sums(np.where(m, res, zero)[None, :])[0]
        dev = res - S1 / np.float64(n)
        S2 = _ordered_sums(np.where(m, dev * dev, zero)[None, :])[0]
    row[0], row[2], row[3], row[4], row[5], row[6] = OK, a, b, S1, S2, D.min() / D.max()
    row[8:9 + d] = c
    return BaselineFit(row, base)


# -- the device calls ----------------------------------------------------------------------------------------------

def per_spectrum(value, K, what):
    """``value`` as a list of K: one value for all, or one per spectrum."""
    if np.ndim(value) == 0:
        return [value] * K
    if len(value) != K:
        raise ValueError("baseline: %s is one value or one per spectrum" % what)
    return list(value)


def pack_jobs(K, deg, intervals, complement):
    """The per-spectrum arrays the library takes: deg (int32), R (int32), edges (float64, 2 sum R), complement (int32).
    ``intervals``: None, or K entries, each None or a list of ``(lo, hi)``."""
    d = np.array([int(x) for x in per_spectrum(deg, K, "deg")], dtype=np.int32)
    if np.any((d < 0) | (d > MAX_DEG)):
        raise ValueError("baseline: the degree is 0 .. %d" % MAX_DEG)
    intervals = [None] * K if intervals is None else list(intervals)
    if len(intervals) != K:
        raise ValueError("baseline: one list of intervals per spectrum")
    R = np.array([0 if iv is None else len(iv) for iv in intervals], dtype=np.int32)
    parts = [_cabi.f64(iv).reshape(-1, 2).ravel() for iv in intervals if iv is not None and len(iv)]
    edges = np.concatenate(parts) if parts else np.empty(0)
    c = np.array([1 if x else 0 for x in per_spectrum(complement, K, "complement")], dtype=np.int32)
    return d, R, edges, c


def fit_many(ws, ys, deg=2, intervals=None, complement=False, device=0, return_baseline=True):
    """The rows of K spectra on the GPU (nmrfit_baseline_fit): ``ws`` K grids (any lengths, any order), ``ys`` per
    spectrum a 1-D array or a (2, N) array of two channels that share the grid and the mask; ``deg``, ``complement``: one
    value or one per spectrum; ``intervals``: None (with ``complement=True``: the whole grid) or K lists of ``(lo, hi)``
    in units of w.  Returns per spectrum a ``BaselineFit`` (1-D) or a pair of them (two channels).  Lists of any length
    are cut into library calls of at most 65535 spectra and 2^26 grid points."""
    from .utils import _weight_calls
    K = len(ws)
    if len(ys) != K:
        raise ValueError("baseline.fit_many: one y per grid")
    ws = [_cabi.f64(w).ravel() for w in ws]
    ys = [_cabi.f64(y) for y in ys]
    for k, (w, y) in enumerate(zip(ws, ys)):
        if y.ndim not in (1, 2) or (y.ndim == 2 and y.shape[0] != 2) or y.shape[-1] != len(w) or len(w) == 0:
            raise ValueError("baseline.fit_many: y is (N,) or (2, N) with N = len(w) > 0 (spectrum %d)" % k)
    deg_all, _, _, comp_all = pack_jobs(K, deg, intervals, complement)
    intervals = [None] * K if intervals is None else list(intervals)
    lib = _cabi.lib()
    result = [None] * K
    for C in (1, 2):
        idx = [k for k in range(K) if ys[k].ndim == C]
        for i0, i1 in _weight_calls([len(ws[k]) for k in idx]):
            sel = idx[i0:i1]
            n = len(sel)
            N = np.array([len(ws[k]) for k in sel], dtype=np.int64)
            total = int(N.sum())
            w = np.concatenate([ws[k] for k in sel])
            y = np.concatenate([ys[k].reshape(C, -1) for k in sel], axis=1).ravel()
            d, R, edges, comp = pack_jobs(n, deg_all[sel], [intervals[k] for k in sel], comp_all[sel])
            rows = np.empty(C * n * ROW)
            base = np.empty(C * total) if return_baseline else None
            _cabi.check(lib.nmrfit_baseline_fit(int(device), n, _cabi.ptr(N), _cabi.ptr(w), C, _cabi.ptr(y), _cabi.ptr(d),
                                                _cabi.ptr(R), _cabi.ptr(edges) if edges.size else None, _cabi.ptr(comp),
                                                _cabi.ptr(rows), _cabi.ptr(base)))
            rows = rows.reshape(C, n, ROW)
            off = np.concatenate(([0], np.cumsum(N)))
            for i, k in enumerate(sel):
                fits = [BaselineFit(rows[c, i], base[c * total + off[i]:c * total + off[i + 1]].copy() if return_baseline else None)
                        for c in range(C)]
                result[k] = fits[0] if C == 1 else tuple(fits)
    return result


def sample_noise_many(ws, ys, regions, device=0):
    """``peaks.sample_noise(w, y, xstart, xstop)`` -- the reference's utils.sample_noise -- for many spectra in one
    library call: a quadratic over ``xstart <= w <= xstop`` and the standard deviation of what is left.  ``regions``: one
    ``(xstart, xstop)`` pair or one per spectrum; ``ys`` per spectrum 1-D or (2, N).  Returns per spectrum the sigma (a
    float, or a pair for two channels); NaN where the stretch holds fewer than three points."""
    K = len(ws)
    regions = np.asarray(regions, dtype=np.float64)
    if regions.shape == (2,):
        regions = np.tile(regions, (K, 1))
    if regions.shape != (K, 2):
        raise ValueError("sample_noise_many: one (xstart, xstop) pair, or one per spectrum")
    got = fit_many(ws, ys, deg=2, intervals=[[tuple(r)] for r in regions], complement=False, device=device,
                   return_baseline=False)
    return [f.sigma if isinstance(f, BaselineFit) else (f[0].sigma, f[1].sigma) for f in got]


def subtract_rotated(u, v, b, p0, p1):
    """New arrays ``u - b cos(phi_j)`` and ``v + b sin(phi_j)``, phi_j = p0 + (p1 j) / N: the spectrum whose
    phase-corrected real channel ``ps2(u, v, p0, p1)[0]`` is lower by the baseline ``b`` and whose imaginary channel is
    unchanged -- what undoes adding ``ps2(b, 0, p0, p1, inv=True)`` to (u, v)."""
    u, v, b = np.asarray(u, dtype=np.float64), np.asarray(v, dtype=np.float64), np.asarray(b, dtype=np.float64)
    N = u.shape[-1]
    phi = p0 + (p1 * np.arange(N)) / N
    return u - b * np.cos(phi), v + b * np.sin(phi)


def option(value):
    """``fit_many``'s ``residual_baseline`` keyword as the keyword arguments of ``FitBatch.residual_baseline``: a degree,
    or a dict with ``deg``, ``margin`` (the peaks' bounds are widened about their centres by this factor and excluded),
    ``intervals`` (given: used as they are for every fit, with ``complement``), ``return_baseline``."""
    if value is None or value is False:
        return None
    opts = dict(value) if isinstance(value, dict) else dict(deg=1 if value is True else int(value))
    unknown = set(opts) - {"deg", "margin", "intervals", "complement", "return_baseline"}
    if unknown:
        raise ValueError("fit_many: residual_baseline takes deg, margin, intervals, complement, return_baseline (got %s)"
                         % ", ".join(sorted(unknown)))
    opts.setdefault("deg", 1)
    opts.setdefault("margin", 1.0)
    opts.setdefault("return_baseline", False)
    return opts


def widened(bounds, margin):
    """``(lo, hi)`` pairs widened about their centres by the factor ``margin`` (1: as they are)."""
    if float(margin) == 1.0:
        return [(float(lo), float(hi)) for lo, hi in bounds]
    out = []
    for lo, hi in bounds:
        c, h = 0.5 * (lo + hi), 0.5 * abs(hi - lo) * float(margin)
        out.append((c - h, c + h))
    return out


def fit_intervals(opts, f):
    """(intervals, complement) of one fit under the ``residual_baseline`` options: the caller's, or the complement of
    the fit's peaks' bounds widened by ``margin``."""
    if opts.get("intervals") is not None:
        return list(opts["intervals"]), bool(opts.get("complement", True))
    return widened([tuple(p.bounds) for p in f.data.peaks], opts["margin"]), True

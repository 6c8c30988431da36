"""
Host mirror of the reference's non-interactive peak utilities (nmrfit/utils.py): ``Peak`` (:58-93),
``Peaks`` (:14-55), ``AutoPeakSelector`` (:670-783), the programmatic path of ``BoundsSelector``
(:342-442, ``supress=True``), ``find_peak`` (:819-853), ``rnd_data`` (:856-875) and
``sample_noise`` (:878-902).  They produce the objects the hot path consumes: ``data.peaks``
(bounds, height -> the weights of FitUtility._compute_weights; width, loc, area -> the swarm box of
Data.generate_solution_bounds).  Host code, once per dataset, as in the reference.

Out of scope: the matplotlib click selectors (BoundsSelector without ``supress``, PeakSelector) and
the ``plot`` methods.

``peakutils.baseline`` (third party, not in the reference tree, not installed; the reference pins
no version) is restated here from its published algorithm as ``baseline`` -- PARITY UNPINNED for
that function; AutoPeakSelector is therefore tested through properties on synthetic spectra, not
against reference output.  ``scipy.integrate.simps`` (utils.py:769) no longer exists in scipy;
``simpson`` is the same rule.
"""
import numpy as np
import scipy.integrate
import scipy.interpolate
import scipy.ndimage
import scipy.signal

from ._cabi import _MAX_SPECTRA_PER_CALL


class Peak:
    """One line of a spectrum: loc, height, bounds = loc -+ 2 FWHM, width (FWHM), area."""

    def __repr__(self):
        fields = (("Location", self.loc), ("Height", self.height),
                  ("Bounds", "[%s, %s]" % (self.bounds[0], self.bounds[1])), ("Width", self.width),
                  ("Area", self.area))
        return "\n".join("               %s: %s" % kv for kv in fields)


class Peaks(list):
    """A list of Peak objects with the reference's two helpers."""

    def average_height(self):
        return sum(abs(p.height) for p in self) / len(self)

    def split(self):
        """(peaks, satellites): at or above / below the average absolute height."""
        h = self.average_height()
        main, sats = Peaks(), Peaks()
        for p in self:
            (main if abs(p.height) >= h else sats).append(p)
        return main, sats


def baseline(y, deg=3, max_it=100, tol=1e-3):
    """peakutils.baseline restated: iterated least-squares polynomial fit where, after every
    fit, the data above the fit are clipped to it, until the coefficients move by less than
    ``tol`` (relative).  Returns the baseline array.  The abscissa is scaled to
    [0, max|y|**(1/(deg+1))] as in the published code, to keep the Vandermonde matrix tame."""
    y = np.array(y, dtype=float)
    order = deg + 1
    coeffs = np.ones(order)
    x = np.linspace(0.0, abs(y).max() ** (1.0 / order), y.size)
    vander = np.vander(x, order)
    pinv = np.linalg.pinv(vander)
    base = y.copy()
    for _ in range(max_it):
        new = pinv @ y
        if np.linalg.norm(new - coeffs) / np.linalg.norm(coeffs) < tol:
            break
        coeffs = new
        base = vander @ coeffs
        y = np.minimum(y, base)
    return base


def argrelmax(x, order):
    """Indices i with x[i] strictly greater than every x[i-order .. i+order] (ends clipped):
    exactly scipy.signal.argrelmax(x, order=order)[0], which the reference calls (utils.py:731),
    but by two sliding-window maxima, O(n) instead of O(n * order) -- on the reference's
    100x-upsampled grid `order` is ~10^4 points and the scipy form takes a minute."""
    x = np.asarray(x)
    order = int(order)
    if order < 1:
        raise ValueError("Order must be an int >= 1")
    n = x.size
    padded = np.pad(x, order, mode="edge")
    win = scipy.ndimage.maximum_filter1d(padded, size=order, mode="nearest")   # win[j] = max padded[j-order//2 .. +order-1]
    at = np.arange(n) + order
    left = win[at - order + order // 2]          # max of the `order` points before i
    right = win[at + 1 + order // 2]             # max of the `order` points after i
    return np.nonzero((x > left) & (x > right))[0]


class AutoPeakSelector:
    """Peak picking by local non-maximum suppression + FWHM analysis (utils.py:670-783).

    The spectrum is upsampled 100x by linear interpolation, smoothed (Savitzky-Golay, 11 points,
    order 4) for the maxima search; a maximum counts when its height above the constant baseline
    exceeds ``thresh``.  Width = distance between the half-height crossings nearest to the
    maximum, bounds = loc -+ 2 widths, area = Simpson integral over the bounds above a local
    constant baseline."""

    def __init__(self, w, u, thresh, window):
        self.thresh = thresh
        self.window = window
        w = np.asarray(w, dtype=float)
        interp = scipy.interpolate.interp1d(w, np.asarray(u, dtype=float))
        self.w = np.linspace(w.min(), w.max(), int(len(w) * 100))
        self.u = interp(self.w)
        self.u_smoothed = scipy.signal.savgol_filter(self.u, 11, 4)
        self.baseline = baseline(self.u_smoothed, 0)[0]
        self.peaks = Peaks()

    def find_maxima(self):
        order = int(self.window / (self.w[1] - self.w[0]))
        for i in argrelmax(self.u_smoothed, order):
            p = Peak()
            p.loc = self.w[i]
            p.i = i
            p.height = self.u[i] - self.baseline
            if p.height > self.thresh:
                self.peaks.append(p)

    def find_width(self):
        kept = Peaks()
        above = self.u - self.baseline
        for p in self.peaks:
            side = np.sign(p.height / 2.0 - above)
            cross = side[:-1] - side[1:]              # < 0 where the curve falls through half height
            falling = np.where(cross < 0)[0]
            rising = np.where(cross > 0)[0]
            if falling.size == 0 or rising.size == 0:
                continue                               # (the reference raises here; nothing to measure)
            x_right = self.w[falling[np.argmin(np.abs(self.w[falling] - p.loc))]]
            x_left = self.w[rising[np.argmin(np.abs(self.w[rising] - p.loc))]]
            if not x_left < x_right:
                continue
            p.width = x_right - x_left
            p.bounds = [p.loc - 2 * p.width, p.loc + 2 * p.width]
            p.idx = np.where((self.w >= p.bounds[0]) & (self.w <= p.bounds[1]))
            p.baseline = baseline(self.u[p.idx], 0)[0]
            p.height = self.u[p.i] - p.baseline
            p.area = scipy.integrate.simpson(self.u[p.idx] - p.baseline, x=self.w[p.idx])
            kept.append(p)
        self.peaks = kept

    def find_peaks(self):
        self.find_maxima()
        self.find_width()


class BoundsSelector:
    """Crop (w, u, v) to low < w < high (utils.py:416-442).  Only the programmatic form: the
    reference's interactive form (two mouse clicks on a matplotlib figure) is out of scope."""

    def __init__(self, w, u, v, supress=True):
        if not supress:
            raise NotImplementedError("interactive bounds selection is a GUI feature of the reference; "
                                      "pass low and high")
        self.w, self.u, self.v = np.asarray(w), np.asarray(u), np.asarray(v)
        self.supress = True

    def apply_bounds(self, low=None, high=None):
        if low is None or high is None:
            raise ValueError("low and high are required")
        keep = np.where((self.w > low) & (self.w < high))
        self.w, self.u, self.v = self.w[keep], self.u[keep], self.v[keep]
        return self.w, self.u, self.v


def find_peak(x, y, low, high):
    """(height, location, index within the window) of the maximum of y for low <= x <= high."""
    sel = np.where((x <= high) & (x >= low))
    k = np.argmax(y[sel])
    return y[sel][k], x[sel][k], k


def rnd_data(width, origdata):
    """origdata + width * standard normal noise (numpy's global generator, as in the reference)."""
    return origdata + width * np.random.randn(origdata.size)


def sample_noise(X, Y, xstart, xstop):
    """Standard deviation of Y about a quadratic fit, over xstart <= X <= xstop."""
    sel = np.where((X <= xstop) & (X >= xstart))
    xs, ys = X[sel], Y[sel]
    return np.std(ys - np.poly1d(np.polyfit(xs, ys, 2))(xs))


# ---- automatic peak picking on the GPU (opt-in; csrc/peaks.hip, nmrfit_peaks_pick) --------------------------------------

UPSAMPLE = 100                     # AutoPeakSelector: np.linspace(w.min(), w.max(), len(w) * 100)
POINT_BUDGET = 1 << 26             # upsampled points per library call: U and S take 16 bytes each point (1 GiB)


def grid_points(wmin, wmax, M, k):
    """np.linspace(wmin, wmax, M)[k] for an integer array k, in numpy's arithmetic: k * step + wmin, the last point
    wmax; a step that rounds to 0 takes (k / div) * delta."""
    k = np.asarray(k, dtype=np.int64)
    delta = np.float64(wmax) - np.float64(wmin)
    div = M - 1
    step = delta / div
    kf = k.astype(np.float64)
    W = (kf / div) * delta + wmin if step == 0 else kf * step + wmin
    return np.where(k == M - 1, np.float64(wmax), W)


def _prepare(w, u, window=None):
    """Host side of one spectrum, with the host's exceptions: (xs, ys sorted by w, the 10 savgol edge values, order,
    M).  order is None without a window."""
    w = np.asarray(w, dtype=float)
    u = np.asarray(u, dtype=float)
    if w.ndim != 1 or u.ndim != 1 or len(w) != len(u):
        raise ValueError("x and y arrays must be equal in length along interpolation axis.")
    ind = np.argsort(w, kind="mergesort")          # interp1d's own sort
    xs, ys = w[ind], u[ind]
    M = int(len(w) * UPSAMPLE)
    wmin, wmax = w.min(), w.max()
    order = None
    if window is not None:
        W01 = grid_points(wmin, wmax, M, [0, 1])
        with np.errstate(divide="ignore", invalid="ignore"):
            order = int(window / (W01[1] - W01[0]))     # (N = 1: a zero step, OverflowError, as on the host)
        if order < 1:
            raise ValueError("Order must be an int >= 1")
    if len(w) < 2:
        raise ValueError("x and y arrays must have at least 2 entries")
    head = np.interp(grid_points(wmin, wmax, M, np.arange(11)), xs, ys)
    tail = np.interp(grid_points(wmin, wmax, M, np.arange(M - 11, M)), xs, ys)
    edges = np.concatenate([scipy.signal.savgol_filter(head, 11, 4)[:5], scipy.signal.savgol_filter(tail, 11, 4)[-5:]])
    return xs, ys, edges, order, M


def _calls(Ms):
    """[k0, k1) ranges of at most _MAX_SPECTRA_PER_CALL spectra and POINT_BUDGET upsampled points (a lone spectrum
    above the budget is its own call; the library refuses it)."""
    k0, n = 0, len(Ms)
    while k0 < n:
        k1, pts = k0, 0
        while k1 < n and k1 - k0 < _MAX_SPECTRA_PER_CALL and (k1 == k0 or pts + Ms[k1] <= POINT_BUDGET):
            pts += Ms[k1]
            k1 += 1
        yield k0, k1
        k0 = k1


def _per_spectrum(x, S, name):
    a = np.asarray(x, dtype=np.float64)
    if a.ndim == 0:
        return [float(a)] * S
    if a.shape != (S,):
        raise ValueError("%s must be a scalar or one value per spectrum (%d), got shape %s" % (name, S, a.shape))
    return list(a)


def _device_smooth(prep, device=0):
    """Stage 1 alone (nmrfit_diag_peaks_smooth): [(U, S)] of every prepared spectrum."""
    from . import _cabi
    out = []
    for k0, k1 in _calls([p[4] for p in prep]):
        part = prep[k0:k1]
        N = np.array([len(p[0]) for p in part], dtype=np.int64)
        xs = np.ascontiguousarray(np.concatenate([p[0] for p in part]))
        ys = np.ascontiguousarray(np.concatenate([p[1] for p in part]))
        edges = np.ascontiguousarray(np.concatenate([p[2] for p in part]))
        tot = int(N.sum()) * UPSAMPLE
        U = np.empty(tot)
        Sm = np.empty(tot)
        _cabi.check(_cabi.lib().nmrfit_diag_peaks_smooth(int(device), len(part), _cabi.ptr(N), _cabi.ptr(xs),
                                                         _cabi.ptr(ys), _cabi.ptr(edges), _cabi.ptr(U), _cabi.ptr(Sm)))
        o = 0
        for p in part:
            out.append((U[o:o + p[4]], Sm[o:o + p[4]]))
            o += p[4]
    return out


def smooth_many(ws, us, device=0):
    """The device's upsampled and smoothed spectra: [(U, S)] with U = interp1d(w, u)(W) on the 100x grid and
    S = savgol_filter(U, 11, 4), bit for bit (what AutoPeakSelector holds as ``u`` and ``u_smoothed``)."""
    ws, us = list(ws), list(us)
    if len(ws) != len(us):
        raise ValueError("ws and us differ in length")
    return _device_smooth([_prepare(w, u) for w, u in zip(ws, us)], device)


def capacity(M, order):
    """The most maxima a spectrum of M upsampled points can have over +-order: two are more than order apart."""
    return (M - 1) // (order + 1) + 1


def find_peaks_many(ws, us, thresh=0.0, window=0.02, device=0, return_baseline=False):
    """``AutoPeakSelector(w, u, thresh, window).find_peaks()`` for every (w, u), on the GPU (opt-in; csrc/peaks.hip).
    Returns a list of ``Peaks`` (and, with ``return_baseline``, the array of global baselines, the host's
    ``selector.baseline``).  ``thresh`` and ``window``: scalars or one value per spectrum.  Spectra may differ in
    length; lists of any length are cut into library calls of at most 65535 spectra and POINT_BUDGET (2^26) upsampled
    points.  Count, i, loc, width, bounds and idx are the host's exactly; the global and local baselines, height and area
    are compensated sums of the device's own, within a few ulp of the exactly summed values (measured: bit-identical to
    them in nearly every case), and so agree with the host as far as the host's own means (BLAS's order) are accurate:
    about 1e-15 relative on ordinary spectra, 1e-10 of max|u| on subnormal ones.  Argument errors raise the host's
    exceptions before any device work."""
    from . import _cabi
    ws, us = list(ws), list(us)
    if len(ws) != len(us):
        raise ValueError("ws and us differ in length")
    S = len(ws)
    th = _per_spectrum(thresh, S, "thresh")
    wi = _per_spectrum(window, S, "window")
    prep = [_prepare(w, u, win) for w, u, win in zip(ws, us, wi)]
    result, base_all = [], np.empty(S)
    for k0, k1 in _calls([p[4] for p in prep]):
        part = prep[k0:k1]
        n = len(part)
        N = np.array([len(p[0]) for p in part], dtype=np.int64)
        xs = np.ascontiguousarray(np.concatenate([p[0] for p in part]))
        ys = np.ascontiguousarray(np.concatenate([p[1] for p in part]))
        edges = np.ascontiguousarray(np.concatenate([p[2] for p in part]))
        order = np.array([p[3] for p in part], dtype=np.int64)
        th_arr = np.array(th[k0:k1], dtype=np.float64)
        cap = np.array([capacity(p[4], p[3]) for p in part], dtype=np.int64)
        off = np.concatenate([[0], np.cumsum(cap)])
        base = np.empty(n)
        count = np.zeros(n, dtype=np.int64)
        pidx = np.empty((int(off[-1]), 3), dtype=np.int64)
        pval = np.empty((int(off[-1]), 5), dtype=np.float64)
        _cabi.check(_cabi.lib().nmrfit_peaks_pick(
            int(device), n, _cabi.ptr(N), _cabi.ptr(xs), _cabi.ptr(ys), _cabi.ptr(edges), _cabi.ptr(order),
            _cabi.ptr(th_arr), _cabi.ptr(base), _cabi.ptr(count), _cabi.ptr(pidx), _cabi.ptr(pval)))
        base_all[k0:k1] = base
        for k in range(n):
            out = Peaks()
            for r in range(int(off[k]), int(off[k]) + int(count[k])):
                i, lo, hi = pidx[r]
                loc, width, pb, height, area = pval[r]
                p = Peak()
                p.loc = np.float64(loc)
                p.i = np.int64(i)
                p.width = np.float64(width)
                p.bounds = [p.loc - 2 * p.width, p.loc + 2 * p.width]
                p.idx = (np.arange(lo, hi + 1, dtype=np.int64),)
                p.baseline = np.float64(pb)
                p.height = np.float64(height)
                p.area = np.float64(area)
                out.append(p)
            result.append(out)
    return (result, base_all) if return_baseline else result

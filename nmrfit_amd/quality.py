"""
Residual statistics of finished fits (include/nmrfit_amd_quality.h, csrc/quality.hip).

The reference judges a fit by a plot of ``fit.V - data.V`` (plot.residual; panel E of plot.isotope_ratio).  At the rates
of ``fit_many`` nobody reads plots: here the residual e = V_fit - V_data is reduced on the device -- per region of the
grid (a peak's bounds, say), over the whole grid and over what no region holds -- and ``(R + 2)`` rows of 8 doubles per
fit come back instead of the ``(2 P + 6) N`` doubles of ``generate_result``.  The rows are summed in a fixed order, so a
fit's rows are the same bits alone, in any batch and from call to call; ``residual_stats_host`` is the numpy mirror of
that order on the arrays ``generate()`` returns.

    residual_stats_many(spectra, X, regions)    K fits from host arrays, one library call (nmrfit_quality_stats)
    residual_stats(w, u, v, x, regions)         one fit
    FitBatch.residual_stats(X, regions)         the fits of a device batch, on its resident spectra
    FitUtility.residual_stats(regions)          a finished fit; the regions default to its peaks' bounds
    fit_many(jobs, quality=True)                every returned fit carries ``fit.quality``
"""
import numpy as np

from . import _cabi

ROW = 8                  # doubles per row (NMRFIT_QUALITY_ROW)
TILE, WAVE = 256, 64     # the summation order's units: point j is lane j % 64 of wave (j % 256) / 64 of tile j / 256
MAX_REGIONS = 2048       # per fit (NMRFIT_QUALITY_MAX_REGIONS)


class FitQuality:
    """The rows of one fit: ``rows`` is (R + 2, 8) -- the R regions, the whole grid, the complement of the regions'
    union -- each ``n, sum e, sum e^2, sum (e_j - e_{j-1})^2, sum d, sum d^2, max |e|, argmax`` (e = V_fit - V_data,
    d = V_data).  Per-row arrays (nan where n = 0 or a denominator is 0):

    n, bias = sum e / n, rms = sqrt(sum e^2 / n), durbin_watson = sum (e_j - e_{j-1})^2 / sum e^2 (near 2 for white
    noise, towards 0 for a structured residual), r2 = 1 - sum e^2 / (sum d^2 - (sum d)^2 / n), max_abs, argmax.

    whole, outside, regions : FitQuality views of the whole-grid row, the complement row and the region rows
    sigma_outside : the rms of the complement row -- the noise estimate where no peak is, without naming a noise region
    chi2_reduced(sigma=None, nparams=None) : sum e^2 / (sigma^2 (n - nparams)) of the whole grid
    """

    def __init__(self, rows, nparams=None, _special=True):
        self.rows = np.asarray(rows, dtype=np.float64).reshape(-1, ROW)
        self.nparams = nparams
        self._special = _special and len(self.rows) >= 2     # (the last two rows are the whole grid and the complement)

    def _view(self, sel):
        return FitQuality(self.rows[sel], self.nparams, _special=False)

    @property
    def regions(self):
        return self._view(slice(0, len(self.rows) - 2)) if self._special else self

    @property
    def whole(self):
        return self._view(slice(-2, -1))

    @property
    def outside(self):
        return self._view(slice(-1, None))

    @staticmethod
    def _ratio(a, b):
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.where(b != 0, a / np.where(b != 0, b, 1.0), np.nan)

    @property
    def n(self):
        return self.rows[:, 0]

    @property
    def bias(self):
        return self._ratio(self.rows[:, 1], self.rows[:, 0])

    @property
    def rms(self):
        with np.errstate(invalid="ignore"):
            return np.sqrt(self._ratio(self.rows[:, 2], self.rows[:, 0]))

    @property
    def durbin_watson(self):
        return self._ratio(self.rows[:, 3], self.rows[:, 2])

    @property
    def r2(self):
        r = self.rows
        with np.errstate(invalid="ignore"):
            spread = r[:, 5] - self._ratio(r[:, 4] * r[:, 4], r[:, 0])
        return 1.0 - self._ratio(r[:, 2], spread)

    @property
    def max_abs(self):
        return self.rows[:, 6]

    @property
    def argmax(self):
        return self.rows[:, 7].astype(np.int64)

    @property
    def sigma_outside(self):
        return float(self.outside.rms[0])

    def chi2_reduced(self, sigma=None, nparams=None):
        """sum e^2 / (sigma^2 (n - nparams)) of the whole grid; ``sigma``: ``sigma_outside`` by default; ``nparams``:
        the fit's D = 4 + 3 P by default (what the constructor was given, else 0)."""
        sigma = self.sigma_outside if sigma is None else float(sigma)
        if nparams is None:
            nparams = 0 if self.nparams is None else self.nparams
        n, _, see = self.whole.rows[0, :3]
        dof = n - nparams
        return float(see / (sigma * sigma * dof)) if dof != 0 and sigma != 0 else float("nan")

    def __repr__(self):
        return "FitQuality(%d rows, rms %s)" % (len(self.rows), np.array2string(self.rms, precision=4))


# -- the numpy mirror --------------------------------------------------------------------------------------------

def region_indices(w, regions):
    """(R, 2) int64: every region's first and last grid index -- the nearest points to its two edges as
    ``np.argmin(|w - edge|)`` finds them, sorted (the rule of ``utils.compute_weights``)."""
    w = np.asarray(w, dtype=np.float64)
    out = np.empty((len(regions), 2), dtype=np.int64)
    for r, (lo, hi) in enumerate(regions):
        a, b = int(np.abs(w - lo).argmin()), int(np.abs(w - hi).argmin())
        out[r] = min(a, b), max(a, b)
    return out


def _tree_sum(terms):
    """The sum of ``terms`` (+0.0 already where a point does not count) in the device's order: the wave tree, the four
    waves of a tile in order, the tiles in ascending order."""
    n = len(terms)
    tiles = max(1, -(-n // TILE))
    a = np.zeros(tiles * TILE)
    a[:n] = terms
    a = a.reshape(tiles * (TILE // WAVE), WAVE)
    a = a[:, :32] + a[:, 32:]
    for half in (16, 8, 4, 2, 1):
        a = a[:, :half] + a[:, half:]
    a = a.reshape(tiles, TILE // WAVE)
    t = a[:, 0]
    for wv in range(1, TILE // WAVE):
        t = t + a[:, wv]
    s = t[0]
    for tile in range(1, tiles):
        s = s + t[tile]
    return s


def _row(e, d, member):
    """One row from the residual, the data and the row's membership mask."""
    ee, dd = e * e, d * d
    step = np.zeros_like(e)
    step[1:] = e[1:] - e[:-1]
    ss = step * step
    pair = member.copy()
    pair[1:] &= member[:-1]
    pair[0] = False
    zero = np.zeros_like(e)
    with np.errstate(invalid="ignore"):
        sums = [_tree_sum(np.where(m, x, zero)) for m, x in ((member, e), (member, ee), (pair, ss), (member, d), (member, dd))]
    counts = member & ~np.isnan(e)
    if counts.any():
        a = np.where(counts, np.abs(e), -1.0)
        top, at = float(a.max()), float(a.argmax())
    else:
        top, at = 0.0, -1.0
    return [float(member.sum()), sums[0], sums[1], sums[2], sums[3], sums[4], top, at]


def residual_stats_host(V, data_V, w, regions):
    """The numpy mirror of the device rows, summation order included: ``V`` and ``data_V`` as ``FitBatch.generate()`` /
    ``FitUtility.generate_result`` return them (scale 1), ``w`` the fit's grid, ``regions`` a list of ``(lo, hi)``.
    Returns the (R + 2, 8) array the device gives for the same fit, bit for bit."""
    V, d = np.asarray(V, dtype=np.float64), np.asarray(data_V, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        e = V - d
    j = np.arange(len(e))
    fl = region_indices(w, regions)
    held = np.zeros(len(e), dtype=bool)
    rows = []
    for first, last in fl:
        member = (j >= first) & (j <= last)
        held |= member
        rows.append(_row(e, d, member))
    rows.append(_row(e, d, np.ones(len(e), dtype=bool)))
    rows.append(_row(e, d, ~held))
    return np.array(rows, dtype=np.float64).reshape(len(fl) + 2, ROW)


# -- the device calls ----------------------------------------------------------------------------------------------

def pack_edges(regions):
    """K lists of ``(lo, hi)`` (None: no region) as the two arrays the library takes: R (int32, K) and the edges
    (float64, 2 sum R), fit after fit."""
    R = np.array([0 if reg is None else len(reg) for reg in regions], dtype=np.int32)
    parts = [_cabi.f64(reg).reshape(-1, 2).ravel() for reg in regions if reg is not None and len(reg)]
    return R, (np.concatenate(parts) if parts else np.empty(0))


def split_rows(out, R, nparams):
    """The library's output, fit after fit, as one FitQuality per fit."""
    roff = np.concatenate(([0], np.cumsum(R.astype(np.int64) + 2)))
    rows = out.reshape(-1, ROW)
    return [FitQuality(rows[roff[k]:roff[k + 1]], nparams=int(nparams[k])) for k in range(len(R))]


def residual_stats_many(spectra, X, regions, device=0):
    """The rows of K fits on the GPU: ``spectra`` K tuples ``(w, u, v)`` (any lengths), ``X`` K parameter vectors
    (4 + 3 P_k), ``regions`` K lists of ``(lo, hi)`` in units of w.  Returns K ``FitQuality``.  Lists of any length are
    cut into library calls of at most 65535 fits and 2^26 grid points."""
    from .utils import _weight_calls
    K = len(spectra)
    if len(X) != K or len(regions) != K:
        raise ValueError("residual_stats_many: one parameter vector and one list of regions per spectrum")
    ws, us, vs = ([_cabi.f64(sp[a]).ravel() for sp in spectra] for a in range(3))
    X = [_cabi.f64(x).ravel() for x in X]
    for k, x in enumerate(X):
        if x.size < 4 or (x.size - 4) % 3:
            raise ValueError("residual_stats_many: a parameter vector has 4 + 3P entries (fit %d)" % k)
        if not len(ws[k]) == len(us[k]) == len(vs[k]):
            raise ValueError("residual_stats_many: w, u, v of a spectrum have the same length (fit %d)" % k)
    lib = _cabi.lib()
    result = []
    for k0, k1 in _weight_calls([len(w) for w in ws]):
        N = np.array([len(w) for w in ws[k0:k1]], dtype=np.int64)
        P = np.array([(x.size - 4) // 3 for x in X[k0:k1]], dtype=np.int32)
        R, edges = pack_edges(regions[k0:k1])
        w, u, v, x = (np.concatenate(a[k0:k1]) for a in (ws, us, vs, X))
        out = np.empty((int(R.sum()) + 2 * (k1 - k0)) * ROW)
        _cabi.check(lib.nmrfit_quality_stats(int(device), k1 - k0, _cabi.ptr(N), _cabi.ptr(w), _cabi.ptr(u), _cabi.ptr(v),
                                             _cabi.ptr(P), _cabi.ptr(x), _cabi.ptr(R), _cabi.ptr(edges) if edges.size else None,
                                             _cabi.ptr(out)))
        result += split_rows(out, R, 4 + 3 * P)
    return result


def residual_stats(w, u, v, x, regions, device=0):
    """``residual_stats_many`` for one spectrum: its ``FitQuality``."""
    return residual_stats_many([(w, u, v)], [x], [regions], device=device)[0]

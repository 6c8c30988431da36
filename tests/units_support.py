"""
Test infrastructure (NOT part of the nmrfit_amd package): changes of units, for tests/test_units_cpu.py and
tests/test_gpu_units.py.

A unit system is (ax, c): the factor of the frequency axis and the factor of the intensities.  Moving a whole problem
into it is

    spectrum        w ax, u c, v c, weights unchanged
    parameter row   p0, p1, r unchanged, yoff c, width ax, loc ax, a ax c          (``pscale``; a box: ``box``)
    regions, edges  ax;  sigma of the noise: c
    least squares   the rows as parameter rows, the factors c_i divided by the column's scale (``lsq_factors``)

and the law is that every output comes back multiplied by a known power of ax and c: f and the residual rows by c, the
reconstruction by c, positions by the column's scale.  When ax and c are powers of two every operation of the chain
commutes with the change EXACTLY in binary floating point, so the outputs are compared bit for bit (``Exact``).  The
objective kernels' scaled pair form takes sqrt(1/al): intensity factors are powers of FOUR wherever they run.

A negative ax is the descending twin: the grid is negated, and so are widths and areas (t = (w - loc) 2/width and
al = a r (2/width)/pi are unchanged, in both channels).  A box under a negative column scale swaps its ends, and
lb + rand (ub - lb) is not symmetric under that swap: a swarm's draws are NOT covariant under negation, only what is
evaluated at given positions is.

Physical systems (``Physical``) are affine maps of the axis with factors that are no powers of two; nothing is exact
there, they are compared by truth (tests/hp_truth.py) or by host parity.

Preconditions of an exact comparison (asserted by every exact case on its own inputs): ``same_forms`` -- the kernel's
per-particle form switches (hp_truth.kernel_forms: ``fast``, ``rec``) agree in both systems -- and ``in_range`` -- no
value, square or product the kernels form leaves [2^-900, 2^900].
"""
import math

import numpy as np

from tests import hp_truth as hp

RANGE_LO, RANGE_HI = 2.0 ** -900, 2.0 ** 900


def is_pow2(x):
    x = abs(float(x))
    return x > 0.0 and math.isfinite(x) and math.frexp(x)[0] == 0.5


class Exact:
    """(ax, c) with both factors powers of two (ax may be negative: the descending twin)."""

    def __init__(self, name, ax, c):
        assert is_pow2(ax) and is_pow2(c) and c > 0, (ax, c)
        self.name, self.ax, self.c = name, float(ax), float(c)

    def __repr__(self):
        return "%s(ax=%s2^%d, c=2^%d)" % (self.name, "-" if self.ax < 0 else "", math.frexp(abs(self.ax))[1] - 1,
                                          math.frexp(self.c)[1] - 1)

    @property
    def even(self):
        """c is a power of four (what the objective kernels' scaled form needs)."""
        return (math.frexp(self.c)[1] - 1) % 2 == 0

    # -- into the system ------------------------------------------------------------------------
    def grid(self, w):
        return np.asarray(w, dtype=np.float64) * self.ax

    def inten(self, a):
        return np.asarray(a, dtype=np.float64) * self.c

    def spectrum(self, w, u, v, weights=None):
        out = (self.grid(w), self.inten(u), self.inten(v))
        return out if weights is None else out + (np.array(weights, dtype=np.float64),)

    def pscale(self, D):
        """The D per-column factors of a parameter row."""
        s = np.ones(D)
        s[3] = self.c
        s[4::3] = self.ax
        s[5::3] = self.ax
        s[6::3] = self.ax * self.c
        return s

    def params(self, X):
        X = np.asarray(X, dtype=np.float64)
        return X * self.pscale(X.shape[-1])

    def amplitudes(self, X):
        """A parameter matrix whose widths and locations are ALREADY in this system's axis (built on its grid), with
        amplitudes of order 1: yoff c, a |ax| c."""
        X = np.array(X, dtype=np.float64)
        X[..., 3] *= self.c
        X[..., 6::3] *= abs(self.ax) * self.c
        return X

    def box(self, lower, upper):
        lo, up = self.params(lower), self.params(upper)
        return np.minimum(lo, up), np.maximum(lo, up)

    def regions(self, regions):
        return [(lo * self.ax, hi * self.ax) for lo, hi in regions]

    def sigma(self, s):
        return np.asarray(s, dtype=np.float64) * self.c

    def lsq_factors(self, cfac):
        """The factors c_i = s / h_i of a forward-difference Jacobian: h_i scales with its column."""
        cfac = np.asarray(cfac, dtype=np.float64)
        return cfac / self.pscale(cfac.size)

    # -- back -----------------------------------------------------------------------------------
    def un_inten(self, a, power=1):
        return np.asarray(a, dtype=np.float64) / self.c ** power

    def un_params(self, X):
        X = np.asarray(X, dtype=np.float64)
        return X / self.pscale(X.shape[-1])

    def un_normal(self, A, g):
        """(A, g) of the normal equations: J' = J c / sigma_i, r' = r c."""
        s = self.pscale(len(g))
        c2 = self.c * self.c
        return np.asarray(A) / c2 * np.outer(s, s), np.asarray(g) / c2 * s

    def un_quality(self, rows):
        """The (R + 2, 8) rows of quality.residual_stats: n, sum e, sum e^2, sum de^2, sum d, sum d^2, max |e|, argmax."""
        c = self.c
        return np.asarray(rows, dtype=np.float64) / np.array([1.0, c, c * c, c * c, c, c * c, c, 1.0])


IDENTITY = Exact("I", 1.0, 1.0)
E1 = Exact("E1", 2.0 ** 7, 1.0)
E2 = Exact("E2", 2.0 ** 14, 4.0 ** 14)
E3 = Exact("E3", 2.0 ** -10, 4.0 ** -12)
DESC = Exact("DESC", -2.0 ** 7, 1.0)
EXACT = (E1, E2, E3, DESC)


class Physical:
    """w' = off + ax (w - w_ref), intensities times c; widths |ax|, areas |ax| c (the lines stay what they are)."""

    def __init__(self, name, off, ax, c, w_ref=3.0):
        self.name, self.off, self.ax, self.c, self.w_ref = name, float(off), float(ax), float(c), float(w_ref)

    def __repr__(self):
        return "%s(w'=%g%+g(w-%g), c=%g)" % (self.name, self.off, self.ax, self.w_ref, self.c)

    def grid(self, w):
        return self.off + self.ax * (np.asarray(w, dtype=np.float64) - self.w_ref)

    def inten(self, a):
        return np.asarray(a, dtype=np.float64) * self.c

    def spectrum(self, w, u, v, weights=None):
        out = (self.grid(w), self.inten(u), self.inten(v))
        return out if weights is None else out + (np.array(weights, dtype=np.float64),)

    def amplitudes(self, X):
        """A parameter matrix whose widths and locations are ALREADY in this system's axis (built on its grid), with
        amplitudes of order 1: yoff c, a |ax| c -- the ratio of model to data that the unit-system particle has."""
        X = np.array(X, dtype=np.float64)
        X[..., 3] *= self.c
        X[..., 6::3] *= abs(self.ax) * self.c
        return X

    def params(self, X):
        X = np.array(X, dtype=np.float64)
        X[..., 3] *= self.c
        X[..., 4::3] *= abs(self.ax)
        X[..., 5::3] = self.off + self.ax * (X[..., 5::3] - self.w_ref)
        X[..., 6::3] *= abs(self.ax) * self.c
        return X


P1 = Physical("P1", 185.0, -25.0, 3.7e8)          # ppm, descending
P2 = Physical("P2", 2.5e4, 2.4e4, 2.1e6)          # Hz, off centre
P3 = Physical("P3", 3.0e-3, 1.0e-3, 1.0e-7)       # w' = 1e-3 (3 + s)
PHYSICAL = (P1, P2, P3)


# ---- preconditions ------------------------------------------------------------------------------------------------

def forms(X, w):
    """[(fast, rec)] of the rows of X on the grid w (hp_truth.kernel_forms), and the extremes of their exponent sums."""
    X = np.atleast_2d(X)
    frame = hp.grid_analysis(w)
    kf = [hp.kernel_forms(x, w, frame) for x in X]
    ehi = [k["ehi"] for k in kf if k["ehi"] is not None]
    elo = [k["elo"] for k in kf if k["elo"] is not None]
    return [(k["fast"], k["rec"]) for k in kf], (max(ehi) if ehi else None, min(elo) if elo else None)


def same_forms(X, w, X2, w2):
    """(rows whose form flags agree in both systems [bool array], the flags in the first system, in the second)."""
    f1, _ = forms(X, w)
    f2, _ = forms(X2, w2)
    return np.array([a == b for a, b in zip(f1, f2)]), f1, f2


def in_range(w, u, v, X):
    """No value, square or product that the kernels form from these inputs leaves [2^-900, 2^900]: the inputs, the
    squares of the intensities (the objective squares its residual), 2/width, a 2/width (the lines' amplitudes) and its
    inverse (the scaled pair form), and (span 2/width)^2 (the largest 1 + t^2)."""
    X = np.atleast_2d(np.asarray(X, dtype=np.float64))
    w, u, v = (np.asarray(a, dtype=np.float64) for a in (w, u, v))
    span = float(np.max(np.abs(w - w[w.size // 2])))
    vals = [w, u, v, u * u, v * v, X]
    if X.shape[1] > 4:
        width, loc, a = X[:, 4::3], X[:, 5::3], X[:, 6::3]
        with np.errstate(divide="ignore", over="ignore", invalid="ignore"):
            ihw = 2.0 / width
            reach = span + np.abs(loc - w[w.size // 2])
            ihw = np.where(np.abs(ihw) > hp.T_CAP / reach, hp.T_CAP / reach, ihw)     # (the width floor)
            al = a * ihw
            vals += [ihw, al, 1.0 / np.where(al == 0, 1.0, al), (reach * ihw) ** 2, a * a]
    for q in vals:
        q = np.abs(np.asarray(q, dtype=np.float64).ravel())
        q = q[q != 0.0]
        if q.size and not (np.all(np.isfinite(q)) and q.min() >= RANGE_LO and q.max() <= RANGE_HI):
            return False
    return True


# ---- the record ----------------------------------------------------------------------------------------------------

def record(case, **fields):
    """One line of the record (profiles/r15/units.txt is made of these): ``units: <case>  key=value ...``."""
    print("units: %-34s %s" % (case, "  ".join("%s=%s" % (k, fields[k]) for k in fields)))


def count_equal(a, b):
    """(number of values compared, number that are equal; NaN equals NaN)."""
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape, (a.shape, b.shape)
    same = (a == b) | ((a != a) & (b != b))
    return int(a.size), int(np.count_nonzero(same))


class Tally:
    """Counts exact comparisons of one case; ``done`` writes the record line and returns the failures."""

    def __init__(self, case, **fields):
        self.case, self.fields, self.n, self.eq, self.bad = case, fields, 0, 0, []

    def equal(self, got, want, where):
        n, eq = count_equal(got, want)
        self.n += n
        self.eq += eq
        if eq != n:
            g, w_ = np.asarray(got, dtype=np.float64).ravel(), np.asarray(want, dtype=np.float64).ravel()
            i = int(np.flatnonzero(~((g == w_) | ((g != g) & (w_ != w_))))[0])
            self.bad.append((where, n - eq, n, i, float(g[i]), float(w_[i])))
        return eq == n

    def done(self):
        record(self.case, compared=self.n, equal=self.eq, **self.fields)
        return self.bad

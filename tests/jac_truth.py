"""
Test infrastructure (NOT part of the nmrfit_amd package): a high-precision truth of the analytic Jacobian of the
real-channel residual (include/nmrfit_amd_lsq_analytic.h), one grid point at a time, and a first-order a-priori bound on
what an fp64 evaluation of each entry may be off by.  The companion of tests/hp_truth.py, whose model, constant C = 32
and rule for the bound it takes over.

For x = (p0, p1, r, yoff, width_k, loc_k, a_k, ...), s = 1/sqrt(N) (the float64 value) and q = s wt_j:

    rho_j = q (V_j - sum_k (yoff + L_k + G_k))                       hp_truth's model: ``residual_mp``
    d/dp0 = -q I_j      d/dp1 = -q I_j j/N      d/dr = -q sum_k a_k (Lh_k - Gh_k)      d/dyoff = -q P
    d/dwidth_k = +q (ihw/2) (L (1 - t^2)/S + G (1 - 2 ln2 t^2))
    d/dloc_k   = -q 2 ihw t (L/S + ln2 G)                            d/da_k = -q (r Lh + (1 - r) Gh)

Each peak's entries are sums of two PIECES, a Lorentzian and a Gaussian one (``peak_pieces``).  The bound of an entry is
C eps |q| mag, mag built by hp_truth's rule from its pieces:

    every piece's magnitude, every difference that can cancel replaced by the sum of its operands' magnitudes
        (1 - t^2 -> 1 + t^2,  1 - 2 ln2 t^2 -> 1 + 2 ln2 t^2)                            ``peak_mags``
    the piece's exact |d/dt| times dt, dt = (|w_j - w0| + |loc - w0|) |ihw| + |t|          ``peak_slopes``
        (the error of t in units of eps: the kernel forms t from the centred grid)
    for a Gaussian piece, its magnitude times ln2 (1 + t^2)                               (the exponent's rounding)

and for the phase columns (|u| + |v|)(1 + |phi|) + |I| (times j/N for p1), for yoff P, for rho itself hp.point's tol_V
with no rotation steps.  Derived, not tuned.

Gradual underflow (``underflow``).  The rule above is relative: it says nothing where fp64 is not.  For 1022 < t^2 < 1075
the Gaussian factor e = 2^-t^2 lies below the normal range, where a result is held to an ABSOLUTE 2^-1074 =: U (the
exponential itself: one unit; a product: half of one), not to a relative eps; additions of such numbers are exact.  A
Gaussian piece is e times a chain of factors -- in the order of csrc/lsq_tile.h: a: e rg q;  r: e dg q;  loc: e ag ln2
(2 q ihw t);  width: e ag (1 - 2 ln2 t^2) (q ihw / 2);  the model: e ag q -- so an absolute error U on an intermediate x of
the chain reaches the entry multiplied by the rest of the chain, |entry's piece| / |x|.  The term is U times the sum of
those ratios over the intermediates (e included, the final product included) that lie below 2^-1022; it is absolute, C
does not multiply it, and it is zero wherever every intermediate is normal (or e underflows to nothing: then the ratio
times e itself is below U times the cofactor, which the term states).  The Lorentzian pieces cannot get there:
1 / S >= 1e-36.
"""
import math

import mpmath
import numpy as np

from tests import hp_truth as hp

mp = mpmath.mp
PIECES = ("aL", "aG", "rL", "rG", "locL", "locG", "wL", "wG")
GAUSSIAN = {"aG", "rG", "locG", "wG"}
LN2 = math.log(2.0)


def scale(N):
    """s = 1/sqrt(N) as the library forms it: the correctly rounded root, one division."""
    return 1.0 / math.sqrt(float(N))


def peak_pieces(t, ihw, r, a):
    """The eight pieces of one peak's entries as functions of t (everything mpf):
    d/da = -q (aL + aG), d/dr's term = -q (rL - rG), d/dloc = -q (locL + locG), d/dwidth = +q (wL + wG)."""
    ln2 = mp.log(2)
    S = 1 + t * t
    Lh = ihw / (mp.pi * S)
    Gh = ihw * mp.sqrt(ln2 / mp.pi) * mp.power(2, -t * t)
    L, G = a * r * Lh, a * (1 - r) * Gh
    return dict(aL=r * Lh, aG=(1 - r) * Gh, rL=a * Lh, rG=a * Gh,
                locL=2 * ihw * t * L / S, locG=2 * ln2 * ihw * t * G,
                wL=(ihw / 2) * L * (1 - t * t) / S, wG=(ihw / 2) * G * (1 - 2 * ln2 * t * t))


def peak_mags(t, ihw, r, a):
    """The pieces' magnitudes with every difference that can cancel replaced by the sum of its operands' magnitudes."""
    ln2 = mp.log(2)
    p = peak_pieces(t, ihw, r, a)
    S = 1 + t * t
    L, G = a * p["aL"], a * p["aG"]
    out = {k: abs(v) for k, v in p.items()}
    out["wL"] = abs(ihw / 2) * abs(L) * (1 + t * t) / S
    out["wG"] = abs(ihw / 2) * abs(G) * (1 + 2 * ln2 * t * t)
    return out


def peak_slopes(t, ihw, r, a):
    """|d piece / dt| in closed form, as the bounds use it."""
    ln2 = mp.log(2)
    p = peak_pieces(t, ihw, r, a)
    S = 1 + t * t
    L, G = a * p["aL"], a * p["aG"]
    return dict(aL=abs(p["aL"]) * 2 * abs(t) / S, aG=abs(p["aG"]) * 2 * ln2 * abs(t),
                rL=abs(p["rL"]) * 2 * abs(t) / S, rG=abs(p["rG"]) * 2 * ln2 * abs(t),
                locL=abs(2 * ihw * L * (1 - 3 * t * t) / (S * S)), locG=abs(2 * ln2 * ihw * G * (1 - 2 * ln2 * t * t)),
                wL=abs(ihw * t * L * (3 - t * t) / (S * S)), wG=abs(ihw * ln2 * t * G * (3 - 2 * ln2 * t * t)))


TINY = mpmath.mpf(2) ** -1022        # the smallest normal fp64
U_ABS = 2.0 ** -1074                  # the spacing below it


def underflow(e, factors, q):
    """The gradual-underflow term of one Gaussian piece e * prod(factors) * q (see the docstring): absolute, a float."""
    chain = [e]
    for f in factors:
        chain.append(chain[-1] * f)
    final = abs(chain[-1] * q)
    if final == 0:
        return 0.0
    total = mp.mpf(0)
    for x in chain:
        if abs(x) < TINY:
            total += final / abs(x)
    if final < TINY:
        total += 1
    return float(total) * U_ABS


def frame(w, w0=None, wspan=None):
    """(w0, wspan) of the grid as hp_truth's functions take them.  On a grid of ONE point wspan is 0, and a peak centred on
    it makes the floor's limit 1e18 / 0: the library's division gives +inf (no width is capped there), Python's raises.
    The smallest positive double in place of 0 gives the same +inf in fp64 and the same verdict at any precision."""
    if w0 is None or wspan is None:
        w0, wspan = hp.grid_frame(w)
    return w0, (wspan if wspan > 0 else 5e-324)


def residual_mp(x, w, u, v, weights, j, w0=None, wspan=None):
    """rho_j = q dV at the working precision, x a sequence of mpf (or floats): hp.point's dV -- the same rotation, the
    same per-peak terms (hp._peak_terms) -- times q, kept as mpf so that mpmath.diff can differentiate it."""
    w = np.asarray(w, dtype=np.float64)
    N = w.size
    w0, wspan = frame(w, w0, wspan)
    P = (len(x) - 4) // 3
    phi = mp.mpf(x[0]) + mp.mpf(x[1]) * j / N
    V = mp.cos(phi) * float(u[j]) - mp.sin(phi) * float(v[j])
    Vf = mp.mpf(0)
    for k in range(P):
        Vf += hp._peak_terms(float(w[j]), x[2], x[3], x[4 + 3 * k], x[5 + 3 * k], x[6 + 3 * k], w0, wspan, False, None, None)[0]
    return mp.mpf(scale(N)) * mp.mpf(float(weights[j])) * (V - Vf)


def point(x, w, u, v, weights, j, w0=None, wspan=None):
    """The truth at grid point j for the parameter vector x (4 + 3P floats): a dict with ``J`` (D mpf), ``r`` (mpf), their
    absolute bounds ``tol_J`` [D] and ``tol_r`` (floats, C eps folded in), and ``q``."""
    x = np.asarray(x, dtype=np.float64)
    w = np.asarray(w, dtype=np.float64)
    N, D = w.size, x.size
    P = (D - 4) // 3
    w0, wspan = frame(w, w0, wspan)
    p0, p1, r, yoff = (float(c) for c in x[:4])
    wj, uj, vj = float(w[j]), float(u[j]), float(v[j])
    q = mp.mpf(scale(N)) * mp.mpf(float(weights[j]))
    phi = mp.mpf(p0) + mp.mpf(p1) * j / N
    cs, sn = mp.cos(phi), mp.sin(phi)
    I = sn * uj + cs * vj
    frac = mp.mpf(j) / N
    J = [mp.mpf(0)] * D
    mag = [0.0] * D
    J[0], J[1] = -q * I, -q * I * frac
    mag[0] = (abs(uj) + abs(vj)) * (1 + abs(float(phi))) + float(abs(I))
    mag[1] = mag[0] * float(frac)
    J[3], mag[3] = -q * P, float(P)
    d_r, mag_r = mp.mpf(0), 0.0
    und, und_r = [0.0] * D, 0.0
    for k in range(P):
        width, loc, a = (float(c) for c in x[4 + 3 * k:7 + 3 * k])
        assert not hp.capped(width, loc, w0, wspan), "the analytic Jacobian is not defined at or below the width floor"
        ihw = 2 / mp.mpf(width)
        t = (mp.mpf(wj) - mp.mpf(loc)) * ihw
        at = float(abs(t))
        dt = (abs(wj - w0) + abs(loc - w0)) * abs(float(ihw)) + at
        args = (t, ihw, mp.mpf(r), mp.mpf(a))
        p, m, sl = peak_pieces(*args), peak_mags(*args), peak_slopes(*args)
        b = {n: float(m[n]) * (1 + (LN2 * (1 + at * at) if n in GAUSSIAN else 0.0)) + float(sl[n]) * dt for n in PIECES}
        e = mp.power(2, -t * t)
        cg = ihw * mp.sqrt(mp.log(2) / mp.pi)
        rm, am = mp.mpf(r), mp.mpf(a)
        und[4 + 3 * k] = underflow(e, [am * (1 - rm) * cg, 1 - 2 * mp.log(2) * t * t], q * ihw / 2)
        und[5 + 3 * k] = underflow(e, [am * (1 - rm) * cg, mp.log(2)], 2 * q * ihw * t)
        und[6 + 3 * k] = underflow(e, [(1 - rm) * cg], q)
        und[2] += underflow(e, [am * cg], q)
        und_r += underflow(e, [am * (1 - rm) * cg], q)
        J[4 + 3 * k], mag[4 + 3 * k] = q * (p["wL"] + p["wG"]), b["wL"] + b["wG"]
        J[5 + 3 * k], mag[5 + 3 * k] = -q * (p["locL"] + p["locG"]), b["locL"] + b["locG"]
        J[6 + 3 * k], mag[6 + 3 * k] = -q * (p["aL"] + p["aG"]), b["aL"] + b["aG"]
        d_r += p["rL"] - p["rG"]
        mag_r += b["rL"] + b["rG"]
    J[2], mag[2] = -q * d_r, mag_r
    aq = float(abs(q))
    with np.errstate(over="ignore"):      # (a one-point grid: the floor's limit is +inf, see frame)
        t_hp = hp.point(x, w, u, v, j, w0=w0, wspan=wspan, n_steps=0, imag=False)
    return dict(J=J, r=residual_mp([mp.mpf(float(c)) for c in x], w, u, v, weights, j, w0, wspan), q=float(q),
                tol_J=hp.C * hp.EPS * aq * np.array(mag) + np.array(und), tol_r=aq * t_hp["tol_V"] + und_r)


COLUMNS = ("p0", "p1", "r", "yoff", "width", "loc", "a")


def column_name(i):
    return COLUMNS[i] if i < 4 else "%s%d" % (COLUMNS[4 + (i - 4) % 3], (i - 4) // 3)

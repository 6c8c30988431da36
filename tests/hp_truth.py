"""
Test infrastructure (NOT part of the nmrfit_amd package): a high-precision truth of the hot path, one grid point at a
time, and a first-order bound on what an fp64 evaluation of it may be off by.

Everything else in the suite that serves as a reference -- the numpy / C oracle, synth._dispersion, scipy's dawsn -- is
itself float64.  Here the exact float64 inputs (w_j, u_j, v_j, j, N, x) are evaluated at ~30 significant digits with
mpmath:

    phi_j  = p0 + p1 j / N                                         proc_autophase.py:31 (real arithmetic)
    V_j    = cos(phi_j) u_j - sin(phi_j) v_j,  I_j = sin(phi_j) u_j + cos(phi_j) v_j
    real_k = yoff + a (r L_k + (1 - r) G_k)                         equations.py:141-147
    imag_k = a (r L~_k + (1 - r) G~_k)     Hilbert partners: L~ = L t,  G~ = (2/sqrt(pi)) G0 D(sqrt(ln2) t),
                                            D(x) = sqrt(pi)/2 exp(-x^2) erfi(x)
    Vf_j   = sum_k real_k;   If_j = imag_{P-1} (fit_im=True: equations.py:199 assigns) or sum_k imag_k ("sum")

with t = (w_j - loc) (2/width).  The line of a width below the kernels' floor (|2/width| > 1e18 / (wspan + |loc - w0|),
DESIGN.md "Needle widths") is the line of the floor width: that is what the library evaluates, consistently in both
channels, and what the truth evaluates too.

The bound ``tol`` is C * eps times the sum of the exact magnitudes through which a rounding of the inputs or of the
kernel's intermediates reaches the value (first order, no per-case factors):

    rotation       (|u| + |v|) (1 + |phi| + n)        n: rotation steps since the block's re-seed point
    Lorentzian     |yoff| + |L| (1 + 2|t|/(1+t^2) dt)
    Gaussian       |G| (1 + ln2 (1 + t^2) + 2 ln2 |t| dt)
    dispersion     |L~| + |AL| |1 - t^2|/(1+t^2)^2 dt
                   |G~| + |AG~| (sqrt(ln2) |1 - 2 x D(x)| dt + kDawTab/eps)
    totals         |V_j| (resp. |I_j|)

where dt = (|w_j - w0| + |loc - w0|) |2/width| + |t| is the error of t in units of eps (the kernels form t from the
centred grid w_j - w0; this is the issue's |t| kappa written so that it stays finite at t = 0), AL = a r (2/(pi width)),
AG~ the Gaussian dispersion's amplitude and kDawTab = 3.3e-16 the Dawson table's stated absolute error.  The opt-in
mixed-precision far-field kernel rounds the variation of the far peaks' tails across a chunk to fp32; its bar adds
C * eps32 * sum_far |AL| |q| rho/(1-rho) (|q| = 1/sqrt(1+tc^2), rho the peak's expansion ratio over the chunk: the
variation term's bound).

The Gaussian recurrence (csrc/objective_chunk.h gauss_add_rec; full chunks of a uniform grid, objective launches of the
default and far-field kernels) does not evaluate G at t_q.  A lane's row q (point q*64 + lane of the chunk) gets

    G_q = G_0 R^q C^(q(q-1)/2),     G_0 = AG 2^-t0^2,  R = 2^-e,  e = 2 t0 d + d^2,  C = 2^-(2 d^2),  t_q = t0 + q d

from t0 at the lane's row 0 and d = 64 grid steps in half-widths.  The inputs' errors stay coherent: with t0' and d' the
rounded values, G_0(t0') R(t0', d')^q C(d')^(q(q-1)/2) is exactly AG 2^-(t0' + q d')^2, so they reach row q only through
t_q.  What does not cancel is the rounding of the two exponents, of the exp2's and of every multiply, all made at row 0,
where s and e are large, and carried to a row where |t_q| may be ~0 and the plain Gaussian term has nothing to cover
them.  First order, in units of eps |G_q| (``rec_term``; the optional argument ``rec`` of peak_terms / point adds it
to the plain bound):

    G_0      ln2 (1 + t0^2) + 2                          rounding of s = 1 + t0^2; the exp2, the multiply by AG
    t_q      2 ln2 |t_q| (dt0 + q kd |d|)                error of t0 (dt0 eps) and of d (kd eps |d|), q times
    R^q      q [ln2 (|e| + d^2) + 2]                     e: rounding of d d and of the fma; the exp2, the multiply g *= ratio
    C^(..)   q(q-1)/2 [2 ln2 d^2 + 2]                    2 d^2: rounding of d d; the exp2, the multiply ratio *= C
    grid     2 ln2 |t_q| |ihw| grid_dev / eps            the grid's departure from the straight line through its ends
                                                         (the truth's t_q is the grid's own; the recurrence's is the line's)

with kd = 3: d = lane_step * ihw carries the roundings of the end-to-end difference and of the division that make
lane_step, and of the product.  dt0 is dt of the row-0 point.  The q^2 growth is real: a relative error of 1e-12 in C
shows as 21e-12 at row 7.
"""
import math
from fractions import Fraction

import mpmath
import numpy as np

mp = mpmath.mp
mp.dps = 30

C = 32.0                       # the one constant of the bound
EPS = 2.0 ** -52
EPS32 = 2.0 ** -23
DAW_TAB_ERR = 3.3e-16          # csrc/objective_math.h dawson_tab: stated absolute error of the gathered table
CHUNK, WAVE, MAX_BLOCKS = 512, 64, 16
T_CAP = 1.0e18                 # csrc: |t| <= 1e18 -> the width floor
ROWS = CHUNK // WAVE           # points per lane of a chunk
INV_PI = 0.31830988618379067154     # csrc/objective_math.h kInvPi
BATCH_INV = 4                  # csrc: points sharing one reciprocal in the pair form
EXP_BUDGET = 1000 // BATCH_INV   # csrc stage_peaks: a group's exponent sums stay inside +-1000/kBatchInv
REC_D_MAX = 2.0                # csrc stage_peaks: |lane_step * it| <= 2
REC_DEVK = 11.0e10             # csrc: rec_devk = grid_dev * 11e10
REC_KD = 3.0                   # roundings behind d = lane_step * ihw (see the docstring)
FAR_RHO2 = 0.01                # csrc: a peak is summed through the chunk's expansion when rho^2 <= 0.01

_SQRT_LN2 = mp.sqrt(mp.log(2))
_SQRT_PI = mp.sqrt(mp.pi)


def dawson(x):
    """D(x) = sqrt(pi)/2 exp(-x^2) erfi(x) at the working precision."""
    x = mp.mpf(x)
    if x == 0:
        return mp.mpf(0)
    if abs(x) > 100:   # (exp(-x^2) erfi(x) leaves the exponent range) the asymptotic series, converged to 1e-40
        s, term, n = mp.mpf(0), 1 / (2 * x), 0
        while abs(term) > mp.mpf(10) ** -40 * abs(s) or n == 0:
            s += term
            n += 1
            term *= (2 * n - 1) / (2 * x * x)
        return s
    return _SQRT_PI / 2 * mp.exp(-x * x) * mp.erfi(x)


def grid_frame(w):
    """(w0, wspan) of a grid exactly as the library forms them at context creation (csrc/ctx.hip analyse_grid)."""
    w = np.asarray(w, dtype=np.float64)
    w0 = float(w[w.size // 2])
    return w0, float(np.max(np.abs(w - w0)))


def grid_analysis(w):
    """(w0, wspan, lane_step, grid_dev) exactly as csrc/ctx.hip analyse_grid forms them: lane_step is 64 grid steps
    when the centred grid lies within 1e-6 of a step of the straight line through its ends (and N >= 1024), else 0."""
    w = np.asarray(w, dtype=np.float64)
    N = w.size
    w0, wspan = grid_frame(w)
    lane_step = grid_dev = 0.0
    if N >= 2 * CHUNK:
        wc = w - w0
        first = float(wc[0])
        step = (float(wc[-1]) - first) / float(N - 1)
        dev = float(np.max(np.abs(wc - (first + np.arange(N, dtype=np.float64) * step))))
        if step != 0.0 and dev <= 1.0e-6 * abs(step):
            lane_step, grid_dev = step * WAVE, 2.0 * dev
    return w0, wspan, lane_step, grid_dev


def _ilogb(v):
    return 100000 if math.isinf(v) else math.frexp(v)[1] - 1


def kernel_forms(x, w, frame=None):
    """Which forms the objective kernel's prologue (csrc/objective_prologue.h StagePeakConstants) picks for the particle x on
    the grid w, mirrored clause by clause in the same float64 operations.  Returns a dict:

        fast        every peak has 0 < al < 1e300 and, per aligned group of eight peaks, the sums of
                    ilogb((1 + tmax^2) ia) + 2 and of ilogb(ia) (ia = 1/al) lie inside +-1000/4: the pair form
        rec         lane_step != 0, |lane_step it| <= 2 and |it| grid_dev 11e10 <= 1 for every peak: the recurrence
        sign_ok     the first clause of ``fast`` alone;  ehi, elo: the group sums' extremes (None without sign_ok)
        fast_margin distance of the exponent sums from +-250, in exponent units (> 0 inside); -inf on a sign failure
        d           max |lane_step it| over the peaks (inf when lane_step == 0)
        rec_margin  min over the clauses of (2 - |d|) and (1 - |it| grid_dev 11e10) (> 0 inside); -inf when lane_step == 0;
                    a particle without a peak has both flags set, whatever the grid
        edge        al so small that 1/al overflows: the kernel's int arithmetic on ilogb(inf) is not mirrored, either
                    form may run
    """
    x = np.asarray(x, dtype=np.float64)
    w0, wspan, lane_step, grid_dev = grid_analysis(w) if frame is None else frame
    P = (x.size - 4) // 3
    r = float(x[2])
    sign_ok, edge = True, False
    ehi, elo = [], []
    dmax, devmax = 0.0, 0.0
    for k in range(P):
        width, loc, a = (float(q) for q in x[4 + 3 * k:7 + 3 * k])
        ihw = math.copysign(math.inf, width) if width == 0.0 else 2.0 / width
        locc = loc - w0
        lim = T_CAP / (wspan + abs(locc))
        it = math.copysign(lim, ihw) if abs(ihw) > lim else ihw
        ia = ihw if math.isinf(ihw) else it
        al = a * r * ia * INV_PI
        pos = 0.0 < al < 1.0e300
        if pos:
            inv = math.inf if al < 2.0 ** -1024 else 1.0 / al
            edge = edge or math.isinf(inv)
            tmax = abs(it) * (wspan + abs(locc))
            # (the kernel's fma(tmax, tmax, 1): one rounding of the exact value)
            hi = math.inf if math.isinf(tmax) else float(Fraction(tmax) ** 2 + 1)
            ehi.append(min(_ilogb(hi * inv) + 2, 100000))
            elo.append(_ilogb(inv))
        else:
            sign_ok = False
            ehi.append(100000)
            elo.append(-100000)
        dmax = max(dmax, abs(lane_step * it))
        devmax = max(devmax, abs(it) * (grid_dev * REC_DEVK))
    fast, fast_margin, hi_s, lo_s = sign_ok, math.inf, None, None
    if P and sign_ok:
        sums = [(sum(ehi[g:g + 8]), sum(elo[g:g + 8])) for g in range(0, P, 8)]
        hi_s, lo_s = max(s_[0] for s_ in sums), min(s_[1] for s_ in sums)
        fast_margin = float(min(EXP_BUDGET - hi_s, lo_s + EXP_BUDGET))
        fast = hi_s < EXP_BUDGET and lo_s > -EXP_BUDGET
    elif not sign_ok:
        fast_margin = -math.inf
    if P == 0:                       # (no peak: nothing refuses either form, whatever the grid)
        rec, rec_margin = True, math.inf
    elif lane_step == 0.0:
        rec, rec_margin, dmax = False, -math.inf, math.inf
    else:
        rec = dmax <= REC_D_MAX and devmax <= 1.0
        rec_margin = min(REC_D_MAX - dmax, 1.0 - devmax)
    return dict(fast=fast, rec=rec, sign_ok=sign_ok, ehi=hi_s, elo=lo_s, fast_margin=fast_margin, d=dmax,
                rec_margin=rec_margin, edge=edge)


def rec_term(q, t0, d, dt0, ihw, grid_dev):
    """The recurrence's addition to a Gaussian's bound at row q, in units of eps |G_q| (derived in the docstring)."""
    ln2 = math.log(2.0)
    e = abs(2.0 * t0 * d + d * d)
    tq = abs(t0 + q * d)
    d = abs(d)
    return (ln2 * (1.0 + t0 * t0) + 2.0
            + 2.0 * ln2 * tq * (dt0 + q * REC_KD * d)
            + q * (ln2 * (e + d * d) + 2.0)
            + 0.5 * q * (q - 1) * (2.0 * ln2 * d * d + 2.0)
            + 2.0 * ln2 * tq * abs(ihw) * grid_dev / EPS)


def block_len(N):
    """Points per phase re-seed block: blk_chunks = ceil(n_chunks / 16) chunks (csrc/nmrfit_internal.h kMaxBlocks)."""
    n_chunks = (N + CHUNK - 1) // CHUNK
    return ((n_chunks + MAX_BLOCKS - 1) // MAX_BLOCKS) * CHUNK


def rotation_steps(j, N):
    """Steps of the phase recurrence between point j and its block's seed (64 points a step, lane seeds at the block's
    first 64 points)."""
    return (j % block_len(N)) // WAVE


def chunk_range(wc, j):
    """[min, max] of the centred grid over point j's chunk of 512 (the table the kernels' skips and expansions use)."""
    c = j // CHUNK
    seg = wc[c * CHUNK:(c + 1) * CHUNK]
    return float(seg.min()), float(seg.max())


def effective_ihw(width, loc, w0, wspan):
    """2/width as the library evaluates it: exact unless the width is below the floor, then exactly the cap."""
    ihw = 2.0 / width
    lim = T_CAP / (wspan + abs(loc - w0))
    if abs(ihw) > lim:
        return mp.mpf(math.copysign(lim, ihw)), True
    return 2 / mp.mpf(width), False


def capped(width, loc, w0, wspan):
    return effective_ihw(width, loc, w0, wspan)[1]


def peak_terms(wj, r, yoff, width, loc, a, w0, wspan, imag=True, chunk=None, rec=None):
    """One peak at one point (see _peak_terms), the recurrence's term -- if asked for -- inside tol_real."""
    real, im, tr, ti, far32, add = _peak_terms(wj, r, yoff, width, loc, a, w0, wspan, imag, chunk, rec)
    return real, im, (tr + add if rec is not None else tr), ti, far32


def _peak_terms(wj, r, yoff, width, loc, a, w0, wspan, imag, chunk, rec):
    """One peak at one point: (real, imag, tol_real, tol_imag, far32, rec_add) -- values as mpf, bounds in units of
    C*eps (floats), far32 the fp32 variation bound of the mixed-precision far-field kernel (units of C*eps32).  ``rec``:
    None, or (q, w_row0, lane_step, grid_dev) -- the point's row in its chunk, the grid value of the same lane's row 0
    -- for rec_add, the Gaussian recurrence's term of tol_real (kept apart: tol_real is the plain bound)."""
    ihw, _ = effective_ihw(width, loc, w0, wspan)
    wj_, loc_, r_, a_ = mp.mpf(wj), mp.mpf(loc), mp.mpf(r), mp.mpf(a)
    t = (wj_ - loc_) * ihw
    s = 1 + t * t
    AL = a_ * r_ * ihw / mp.pi
    AG = a_ * (1 - r_) * ihw * mp.sqrt(mp.log(2) / mp.pi)
    L = AL / s
    G = AG * mp.power(2, -t * t)
    real = mp.mpf(yoff) + L + G
    at = float(abs(t))
    dt = (abs(wj - w0) + abs(loc - w0)) * abs(float(ihw)) + at
    tr = abs(yoff) + float(abs(L)) * (1 + 2 * at / (1 + at * at) * dt) \
        + float(abs(G)) * (1 + math.log(2) * (1 + at * at) + 2 * math.log(2) * at * dt)
    add = 0.0
    if rec is not None:
        q, w_row0, lane_step, grid_dev = rec
        fi = float(ihw)
        t0 = (w_row0 - loc) * fi
        dt0 = (abs(w_row0 - w0) + abs(loc - w0)) * abs(fi) + abs(t0)
        add = float(abs(G)) * rec_term(q, t0, lane_step * fi, dt0, fi, grid_dev)
    im, ti = mp.mpf(0), 0.0
    if imag:
        x = _SQRT_LN2 * t
        D = dawson(x)
        AGd = AG * 2 / _SQRT_PI
        HL = AL * t / s
        HG = AGd * D
        im = HL + HG
        ti = float(abs(HL)) + float(abs(AL)) * abs(1 - at * at) / (1 + at * at) ** 2 * dt \
            + float(abs(HG)) + float(abs(AGd)) * (float(_SQRT_LN2) * float(abs(1 - 2 * x * D)) * dt + DAW_TAB_ERR / EPS)
    far32 = 0.0
    if chunk is not None:
        lo, hi = chunk
        fi = float(ihw)
        tc = (0.5 * (lo + hi) - (loc - w0)) * fi
        hk = 0.5 * (hi - lo) * fi
        den = 1 + tc * tc
        if den * FAR_RHO2 >= hk * hk * (1 - 1e-9) or not math.isfinite(den):   # (the kernel's test, rounding-safe)
            rho = min(abs(hk) / math.sqrt(den), 0.5) if math.isfinite(den) else 0.0
            far32 = float(abs(AL)) / math.sqrt(den) * rho / (1 - rho) if math.isfinite(den) else 0.0
    return real, im, tr, ti, far32, add


def point(x, w, u, v, j, w0=None, wspan=None, n_steps=None, imag=True, chunk=None, rec=None):
    """The truth at grid point j of (w, u, v) for the parameter vector x (4 + 3P).  Returns a dict of floats:
    V, I (the rotated data), Vf, If1 (last peak), If2 (all peaks), real[k], imag[k] and their bounds tol_V (data and
    real model), tol_I1, tol_I2, tol_real[k], tol_imag[k] (absolute, C*eps folded in), far32 (absolute, C*eps32 folded
    in).  w0 / wspan default to the grid's own frame; n_steps to the objective kernels' phase recurrence.  ``rec``:
    None, or (lane_step, grid_dev) of a uniform grid -- every Gaussian's bound then takes the recurrence's term for
    point j's row, and the plain bounds (what rec=None returns, bit for bit) come along under "plain"."""
    x = np.asarray(x, dtype=np.float64)
    w = np.asarray(w, dtype=np.float64)
    N = w.size
    if w0 is None or wspan is None:
        w0, wspan = grid_frame(w)
    if n_steps is None:
        n_steps = rotation_steps(j, N)
    P = (x.size - 4) // 3
    p0, p1, r, yoff = (float(q) for q in x[:4])
    wj, uj, vj = float(w[j]), float(u[j]), float(v[j])
    phi = mp.mpf(p0) + mp.mpf(p1) * j / N
    cs, sn = mp.cos(phi), mp.sin(phi)
    V = cs * uj - sn * vj
    I = sn * uj + cs * vj
    rot = (abs(uj) + abs(vj)) * (1 + abs(float(phi)) + n_steps)
    Vf, If2 = mp.mpf(0), mp.mpf(0)
    real, im, tr, ti, add = [], [], [], [], []
    far32 = 0.0
    if rec is not None:
        q = (j % CHUNK) // WAVE
        rec = (q, float(w[j - q * WAVE]), rec[0], rec[1])
    for k in range(P):
        re_k, im_k, tr_k, ti_k, f32, add_k = _peak_terms(wj, r, yoff, *x[4 + 3 * k:7 + 3 * k], w0, wspan, imag, chunk, rec)
        add.append(add_k)
        Vf += re_k
        If2 += im_k
        real.append(re_k)
        im.append(im_k)
        tr.append(tr_k)
        ti.append(ti_k)
        far32 += f32
    If1 = im[-1] if P else mp.mpf(0)
    ce = C * EPS
    out = dict(V=float(V), I=float(I), Vf=float(Vf), If1=float(If1), If2=float(If2),
               dV=float(V - Vf), dI1=float(I - If1), dI2=float(I - If2),
               real=np.array([float(q) for q in real]), imag=np.array([float(q) for q in im]),
               tol_real=ce * np.array(tr), tol_imag=ce * np.array(ti),
               far32=C * EPS32 * far32)
    out["tol_V"] = ce * (rot + sum(tr) + float(abs(V)))
    out["tol_I1"] = ce * (rot + (ti[-1] if P else 0.0) + float(abs(I)))
    out["tol_I2"] = ce * (rot + sum(ti) + float(abs(I)))
    out["tol_Vf"] = ce * (sum(tr) + float(abs(Vf)))
    out["tol_If"] = ce * (sum(ti) + float(abs(If2)))
    if rec is not None:
        out["plain"] = {k: out[k] for k in ("tol_real", "tol_V", "tol_Vf")}
        out["tol_real"] = out["tol_real"] + ce * np.array(add)
        out["tol_V"] = out["tol_V"] + ce * sum(add)
        out["tol_Vf"] = out["tol_Vf"] + ce * sum(add)
    return out


def plain_bounds(t):
    """The truth t of point() with its plain bounds in place (t itself when no recurrence term was asked for)."""
    return dict(t, **t["plain"]) if "plain" in t else t


def objective_probe(t, fit_im):
    """What the objective returns with one-hot weights at the probe point, times sqrt(N), and its bound:
    |dV| (fit_im off) or (|dV| + |dI|) / 2 (reference / all-peak imaginary model)."""
    if fit_im in (False, 0, None):
        return abs(t["dV"]), t["tol_V"]
    if fit_im in (True, 1):
        return 0.5 * (abs(t["dV"]) + abs(t["dI1"])), 0.5 * (t["tol_V"] + t["tol_I1"])
    return 0.5 * (abs(t["dV"]) + abs(t["dI2"])), 0.5 * (t["tol_V"] + t["tol_I2"])


class Worst:
    """Tracks the worst err/tol ratio of a test (printed at its end)."""

    def __init__(self, name):
        self.name, self.ratio, self.where = name, 0.0, None
        self.fails = []

    def check(self, got, want, tol, where):
        err = abs(got - want)
        q = err / tol if tol > 0 else (0.0 if err == 0 else math.inf)
        if not q <= self.ratio:
            self.ratio, self.where = q, where
        if not q <= 1.0:
            self.fails.append((q, got, want, tol, where))
        return q

    def report(self):
        print("%s: worst err/tol %.3g at %s" % (self.name, self.ratio, self.where))
        return self.fails

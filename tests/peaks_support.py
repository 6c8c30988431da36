"""
Test infrastructure for the device-batched peak picking (NOT part of the nmrfit_amd package): the numpy restatement of
csrc/peaks.hip's exact steps, an exactly summed truth for its compensated sums, the tolerance a device sum may take
against that truth, and the table of edge cases that tests/test_peaks_cpu.py (no GPU) and tests/test_gpu_peaks_edges.py
share.

``emulate``      the device's plan step by step: W, U, S, the maxima, crossings, width, bounds and index range as exact
                 restatements (they equal the host mirror AutoPeakSelector bit for bit); the means of the baselines and
                 the Simpson terms summed by ``math.fsum`` (exactly rounded), so baseline, height and area are the truth
                 the device's sums are measured against.
``sum_bound``    how far a device sum may lie from the exact one (derived in its docstring, not tuned).
``margin_ok``    the condition on a case's inputs under which device and truth must take the same baseline passes.
``CASES``        the edge cases, each with the path of peaks.hip it is named for (``reaches`` says whether it got there).
"""
import collections
import math
import os
import re

import numpy as np

from nmrfit_amd import peaks, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "nmrfit_amd", "csrc", "peaks.hip")

EPS = float(np.finfo(np.float64).eps)      # 2^-52 = 2 u, u the unit roundoff
TOL = 1e-3                                 # peakutils.baseline: tol
MAX_IT = 100                               # ... max_it
GLOBAL_LANES = 1024                        # stage 2: threads that share a spectrum's sum
LOCAL_LANES = 64                           # stage 3: one wave
SUM_C = 32                                 # sum_bound's second-order constant
TINY = 5e-324                              # the spacing of subnormal numbers: what an operation that underflows may lose


# ---- the device's steps, restated in numpy (the order of every exact operation is peaks.hip's) ------------------------

def interp_np(xs, ys, W):
    """numpy.interp's arithmetic (csrc/peaks.hip: interp_at)."""
    N = len(xs)
    j = np.searchsorted(xs, W, side="right") - 1
    j = np.clip(j, 0, N - 1)
    jj = np.minimum(j, N - 2)
    with np.errstate(all="ignore"):
        slope = (ys[jj + 1] - ys[jj]) / (xs[jj + 1] - xs[jj])
        r = slope * (W - xs[jj]) + ys[jj]
        bad = np.isnan(r)
        r2 = slope * (W - xs[jj + 1]) + ys[jj + 1]
        r = np.where(bad, r2, r)
        r = np.where(np.isnan(r) & bad & (ys[jj] == ys[jj + 1]), ys[jj], r)
    r = np.where(xs[j] == W, ys[j], r)
    return np.where(j == N - 1, ys[N - 1], r)


def _hip_savgol():
    text = open(SRC).read()
    body = re.search(r"kSavgol\[6\]\s*=\s*\{([^}]*)\}", text).group(1)
    return [t.strip() for t in body.split(",")]


def savgol_np(U, edges):
    c = [float.fromhex(h) for h in _hip_savgol()]
    with np.errstate(all="ignore"):
        S = U[5:-5] * c[0]
        for k in (5, 4, 3, 2, 1):
            S = S + (U[5 + k:len(U) - 5 + k] + U[5 - k:len(U) - 5 - k]) * c[k]
    return np.concatenate([edges[:5], S, edges[5:]])


def exact_sum(a):
    """The exactly rounded sum (math.fsum); numpy's NaN / inf where fsum would raise."""
    a = np.asarray(a, dtype=np.float64)
    if not np.isfinite(a).all():
        with np.errstate(all="ignore"):
            return float(np.sum(a))
    try:
        return math.fsum(a.tolist())
    except OverflowError:                       # a finite list whose exact sum is not: the device's plain sum says inf too
        with np.errstate(all="ignore"):
            return float(np.sum(a))


def sum_bound(terms, lanes=LOCAL_LANES, total=None):
    """How far the device's sum of ``terms`` may lie from the exactly rounded one: 2 eps |sum| + 32 n eps^2 sum|x|.

    The device gives every lane the terms k = lane, lane + lanes, ...; a lane adds its m = ceil(n / lanes) terms with
    Neumaier's step (CSum::add): s <- fl(s + v) and the step's rounding error, recovered EXACTLY (the larger operand
    first), goes into c <- fl(c + e).  Lanes are then merged pairwise (CSum::merge: Knuth's two-sum of the s parts, exact
    again; c <- fl(fl(c + c') + e)): 6 merges in a wave, 15 more across the waves of a 1024-thread workgroup.  So at
    every point s + sum(e) is the exact sum of what was added, and the only inexact operations are the additions into c
    and the final fl(s + c).
      * first order: fl(s + c) errs by u |sum| (1 + O(u)); nothing else is first order.  We allow 2 eps |sum| = 4 u |sum|.
      * second order: every e is at most u |s_k| <= u sum|x| (1 + O(mu)).  A chain of L = m + 21 additions into c,
        each losing at most u times the running |c| <= L u sum|x|, loses at most (L u)^2 sum|x| in all, and a tree of
        such chains no more than its longest root-to-leaf chain does.
    The second-order term is written in the linear form c n eps^2 sum|x| with c = 32.  That covers the chain bound
    (L u)^2 = (L eps)^2 / 4 as long as L^2 <= 128 n, which holds for n <= 5e5 terms over 64 lanes and for n up to the
    library's point budget 2^26 over 1024 lanes; outside that range this function raises instead of promising.  The term
    matters only when the terms cancel to below 1e-8 of their magnitudes; without it an exactly zero sum would allow
    nothing.  The constants 2 and 32 are not fitted to any device output.  Additions do not underflow, so the bound needs
    no absolute floor; the divisions and products around a sum do, and their bounds add multiples of TINY = 2^-1074.
    """
    t = np.asarray(terms, dtype=np.float64)
    n = t.size
    if n == 0:
        return 0.0
    L = -(-n // lanes) + 21
    if L * L > 4 * SUM_C * n and L > 22:
        raise ValueError("sum_bound: %d terms over %d lanes is outside the range its derivation covers" % (n, lanes))
    with np.errstate(all="ignore"):
        if total is None:
            total = exact_sum(t)
        mag = float(np.sum(np.abs(t))) * (1.0 + 1e-9)       # (numpy's pairwise sum of positive terms: good to 1e-13)
        return 2.0 * EPS * abs(total) + SUM_C * max(n, L) * EPS * EPS * mag


def neumaier_lanes(x, lanes=LOCAL_LANES):
    """A numpy model of the device's sum (CSum::add per lane over k = lane, lane + lanes, ...; wave_csum's xor butterfly;
    BlockReduce's serial merge of the waves; total())."""
    x = np.asarray(x, dtype=np.float64)
    n = x.size
    m = -(-n // lanes)
    pad = np.zeros(m * lanes)
    pad[:n] = x
    rows = pad.reshape(m, lanes)
    live = (np.arange(m * lanes) < n).reshape(m, lanes)
    s, c = np.zeros(lanes), np.zeros(lanes)
    with np.errstate(all="ignore"):
        for v, on in zip(rows, live):
            t = s + v
            e = np.where(np.abs(s) >= np.abs(v), (s - t) + v, (v - t) + s)
            c = np.where(on, c + e, c)
            s = np.where(on, t, s)

        def merge(s, c, os_, oc):
            t = s + os_
            bb = t - s
            err = (s - (t - bb)) + (os_ - bb)
            return t, (c + oc) + err
        tot_s, tot_c = [], []
        for w0 in range(0, lanes, 64):
            ws, wc = s[w0:w0 + 64].copy(), c[w0:w0 + 64].copy()
            o = 32
            while o > 0:
                idx = np.arange(64) ^ o
                ws, wc = merge(ws, wc, ws[idx], wc[idx])
                o >>= 1
            tot_s.append(ws[0])
            tot_c.append(wc[0])
        rs, rc = tot_s[0], tot_c[0]
        for k in range(1, len(tot_s)):
            rs, rc = merge(rs, rc, tot_s[k], tot_c[k])
        return float(rs + rc) if np.isfinite(rs) else float(rs)


def plain_sum(x, lanes=None):
    """A left-to-right float64 sum (what the device's sums would be without the compensation)."""
    s = 0.0
    with np.errstate(all="ignore"):
        for v in np.asarray(x, dtype=np.float64).tolist():
            s = s + v
    return s


Trace = collections.namedtuple("Trace", "ratios accepted err")
Trace.__doc__ = """One const_baseline run: the ratio |new - c| / |c| of EVERY pass (the one that stopped it included),
the number of accepted passes (0: the first test passed and y[0] came back), and a bound on |device result - truth|."""


def const_baseline_trace(y, sum_fn=exact_sum, lanes=LOCAL_LANES):
    """peakutils.baseline(y, 0)[0] with the device's quirks (the last accepted c; y[0] on a first-test pass) and its trace.

    The error bound follows the passes.  Pass k's mean may be off by b_k = sum_bound(min(y, clip)) / n + eps |mean| (the
    division) plus what an error c_k of the clip moves: only points with y > clip - c_k can change, each by at most c_k,
    so f_k c_k with f_k their fraction.  The clip is a running minimum of accepted means: c_{k+1} = e_k where the new
    mean is below the old clip by more than both errors (the usual, strictly falling, run), max(c_k, e_k) otherwise."""
    y = np.asarray(y, dtype=np.float64)
    n = len(y)
    coef, clip, out = 1.0, np.inf, float(y[0])
    ratios, accepted, out_err, clip_err = [], 0, 0.0, 0.0
    for _ in range(MAX_IT):
        with np.errstate(all="ignore"):
            cl = np.minimum(y, clip)
            tot = sum_fn(cl)
            m = np.float64(tot) / n
            d = m - coef
            ratio = float(np.sqrt(d * d) / np.sqrt(coef * coef))
            if sum_fn is exact_sum and np.isfinite(m):
                frac = np.count_nonzero(y > clip - clip_err) / n if np.isfinite(clip) else 0.0
                e = frac * clip_err + sum_bound(cl, lanes, tot) / n + EPS * abs(m) + 2 * TINY
            else:
                e = 0.0 if sum_fn is not exact_sum else np.nan
        ratios.append(ratio)
        if ratio < TOL:
            break
        coef = out = float(m)
        out_err = e
        accepted += 1
        with np.errstate(all="ignore"):
            sure = not np.isfinite(clip) or m + e < clip - clip_err     # the new mean is the smaller one on both sides
            clip = np.minimum(clip, m)
        clip_err = e if sure or not np.isfinite(e) else max(clip_err, e)
    return out, Trace(ratios, accepted, out_err)


def const_baseline_np(y, mean=None):
    """The value alone; ``mean`` (of an array) replaces the exact mean."""
    if mean is None:
        return const_baseline_trace(y)[0]
    return const_baseline_trace(y, sum_fn=lambda a: mean(a) * len(a))[0]


SimpsonTerms = collections.namedtuple("SimpsonTerms", "pairs corr mag weight")
SimpsonTerms.__doc__ = """scipy.integrate.simpson(y, x=x) term by term in float64, in peaks.hip's order: ``pairs`` the
composite rule's terms (the trapezoid for two points), ``corr`` the three products of the even-count correction
(alpha y[-1], beta y[-2], -eta y[-3]; empty for odd n); ``mag`` the sum of the |products| inside the terms and ``weight``
the sum of the |weights| (what an error of y moves the area by)."""


def simpson_terms(y, x):
    y = np.asarray(y, dtype=np.float64)
    x = np.asarray(x, dtype=np.float64)
    n = len(y)
    none = np.zeros(0)
    if n < 2:
        return SimpsonTerms(none, none, 0.0, 0.0)
    with np.errstate(all="ignore"):
        if n == 2:
            h = x[1] - x[0]
            return SimpsonTerms(np.array([0.5 * h * (y[1] + y[0])]), none, float(abs(0.5 * h) * (abs(y[1]) + abs(y[0]))),
                                float(abs(h)))
        npairs = (n - 1) // 2 if n % 2 == 1 else (n - 2) // 2
        i = 2 * np.arange(npairs)
        h0, h1 = x[i + 1] - x[i], x[i + 2] - x[i + 1]
        hsum, hprod = h0 + h1, h0 * h1
        r = np.divide(h0, h1, out=np.zeros_like(h0), where=h1 != 0)
        inv = np.divide(1.0, r, out=np.zeros_like(r), where=r != 0)
        q = np.divide(hsum, hprod, out=np.zeros_like(hsum), where=hprod != 0)
        a, b, c = 2.0 - inv, hsum * q, 2.0 - r
        pairs = hsum / 6.0 * ((y[i] * a + y[i + 1] * b) + y[i + 2] * c)
        mag = exact_sum(np.abs(hsum / 6.0) * (np.abs(y[i] * a) + np.abs(y[i + 1] * b) + np.abs(y[i + 2] * c)))
        weight = exact_sum(np.abs(hsum / 6.0) * (np.abs(a) + np.abs(b) + np.abs(c)))
        corr = none
        if n % 2 == 0:
            g0, g1 = x[n - 2] - x[n - 3], x[n - 1] - x[n - 2]
            den = 6.0 * (g1 + g0)
            alpha = (2.0 * (g1 * g1) + (3.0 * g0) * g1) / den if den != 0 else 0.0
            den = 6.0 * g0
            beta = (g1 * g1 + (3.0 * g0) * g1) / den if den != 0 else 0.0
            den = (6.0 * g0) * (g0 + g1)
            eta = np.float64(g1) ** 3 / den if den != 0 else 0.0
            corr = np.array([alpha * y[n - 1], beta * y[n - 2], -(eta * y[n - 3])])
            mag += float(np.abs(corr).sum())
            weight += float(abs(alpha) + abs(beta) + abs(eta))
    return SimpsonTerms(pairs, corr, float(mag), float(weight))


def simpson_exact(st):
    return exact_sum(np.concatenate([st.pairs, st.corr]))


def area_bound(st, base_err):
    """|device area - truth|.  The pair terms: sum_bound.  An even count adds, on the device, result + ((a + b) + c) of
    the three correction products: two additions that each lose at most u (|a| + |b| + |c|) and one that loses u |area|
    (allowed: eps each), and the device's pow(h1, 3.0) inside eta is not correctly rounded (allowed: 2 ulp of the product
    eta |y|).  The local baseline the ordinates are taken above may itself be off by ``base_err``: that moves the area by
    base_err times the sum of the |weights|, and, the ordinates then being different float64 numbers, every term is
    rounded afresh: 8 roundings of at most u (or, underflowing, TINY) on products whose magnitudes sum to ``mag``."""
    with np.errstate(all="ignore"):
        b = sum_bound(st.pairs)
        if st.corr.size:
            c = float(np.abs(st.corr).sum())
            b += 2.0 * EPS * c + EPS * abs(simpson_exact(st)) + 2.0 * EPS * abs(st.corr[2])
        b += 4 * TINY
        if base_err > 0:
            b += base_err * st.weight * (1.0 + 8.0 * EPS) + 8.0 * EPS * st.mag + 8 * (st.pairs.size + 1) * TINY
        elif not base_err == 0:
            b = np.nan
    return float(b)


def nearest(cands, W, loc):
    if cands.size == 0:
        return None
    d = np.abs(W[cands] - loc)
    return cands[np.argmin(d)]


Emulated = collections.namedtuple("Emulated", "peaks B U S W order M trace candidates")
Emulated.__doc__ = """emulate's result.  ``peaks``: a dict per measured peak (i, loc, width, bounds, lo, hi, n, jr, jf =
the rising and falling crossing, baseline, height, area, trace, and the bounds base_err, height_err, area_err on the
device's distance from them).  ``B``, ``trace``: the global baseline and its passes (trace.err bounds the device's
distance).  ``candidates``: every maximum of S over +-order as (i, U[i] - B, fate, tie), fate one of "thresh", "no
crossing", "crossings in the wrong order", "peak"; tie: two crossings of one kind equally near (the lower index wins)."""


def emulate(w, u, thresh, window, sum_fn=exact_sum):
    """The device's plan on (w, u); ``sum_fn`` sums an array (the default: exactly)."""
    xs, ys, edges, order, M = peaks._prepare(w, u, window)
    W = peaks.grid_points(xs[0], xs[-1], M, np.arange(M))
    U = interp_np(xs, ys, W)
    S = savgol_np(U, edges)
    B, gtrace = const_baseline_trace(S, sum_fn, GLOBAL_LANES)
    out, cands = [], []
    for i in peaks.argrelmax(S, order):
        with np.errstate(all="ignore"):
            h = U[i] - B
        if not h > thresh:
            cands.append((int(i), float(h), "thresh", False))
            continue
        with np.errstate(all="ignore"):
            side = np.sign(h / 2.0 - (U - B))
        cr = side[:-1] - side[1:]
        falling, rising = np.flatnonzero(cr < 0), np.flatnonzero(cr > 0)
        jf, jr = nearest(falling, W, W[i]), nearest(rising, W, W[i])
        if jf is None or jr is None:
            cands.append((int(i), float(h), "no crossing", False))
            continue
        tie = any(np.count_nonzero(np.abs(W[c] - W[i]) == abs(W[j] - W[i])) > 1 for c, j in ((falling, jf), (rising, jr)))
        if not W[jr] < W[jf]:
            cands.append((int(i), float(h), "crossings in the wrong order", tie))
            continue
        cands.append((int(i), float(h), "peak", tie))
        width = W[jf] - W[jr]
        b = [W[i] - 2 * width, W[i] + 2 * width]
        sel = np.flatnonzero((W >= b[0]) & (W <= b[1]))
        pb, tr = const_baseline_trace(U[sel], sum_fn, LOCAL_LANES)
        with np.errstate(all="ignore"):
            st = simpson_terms(U[sel] - pb, W[sel])
            height = U[i] - pb
        area = float(sum_fn(np.concatenate([st.pairs, st.corr]))) if sum_fn is exact_sum else _device_simpson(st, sum_fn)
        out.append(dict(i=i, loc=W[i], width=width, bounds=b, lo=int(sel[0]), hi=int(sel[-1]), n=int(sel.size),
                        jr=int(jr), jf=int(jf), baseline=pb, height=height, area=area, trace=tr, base_err=tr.err,
                        height_err=tr.err + EPS * abs(height) + TINY, area_err=area_bound(st, tr.err)))
    return Emulated(out, B, U, S, W, order, M, gtrace, cands)


def _device_simpson(st, sum_fn):
    """The device's order: the pair terms by ``sum_fn``, then result + ((a + b) - c)."""
    r = np.float64(sum_fn(st.pairs))
    if st.corr.size:
        r = r + ((st.corr[0] + st.corr[1]) + st.corr[2])
    return float(r)


def margin_ok(trace, margin=1e-9):
    """True when no pass of the trace lands within ``margin`` (relative) of the tolerance 1e-3.  Device and truth differ
    in the last bits of a mean; a pass that close to the tolerance could legitimately stop on one side and go on on the
    other, which moves the baseline by about 1e-3.  A condition on a case's inputs, not a tolerance on its outputs."""
    return all(not abs(r - TOL) <= margin * TOL for r in trace.ratios)


def thresh_margin_ok(em, thresh, margin=1e-9):
    """No candidate's height within ``margin`` of the threshold (relative to the larger of the two and max|U|)."""
    fin = np.abs(em.U[np.isfinite(em.U)])
    scale = float(fin.max()) if fin.size else 0.0
    return all(not abs(h - thresh) <= margin * max(abs(h), abs(thresh), scale) for _, h, _, _ in em.candidates
               if np.isfinite(h))


def close(a, b, scale, rel=1e-12):
    return abs(a - b) <= rel * max(abs(b), scale)


# ---- the edge cases -----------------------------------------------------------------------------------------------------

def grid_step(w, N=None):
    w = np.asarray(w, dtype=float)
    W01 = peaks.grid_points(w.min(), w.max(), 100 * len(w), [0, 1])
    return W01[1] - W01[0]


def window_for(w, order):
    """A window that AutoPeakSelector turns into exactly this ``order`` on w's grid."""
    step = grid_step(w)
    window = (order + 0.5) * step
    assert int(window / step) == order
    return window


def tents(N, heights, floor=0.0, lo=0.0, hi=1.0):
    """N uniform knots, u = floor + heights[knot]: triangles two knot intervals (about 202 grid points) wide."""
    w = np.linspace(lo, hi, N)
    u = np.full(N, float(floor))
    for k, v in heights.items():
        u[k] += v
    return w, u


def on_grid(points, lo=0.0, hi=1.0):
    """Knots placed ON points of the upsampled grid: ``points`` maps a grid index (negative: from the end) to an
    ordinate; the spectrum has as many knots as entries, so M = 100 len(points), and must name the indices 0 and -1.
    U is then known point by point at those indices and linear between them."""
    N = len(points)
    M = 100 * N
    idx = np.array(sorted(k % M for k in points))
    assert idx[0] == 0 and idx[-1] == M - 1 and len(set(idx)) == N
    val = {k % M: v for k, v in points.items()}
    w = peaks.grid_points(lo, hi, M, idx)
    return w, np.array([float(val[k]) for k in idx])


def lines(N, P, seed, lo=0.0, hi=1.0, offset=0.0, noise=0.0):
    sp = synth.make_spectrum(N, P, seed=seed, noise=noise, w_lo=lo, w_hi=hi)
    return sp["w"] + offset, sp["u"]


def reverse(wu):
    return wu[0][::-1].copy(), wu[1][::-1].copy()


EVEN_SEED = 4                                       # lines(256, 2, seed): a peak with an even count inside the spectrum
BASE = dict(N=12, heights={3: 1.0, 8: 0.6})        # two clean tents: the spectrum the baseline cases scale and shift

Case = collections.namedtuple("Case", "name make thresh order window tags host_sums cpu_make sums_only")


def _case(name, make, tags, thresh=0.1, order=None, window=None, host_sums=True, cpu_make=None, sums_only=False):
    assert (order is None) != (window is None)
    return Case(name, make, thresh, order, window, tuple(tags), host_sums, cpu_make, sums_only)


def case_inputs(case, cpu=False):
    """(w, u, thresh, window) of a case; ``cpu``: at the size the CPU tier affords."""
    w, u = (case.cpu_make if cpu and case.cpu_make else case.make)()
    window = case.window if case.order is None else window_for(w, case.order)
    return w, u, case.thresh, window


def _far_fall(D, rise=30):
    """A maximum at grid index 400 whose falling crossing lies exactly D points to its right: U falls slowly to 0.9 at
    400 + D and to 0 one point later; the rising crossing is within ``rise`` points on the left."""
    return lambda: on_grid({0: 0.0, 400 - rise: 0.0, 400: 1.0, 400 + D: 0.9, 401 + D: 0.0, -1: 0.0, 900: 0.0, 950: 0.0})


def _far_rise(D):
    """The mirror image: the rising crossing exactly D + 1 points to the left of the maximum at 500."""
    return lambda: on_grid({0: 0.0, 100: 0.0, 499 - D: 0.0, 500 - D: 0.9, 500: 1.0, 530: 0.0, 700: 0.0, -1: 0.0})


def _shoulder():
    # a tall line, a narrow dip below the shoulder's half height, the shoulder (maximum at 380), a long slow decline:
    # the nearest falling crossing is the dip's left wall, LEFT of the nearest rising crossing (its right wall)
    return on_grid({0: 0.0, 300: 2.0, 360: 1.9, 365: 0.0, 370: 0.0, 380: 1.0, 700: 0.8, 705: 0.0, 800: 0.0, -1: 0.0})


def _tie():
    # a grid step of exactly 2^-10, so distances are exact: the maximum at 500, falling crossings at 460 (the right wall of a
    # tall neighbour) and at 540, both 40 steps away; the rising crossing between 480 and 494.  np.argmin takes the lower
    # index, 460, which lies LEFT of the rising crossing: the host skips the peak
    return on_grid({0: 0.0, 200: 2.0, 460: 1.9, 461: 0.0, 480: 0.0, 494: 0.94, 500: 1.0, 506: 0.94, 540: 0.9, 541: 0.0,
                    -1: 0.0}, hi=1099.0 / 1024.0)


def _dup():
    w = np.array([0.0, 1.0, 2.0, 2.0, 3.0, 4.0, 5.0, 5.0, 6.0, 7.0])
    u = np.array([0.0, 0.2, 1.0, 0.7, 0.1, 0.0, 0.3, 0.6, 0.1, 0.0])
    return w, u


def _with(make, k, v):
    def f():
        w, u = make()
        u = u.copy()
        u[k] = v
        return w, u
    return f


_B = lambda scale=1.0, shift=0.0: (lambda: (lambda w, u: (w, scale * u + shift))(*tents(**BASE)))   # noqa: E731
_T = lambda N, heights, **kw: (lambda: tents(N, heights, **kw))                                       # noqa: E731

CASES = [
    # 1. simpson_area, even count: bounds clipped by an end of the spectrum, or a rounding
    _case("clipped left", _T(8, {1: 1.0}), ["clip_left", "peak"], order=150),
    _case("clipped right", _T(8, {6: 1.0}), ["clip_right", "peak"], order=150),
    _case("clipped both, N=3", lambda: (np.array([0.0, 0.45, 1.0]), np.array([0.0, 1.0, 0.0])), ["clip_left", "clip_right", "even", "peak"], order=100),
    _case("even count inside", lambda: lines(256, 2, seed=EVEN_SEED), ["even_inside", "peak"], window=0.02),
    # 2. an abscissa whose ulp is about the grid step
    _case("offset 2^38", lambda: lines(256, 2, seed=1, offset=2.0 ** 38), ["coincident", "order=327", "peak"], window=0.02),
    _case("offset 2^38 descending", lambda: reverse(lines(256, 2, seed=1, offset=2.0 ** 38)), ["coincident", "peak"],
          window=0.02),
    _case("offset 2^37", lambda: lines(256, 2, seed=1, offset=2.0 ** 37), ["quantised", "peak"], window=0.02),
    _case("offset 2^37 descending", lambda: reverse(lines(256, 2, seed=1, offset=2.0 ** 37)), ["quantised", "peak"],
          window=0.02),
    # 3. slot geometry
    _case("order 1", _T(10, {3: 1.0, 6: 0.5}), ["order=1", "peak"], order=1),
    _case("order 2", _T(10, {3: 1.0, 6: 0.5}), ["order=2", "peak"], order=2),
    _case("order 63", _T(10, {3: 1.0, 6: 0.5}), ["order=63", "peak"], order=63),
    _case("order 64", _T(10, {3: 1.0, 6: 0.5}), ["order=64", "peak"], order=64),
    _case("order 65", _T(10, {3: 1.0, 6: 0.5}), ["order=65", "peak"], order=65),
    _case("slots divide M-1", _T(10, {3: 1.0, 6: 0.5}), ["rem=0", "peak"], order=36),          # 999 = 27 * 37
    _case("full last slot", _T(10, {3: 1.0, 6: 0.5}), ["rem=order", "peak"], order=39),       # 1000 = 25 * 40
    _case("maximum on a slot's first point", lambda: on_grid({0: 0.0, 170: 0.0, 200: 1.0, 230: 0.0, 400: 0.0, -1: 0.0}),
          ["slot_first", "peak"], order=99),
    _case("maximum on a slot's last point", lambda: on_grid({0: 0.0, 169: 0.0, 199: 1.0, 229: 0.0, 400: 0.0, -1: 0.0}),
          ["slot_last", "peak"], order=99),
    _case("maximum at i = 1", lambda: on_grid({0: 0.0, 1: 1.0, 2: 0.0, 3: 0.0, -1: 0.0}), ["i=1", "cross_at_i", "clip_left",
                                                                                            "even", "peak"], order=3),
    _case("maximum at i = M-2", lambda: on_grid({0: 0.0, -4: 0.0, -3: 0.0, -2: 1.0, -1: 0.0}), ["i=M-2", "cross_at_i",
                                                                                                 "clip_right", "peak"], order=3),
    _case("plateau", _T(8, {3: 1.0, 4: 1.0}), ["plateau"], order=150),
    _case("two maxima order-1 apart", _T(12, {3: 1.0, 5: 0.8}), ["close_pair", "peak"], order=219),
    # 4. the crossing search
    _case("falling crossing 64 away", _far_fall(66), ["fall=64", "peak"], order=20),
    _case("falling crossing 65 away", _far_fall(67), ["fall=65", "peak"], order=20),
    _case("falling crossing 4*64 away", _far_fall(260), ["fall>256", "peak"], order=20),
    _case("rising crossing 63 away", _far_rise(64), ["rise=63", "peak"], order=20),
    _case("rising crossing 64 away", _far_rise(65), ["rise=64", "peak"], order=20),
    _case("rising crossing 4*64 away", _far_rise(260), ["rise>256", "peak"], order=20),
    _case("shoulder: crossings in the wrong order", _shoulder, ["skip_order"], order=8),
    _case("two falling crossings equally near", _tie, ["tie", "skip_order"], order=8),
    _case("starts above half height", _T(8, {0: 0.9, 1: 1.0}), ["skip_nocross"], order=50),
    _case("spike: crossing at j = i", lambda: on_grid({0: 0.0, 299: 0.0, 300: 1.0, 301: 0.0, 500: 0.0, -1: 0.0}),
          ["cross_at_i", "local<64", "peak"], order=10),
    # 5. const_baseline
    _case("mean within 1e-3 of 1.0", _T(20, {10: 0.3}, floor=0.985), ["first_pass", "peak"], order=150),
    _case("all negative", _B(1.0, -2.0), ["negative", "peak"], order=150),
    _case("1e200 u", _B(1e200), ["passes=100", "peak"], thresh=1e199, order=150),
    _case("1e-300 u", _B(1e-300), ["passes=100", "peak"], thresh=1e-301, order=150),
    _case("1e-310 u", _B(1e-310), ["passes=100", "subnormal", "peak"], thresh=1e-311, order=150, host_sums=False),
    _case("constant", lambda: (np.linspace(0.0, 1.0, 9), np.full(9, 0.7)), ["nopeaks", "plateau"], order=150),
    _case("N=2", lambda: (np.array([0.0, 1.0]), np.array([0.25, 1.0])), ["nopeaks", "M<1024"], order=20),
    _case("N=3", lambda: (np.array([0.0, 0.45, 1.0]), np.array([0.1, 1.1, 0.1])), ["M<1024", "peak"], order=20),
    _case("N=5", _T(5, {1: 1.0}, floor=0.1), ["M<1024", "peak"], order=20),
    _case("N=10", _T(10, {4: 1.0}, floor=0.1), ["M<1024", "peak"], order=20),
    _case("N=11", _T(11, {4: 1.0}, floor=0.1), ["peak"], order=20),
    # 6. awkward axes through the whole pipeline
    _case("duplicate abscissae", _dup, ["duplicate", "peak"], order=50),
    _case("one huge gap", lambda: (np.array([0.0, 1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 1e6]),
                                   np.array([0.0, 0.1, 1.0, 0.2, 0.1, 0.0, 0.0, 0.5])), ["gap"], order=50),
]

# non-finite ordinates: no peaks, the baseline NaN as on the host
for _name, _k, _v in (("+inf", 5, np.inf), ("-inf", 5, -np.inf), ("NaN first", 0, np.nan), ("NaN last", -1, np.nan),
                      ("NaN on a slot boundary", 4, np.nan)):
    CASES.append(_case(_name, _with(_B(), _k, _v), ["nopeaks", "nan_baseline"], order=100))

# the large one: the 6.5 M-point global mean against math.fsum; on the CPU at 4096 points
LARGE = _case("65536 points, 24 lines", lambda: (lambda sp: (sp["w"], sp["u"]))(synth.make_spectrum(65536, 24, seed=3)),
              ["peak"], window=0.02, sums_only=True,
              cpu_make=lambda: (lambda sp: (sp["w"], sp["u"]))(synth.make_spectrum(4096, 6, seed=3)))

BY_NAME = {c.name: c for c in CASES + [LARGE]}
assert len(BY_NAME) == len(CASES) + 1


def reaches(tag, em, case):
    """Whether the emulated case got to the path of peaks.hip that ``tag`` names."""
    P, M, W = em.peaks, em.M, em.W
    slot = em.order + 1
    if tag == "peak":
        return len(P) > 0
    if tag == "nopeaks":
        return len(P) == 0
    if tag == "even":
        return any(p["n"] % 2 == 0 and p["n"] > 2 for p in P)
    if tag == "even_inside":
        return any(p["n"] % 2 == 0 and p["lo"] > 0 and p["hi"] < M - 1 for p in P)
    if tag == "clip_left":
        return any(p["lo"] == 0 and p["bounds"][0] < W[0] for p in P)
    if tag == "clip_right":
        return any(p["hi"] == M - 1 and p["bounds"][1] > W[-1] for p in P)
    if tag == "coincident":
        return all((np.diff(W[p["lo"]:p["hi"] + 1]) == 0).any() for p in P) and any(p["n"] % 2 == 0 for p in P)
    if tag == "quantised":
        d = np.diff(W)
        return (d > 0).all() and len(np.unique(d)) <= 3 and float(np.spacing(W[0])) * 4 > d.min()
    if tag.startswith("order="):
        return em.order == int(tag[6:])
    if tag == "rem=0":
        return (M - 1) % slot == 0
    if tag == "rem=order":
        return (M - 1) % slot == em.order
    if tag == "slot_first":
        return any(p["i"] % slot == 0 for p in P)
    if tag == "slot_last":
        return any(p["i"] % slot == em.order for p in P)
    if tag == "i=1":
        return any(p["i"] == 1 for p in P)
    if tag == "i=M-2":
        return any(p["i"] == M - 2 for p in P)
    if tag == "plateau":                          # a slot whose largest value is taken twice
        S = em.S
        for b0 in range(0, M, slot):
            s = S[b0:b0 + slot]
            if np.count_nonzero(s == s.max()) > 1:
                return True
        return False
    if tag == "close_pair":                       # two maxima of their own slots, order - 1 apart, in adjacent slots
        S, keep = em.S, [p["i"] for p in P]
        tops = [b0 + int(np.argmax(S[b0:b0 + slot])) for b0 in range(0, M, slot)]
        return any(b - a == em.order - 1 and ((a in keep) != (b in keep)) for a, b in zip(tops, tops[1:]))
    if tag.startswith("fall") or tag.startswith("rise"):
        d = [(p["jf"] - p["i"]) if tag.startswith("fall") else (p["i"] - p["jr"]) for p in P]
        return any(x == int(tag[5:]) if tag[4] == "=" else x > int(tag[5:]) for x in d)
    if tag == "cross_at_i":
        return any(p["jf"] == p["i"] for p in P)
    if tag == "local<64":
        return any(p["n"] < 64 for p in P)
    if tag == "skip_order":
        return any(f == "crossings in the wrong order" for _, _, f, _ in em.candidates)
    if tag == "skip_nocross":
        return any(f == "no crossing" for _, _, f, _ in em.candidates)
    if tag == "tie":                              # ... and the tie decided the candidate's fate
        return any(t and f == "crossings in the wrong order" for _, _, f, t in em.candidates)
    if tag == "first_pass":
        return em.trace.accepted == 0 and em.B == em.S[0]
    if tag == "negative":
        return (em.U < 0).all() and em.B < 0
    if tag == "passes=100":
        return len(em.trace.ratios) == MAX_IT
    if tag == "subnormal":
        return 0 < np.abs(em.U).max() < np.finfo(np.float64).tiny
    if tag == "M<1024":
        return M < 1024
    if tag == "duplicate":
        w = np.sort(case_inputs(case)[0])
        return (np.diff(w) == 0).any()
    if tag == "gap":
        w = np.sort(case_inputs(case)[0])
        return np.diff(w).max() > 1e5 * np.median(np.diff(w))
    if tag == "nan_baseline":
        return bool(np.isnan(em.B))
    raise KeyError(tag)


def all_margins_ok(em, thresh):
    return margin_ok(em.trace) and all(margin_ok(p["trace"]) for p in em.peaks) and thresh_margin_ok(em, thresh)


# ---- stage 1 alone: (name, w, u) for smooth_many against interp1d + savgol_filter ------------------------------------------

def smooth_cases():
    rng = np.random.default_rng(17)
    out = []
    w = np.array([0.0, 1.0, 1.0, 1.0, 2.0, 3.0, 3.0, 4.0])
    out.append(("duplicate abscissae, different ordinates", w, rng.standard_normal(8)))
    w = np.concatenate([np.linspace(0.0, 1.0, 15), [1e6]])
    out.append(("one gap of 1e6 spans", w, rng.standard_normal(16)))
    out.append(("wmin == wmax", np.full(4, 2.5), rng.standard_normal(4)))
    out.append(("a span of one subnormal", np.array([0.0, 5e-324]), np.array([1.0, 2.0])))
    out.append(("N = 3", np.array([0.0, 0.3, 1.0]), np.array([1.0, -2.0, 0.5])))
    out.append(("float32 input", np.linspace(3.0, 4.0, 50).astype(np.float32), rng.standard_normal(50).astype(np.float32)))
    big_w, big_u = np.linspace(-1.0, 1.0, 200), rng.standard_normal(200)
    out.append(("a non-contiguous view", big_w[::2], big_u[::2]))
    return out

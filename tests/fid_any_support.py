"""
What the tests of the any-length FID transform share (NOT part of the nmrfit_amd package): the bar, the raw call, the
mixed batch of the purity and fresh-memory tests, and the driver of the poisoned-allocation children,

    python -m tests.fid_any_support poison OUT.npz

THE TRUTH is fid.bluestein_host / fid.condition_host on np.clongdouble (numpy >= 2.0 transforms in the 80-bit format).

THE BAR is include/nmrfit_amd_fid_any.h's, first order, per trace, with eta (Higham Thm 24.2) and kappa (Lemma 3.5) of
tests/fid_support.py and tests/fid_cond_support.py, M = 2^m >= 2 N - 1, eps = log2(M) eta:
    || Y^ - Y ||_2 <= ( beta (2 eps + 2 kappa + sqrt(2) gamma_2) + (eps + mu) sqrt(n_in' (2 N - 1)) ) ||x'||_2
                      + beta || x'^ - x' ||_2          (the conditioned trace's own bar: form 1, the window)
beta = max_k |fft_M(b)[k]| is computed from the definition's b in long double on the host (fid.filter_peak), never from
device output.  Every single point is held to the same absolute amount.  No measured constant.
"""
import os
import sys

import numpy as np

from nmrfit_amd import fid
from tests import fid_cond_support as fc
from tests import fid_support as fs

U = fs.U
# the lengths of the device tests: the shortest, a small prime, an even composite, 1000, the last with M = 4096 (the
# LDS-resident transform), the first with M = 8192 (the two-pass transform), a prime, a round number
LENGTHS = (3, 7, 12, 1000, 2047, 2049, 4099, 5000)


def bar(x, N, mu=fs.MU_DEVICE, conditioned_bar=0.0):
    """The absolute bar on || Y^ - Y ||_2 per trace of x (T, n_in') as it enters the transform of length N;
    ``conditioned_bar``: the bar on || x'^ - x' ||_2 per trace (0 for an input given exactly)."""
    x = np.asarray(x).reshape(-1, np.shape(x)[-1])
    n_in = x.shape[-1]
    M = fid.conv_length(N)
    eta, kappa = fs.eta(mu), mu + np.sqrt(2.0) * fc.GAMMA2 * (1.0 + mu)
    eps, beta = np.log2(M) * eta, fid.filter_peak(N)
    norm = np.sqrt((np.abs(x.astype(np.clongdouble)) ** 2).sum(axis=-1)).astype(np.float64)
    rel = beta * (2.0 * eps + 2.0 * kappa + np.sqrt(2.0) * fc.GAMMA2) + (eps + mu) * np.sqrt(n_in * (2.0 * N - 1.0))
    return rel * norm + beta * conditioned_bar


def truth(x, N):
    """Y (T, N) of x' given exactly: the definition in long double."""
    return fid.bluestein_host(np.asarray(x).astype(np.clongdouble), N)


def raw_call(L, n_in, n, T, x, form, g, window_of, windows, device=0, entry="nmrfit_fid_transform_any"):
    """An entry point with nmrfit_fid_condition_transform's arguments on numpy arrays: (rc, u, v, rows, Z, C)."""
    from nmrfit_amd import _cabi
    p = _cabi.ptr
    n_in, n = np.asarray(n_in, dtype=np.int64), np.asarray(n, dtype=np.int64)
    T, form, window_of = (np.asarray(a, dtype=np.int32) for a in (T, form, window_of))
    g = np.asarray(g, dtype=np.float64)
    K = len(n_in)
    wl = np.array([len(w) for w in windows], dtype=np.int64)
    wf = np.concatenate([np.asarray(w, dtype=np.float64) for w in windows]) if len(windows) else None
    points, values = int(n.sum()), int((T * n).sum())
    refused_early = values > 1 << 26                             # (over the budget: refused, nothing is written)
    u, v = (np.zeros(1), np.zeros(1)) if refused_early else (np.zeros(points), np.zeros(points))
    rows = np.zeros(K * fid.ROW)
    Z = np.zeros(1 if refused_early else 2 * values)
    C = np.zeros(2 * int((T * n_in).sum()))                      # (at least as long as the conditioned traces)
    rc = getattr(L, entry)(device, K, p(n_in), p(n), p(T), p(np.ascontiguousarray(x)), p(form), p(g), p(window_of), len(windows),
                           p(wl) if len(windows) else None, p(wf), p(u), p(v), p(rows), p(Z), p(C))
    return rc, u, v, rows, Z, C


# ---- ties across the chunks of the partial maxima --------------------------------------------------------------------

# (name, n, T, placements of the larger trace).  A partial maximum is over 8192 values of a spectrum's Z: 700 traces of 12
# points (a finish-only job: the point within the trace is a remainder) are 8400 values, and flat value 8192 is point 8 of
# trace 682, which straddles the chunks; 1100 traces of 8 points (the mask) are 8800 values with the boundary at trace 1024.
TIES = (("A", 12, 700, ((5, 682, 699), (682, 699), (699,))),
        ("B", 8, 1100, ((5, 1024, 1099), (1024, 1099), (1099,))))


def tie_stack(lo, T, hi_at):
    """T copies of the row ``lo`` with 3 * lo at the traces ``hi_at``: equal traces tie in every value."""
    x = np.repeat(np.asarray(lo).reshape(1, -1), T, axis=0)
    x[list(hi_at)] = 3.0 * x[0]
    return x


# ---- the mixed batch -----------------------------------------------------------------------------------------------------

def mixed_jobs():
    """(x, g, mode, W, zero_fill) jobs that reach every new piece of the call's device block: chirp jobs with the
    LDS-resident and the two-pass M, T = 1 and 3, zero fill (n_in' < N), two jobs sharing one N and one job with that N
    alone in its own call (the tests run each alone), form 1 into an exact length with and without a window, a window
    alone -- among power-of-two jobs of every form."""
    W = fid.window_em(4096 - 69, 3.0, 4096.0, first_point=0.5)
    return [(fs.sample_fid(1000, 1, seed=70), None, "fid", None, None),
            (fs.sample_fid(512, 2, seed=71), None, "fid", None, "pow2"),
            (fs.sample_fid(900, 3, seed=72), None, "fid", None, 1000),                # shares N = 1000; zero fill
            (fs.sample_fid(4096, 1, seed=73), 67.98416137695312, "fid", None, None),  # Bruker: N = 4027, M = 8192
            (fs.sample_fid(4096, 3, seed=74), 67.98416137695312, "fid", W, None),
            (fs.sample_fid(8192, 1, seed=75), 5.0, "fid", None, "pow2"),
            (fs.sample_fid(1000, 1, seed=76), 68.0, "spectrum", None, "pow2"),
            (fs.sample_fid(2047, 2, seed=77), None, "fid", fid.window_sine(2047, 0.0, 0.95, 2.0), None),   # M = 4096
            (fs.sample_fid(5000, 1, seed=78), None, "fid", None, None),               # M = 16384
            (fs.sample_fid(7, 1, seed=79), None, "fid", None, None),
            (fs.sample_fid(256, 1, seed=80), 4.0, "fid", None, 300)]                  # form 1, zero fill to N = 300


def run_jobs(jobs, **kw):
    """(x, g, mode, W, zero_fill) jobs in ONE library call, each at the length fid.transform_length(any_length=True) gives
    its zero_fill: (u, v, row, Y, xc) per job."""
    ns = []
    for x, g, mode, W, zf in jobs:
        n_out = fid.conditioned_length(x.shape[-1], g, mode) if g is not None else x.shape[-1]
        ns.append(fid.transform_length(n_out, zf, any_length=True))
    return run_lengths(jobs, ns, **kw)


def run_lengths(jobs, ns, **kw):
    """One library call with a transform length per job (transform_many takes one zero_fill: the raw entry point does
    the ragged batch)."""
    from nmrfit_amd import _cabi
    L = _cabi.lib()
    windows, window_of = [], []
    for j in jobs:
        if j[3] is None:
            window_of.append(-1)
        else:
            window_of.append(len(windows))
            windows.append(np.asarray(j[3], dtype=np.float64))
    xs = [fid._as_traces(j[0]) for j in jobs]
    form = [fid.FORM_NONE if j[1] is None else fid._MODES[j[2]] for j in jobs]
    g = [0.0 if j[1] is None else j[1] for j in jobs]
    n_in, T = [x.shape[1] for x in xs], [x.shape[0] for x in xs]
    n_out = [fid.conditioned_length(x.shape[1], j[1], j[2]) if j[1] is not None else x.shape[1] for x, j in zip(xs, jobs)]
    flat = np.concatenate([x.ravel() for x in xs]).view(np.float64)
    rc, u, v, rows, Z, C = raw_call(L, n_in, ns, T, flat, form, g, window_of, windows, **kw)
    _cabi.check(rc)
    out, au, az, ac = [], 0, 0, 0
    for k in range(len(jobs)):
        n, t, m = ns[k], T[k], n_out[k]
        z = Z[2 * az:2 * (az + t * n)].view(np.complex128).reshape(t, n)
        c = C[2 * ac:2 * (ac + t * m)].view(np.complex128).reshape(t, m)
        out.append((u[au:au + n].copy(), v[au:au + n].copy(), rows[k * fid.ROW:(k + 1) * fid.ROW].copy(), z[:, ::-1].copy(), c.copy()))
        au, az, ac = au + n, az + t * n, ac + t * m
    return out


def poison_run(out):
    """The mixed batch with every output asked for.  Host outputs start as zeros the library overwrites; every value of
    a status-0 job is finite."""
    arrays = {}
    full = run_jobs(mixed_jobs())
    for k, f in enumerate(full):
        arrays["u%d" % k], arrays["v%d" % k], arrays["row%d" % k] = f[0], f[1], f[2]
        arrays["Y%d" % k], arrays["C%d" % k] = f[3].view(np.float64), f[4].view(np.float64)
        assert f[2][0] == 0 and all(np.isfinite(np.asarray(a).view(np.float64)).all() for a in f), k
    arrays["__poison__"] = np.array(os.environ.get("NMRFIT_POISON_ALLOC", ""))
    np.savez(out, **arrays)


if __name__ == "__main__":
    if len(sys.argv) != 3 or sys.argv[1] != "poison":
        sys.exit("usage: python -m tests.fid_any_support poison OUT.npz")
    poison_run(sys.argv[2])

"""
What the tests of the FID conditioning share (NOT part of the nmrfit_amd package): the bars, the group delays, the mixed
batch of the purity and fresh-memory tests, and the driver of the poisoned-allocation children,

    python -m tests.fid_cond_support poison OUT.npz

NO PARITY WITH nmrglue is claimed or tested: it is not installed where these tests run.  The definition is the one of
include/nmrfit_amd_fid_cond.h; nmrfit_amd.fid.condition_host restates it in numpy, tests/test_fid_cond_cpu.py holds that
restatement to the definition independently (a long-double DFT matrix, circular shifts), and THE TRUTH of the device
tests is condition_host on np.clongdouble.

THE BARS are the header's, first order, from Higham Thm 24.2 (eta, tests/fid_support.py) and Lemma 3.5 (a complex
product: sqrt(2) gamma_2), with the ramp values within mu = u of the exact ones:
    kappa = mu + sqrt(2) gamma_2 (1 + mu)                               a product with a ramp value
    conditioned trace   (2 log2(s) eta + kappa + 2u) F max|W| ||x||_2    form 1; F = sqrt(2) with a fold (add > 0), else 1
                        u max|W| ||x||_2 with a window alone, 0 without
    spectrum            ([the bracket above] + log2(n) eta [+ kappa in form 2]) sqrt(n) F max|W| ||x||_2
per trace, in the 2-norm, and every single point is held to the same absolute amount.  No measured constant.
"""
import os
import sys

import numpy as np

from nmrfit_amd import fid
from tests import fid_support as fs

U = fs.U
GAMMA2 = 2.0 * U / (1.0 - 2.0 * U)
KAPPA = fs.MU_DEVICE + np.sqrt(2.0) * GAMMA2 * (1.0 + fs.MU_DEVICE)
ETA = fs.eta(fs.MU_DEVICE)
# the group delays of the tests, as used (no rounding: truncate_grpdly=False): add = 62, 61 (67.9: skip = 69), 1, 0, and
# skip = 2; the last is a parameter file's own value, unrounded
G_VALUES = (68.0, 67.9, 5.0, 4.0, 0.3, 67.98416137695312)


def skip_add(g):
    skip = int(np.floor(g + 2.0))
    return skip, max(skip - 6, 0)


def bracket(form, s, has_window):
    """The relative bound on the conditioned trace, without F max|W| ||x||_2."""
    if form == fid.FORM_FID:
        return 2.0 * np.log2(s) * ETA + KAPPA + 2.0 * U
    return U if has_window else 0.0


def scale(x, form, g, W):
    """F max|W| ||x_t||_2 per trace."""
    F = np.sqrt(2.0) if form == fid.FORM_FID and skip_add(g)[1] > 0 else 1.0
    wmax = 1.0 if W is None else float(np.abs(W).max())
    return F * wmax * np.sqrt((np.abs(np.asarray(x).reshape(-1, np.shape(x)[-1])) ** 2).sum(axis=-1))


def bars(x, form, g, W, n):
    """(the bar of the conditioned trace, of the spectrum): absolute, per trace."""
    s = np.shape(x)[-1]
    sc = scale(x, form, g, W)
    b = bracket(form, s, W is not None)
    return b * sc, (b + np.log2(n) * ETA + (KAPPA if form == fid.FORM_SPECTRUM else 0.0)) * np.sqrt(n) * sc


def ratio(got, want, bar):
    """max(2-norm error, worst point) / bar, the worst over the traces.  ``want`` in long double; a bar of 0 asks for
    equality (the ratio is then 0 or inf)."""
    d = np.abs(np.asarray(got).astype(np.clongdouble) - want)
    e2 = np.sqrt((d ** 2).sum(axis=-1)).astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(e2 == 0.0, 0.0, e2 / bar)
    return float(np.max(r))


def truth(x, g, mode, W, n):
    """condition_host in long double: (xc, Y)."""
    return fid.condition_host(np.asarray(x).astype(np.clongdouble), g, mode, None if W is None else np.asarray(W, dtype=np.longdouble), n)


def raw_call(L, n_in, n, T, x, form, g, window_of, windows, device=0, want_Z=True, want_C=True):
    """nmrfit_fid_condition_transform on numpy arrays: (rc, u, v, rows, Z, C)."""
    from nmrfit_amd import _cabi
    p = _cabi.ptr
    n_in, n = np.asarray(n_in, dtype=np.int64), np.asarray(n, dtype=np.int64)
    T, form, window_of = (np.asarray(a, dtype=np.int32) for a in (T, form, window_of))
    g = np.asarray(g, dtype=np.float64)
    K = len(n_in)
    wl = np.array([len(w) for w in windows], dtype=np.int64)
    wf = np.concatenate([np.asarray(w, dtype=np.float64) for w in windows]) if len(windows) else None
    u, v, rows = np.zeros(int(n.sum())), np.zeros(int(n.sum())), np.zeros(K * fid.ROW)
    Z = np.zeros(2 * int((T * n).sum())) if want_Z else None
    C = np.zeros(2 * int((T * n_in).sum())) if want_C else None      # (at least as long as the conditioned traces)
    rc = L.nmrfit_fid_condition_transform(device, K, p(n_in), p(n), p(T), p(np.ascontiguousarray(x)), p(form), p(g), p(window_of),
                                          len(windows), p(wl) if len(windows) else None, p(wf), p(u), p(v), p(rows), p(Z), p(C))
    return rc, u, v, rows, Z, C


# ---- the mixed batch -----------------------------------------------------------------------------------------------------

def mixed_jobs():
    """Every form, shared and private windows, shared and different g, T = 1 and 3, short and two-pass lengths, one job
    with nothing asked: a list of (x, g, mode, W).  Windows A and B are shared by two jobs each."""
    A = fid.window_em(512 - 70, 3.0, 1000.0, first_point=0.5)
    B = fid.window_sine(1000, 0.0, 0.95, 2.0)
    jobs = [(fs.sample_fid(300, 2, seed=20), None, "fid", None),
            (fs.sample_fid(512, 1, seed=21), 68.0, "fid", A),
            (fs.sample_fid(512, 3, seed=22), 68.0, "fid", A.copy()),
            (fs.sample_fid(8192, 1, seed=23), 5.0, "fid", fid.window_gauss(8192 - 7, 2.0, 8000.0)),
            (fs.sample_fid(1 << 14, 3, seed=24), 67.98416137695312, "fid", None),
            (fs.sample_fid(1000, 1, seed=25), 68.0, "spectrum", B),
            (fs.sample_fid(5000, 3, seed=26), 0.3, "spectrum", None),
            (fs.sample_fid(1000, 2, seed=27), None, "fid", B),
            (fs.sample_fid(64, 1, seed=28), None, "spectrum", fid.window_em(64, 1.0, 64.0)),
            (fs.sample_fid(256, 1, seed=29), 4.0, "fid", None)]
    return jobs


def run_mixed(jobs, **kw):
    """One transform_many call over (x, g, mode, W) jobs: (u, v, row, Y, xc) per job."""
    return fid.transform_many([j[0] for j in jobs], zero_fill="pow2", grpdly=[j[1] for j in jobs], grpdly_mode=[j[2] for j in jobs],
                              window=[j[3] for j in jobs], truncate_grpdly=False, return_transform=True, return_conditioned=True, **kw)


def poison_run(out):
    """The mixed batch with every output asked for.  Host outputs start as NaN (np.empty is filled), so a copy that came
    up short shows."""
    from tests import poison_support
    arrays = {}
    with poison_support.nan_outputs():
        full = run_mixed(mixed_jobs())
        for k, f in enumerate(full):
            arrays["u%d" % k], arrays["v%d" % k], arrays["row%d" % k] = f[0], f[1], f[2]
            arrays["Y%d" % k], arrays["C%d" % k] = f[3].view(np.float64), f[4].view(np.float64)
            assert f[2][0] == 0 and all(np.isfinite(np.asarray(a).view(np.float64)).all() for a in f), k
    arrays["__poison__"] = np.array(os.environ.get("NMRFIT_POISON_ALLOC", ""))
    np.savez(out, **arrays)


if __name__ == "__main__":
    if len(sys.argv) != 3 or sys.argv[1] != "poison":
        sys.exit("usage: python -m tests.fid_cond_support poison OUT.npz")
    poison_run(sys.argv[2])

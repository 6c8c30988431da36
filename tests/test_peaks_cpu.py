"""
CPU tier of the device-batched peak picking (nmrfit_peaks_pick, csrc/peaks.hip): the entry points are bound, argument
errors are the host's and come before any device work, the per-spectrum capacity bound holds, and a numpy restatement
of the device's exact steps reproduces scipy / numpy bit for bit and AutoPeakSelector under the parity contract.  No GPU.
"""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import scipy.integrate
import scipy.interpolate
import scipy.signal

from nmrfit_amd import _cabi, containers, peaks, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "nmrfit_amd", "csrc", "peaks.hip")


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


def savgol_np(U, edges):
    c = [float.fromhex(h) for h in _hip_savgol()]
    S = U[5:-5] * c[0]
    for k in (5, 4, 3, 2, 1):
        S = S + (U[5 + k:len(U) - 5 + k] + U[5 - k:len(U) - 5 - k]) * c[k]
    return np.concatenate([edges[:5], S, edges[5:]])


def const_baseline_np(y, mean=lambda a: np.float64(__import__("math").fsum(a)) / len(a)):
    """peakutils.baseline(y, 0)[0] with the device's quirks: the last accepted c, y[0] on a first-test pass."""
    coef, clip, out = 1.0, np.inf, y[0]
    for _ in range(100):
        with np.errstate(all="ignore"):
            m = mean(np.minimum(y, clip))
            d = m - coef
            if np.sqrt(d * d) / np.sqrt(coef * coef) < 1e-3:
                break
        coef = out = m
        clip = np.minimum(clip, m)
    return out


def nearest(cands, W, loc):
    if cands.size == 0:
        return None
    d = np.abs(W[cands] - loc)
    return cands[np.argmin(d)]


def emulate(w, u, thresh, window):
    """(peak dicts, global baseline) by the device's plan, the means by math.fsum."""
    xs, ys, edges, order, M = peaks._prepare(w, u, window)
    W = peaks.grid_points(xs[0], xs[-1], M, np.arange(M))
    U = interp_np(xs, ys, W)
    S = savgol_np(U, edges)
    B = const_baseline_np(S)
    out = []
    for i in peaks.argrelmax(S, order):
        h = U[i] - B
        if not h > thresh:
            continue
        with np.errstate(all="ignore"):
            side = np.sign(h / 2.0 - (U - B))
        cr = side[:-1] - side[1:]
        jf, jr = nearest(np.flatnonzero(cr < 0), W, W[i]), nearest(np.flatnonzero(cr > 0), W, W[i])
        if jf is None or jr is None or not W[jr] < W[jf]:
            continue
        width = W[jf] - W[jr]
        b = [W[i] - 2 * width, W[i] + 2 * width]
        sel = np.flatnonzero((W >= b[0]) & (W <= b[1]))
        pb = const_baseline_np(U[sel])
        out.append(dict(i=i, loc=W[i], width=width, bounds=b, lo=sel[0], hi=sel[-1], baseline=pb, height=U[i] - pb,
                        area=scipy.integrate.simpson(U[sel] - pb, x=W[sel])))
    return out, B, U, S


def _hip_savgol():
    text = open(SRC).read()
    body = re.search(r"kSavgol\[6\]\s*=\s*\{([^}]*)\}", text).group(1)
    return [t.strip() for t in body.split(",")]


def close(a, b, scale, rel=1e-12):
    return abs(a - b) <= rel * max(abs(b), scale)


# ---- tests -------------------------------------------------------------------------------------------------------------

def test_entry_points_are_exported_and_bound():
    L = ctypes.CDLL(_cabi.LIB_PATH)
    assert hasattr(L, "nmrfit_peaks_pick") and "nmrfit_peaks_pick" in _cabi.SIGNATURES
    assert hasattr(L, "nmrfit_diag_peaks_smooth") and "nmrfit_diag_peaks_smooth" in _cabi.DIAG_SIGNATURES
    assert _cabi.lib().nmrfit_abi_version() == 6


def test_device_savgol_coefficients_are_scipys():
    c = scipy.signal.savgol_coeffs(11, 4)
    assert [float.fromhex(h) for h in _hip_savgol()] == c[5:].tolist()


@pytest.mark.parametrize("descending", [False, True])
def test_restated_upsample_and_smooth_are_scipys_bit_for_bit(descending):
    rng = np.random.default_rng(3)
    for N in (2, 7, 300, 1000):
        w = np.sort(rng.uniform(-2, 5, N)) if N > 2 else np.array([0.5, 2.0])
        if N == 1000:
            w = np.linspace(3.0, 4.0, N)
        if descending:
            w = w[::-1].copy()
        u = rng.standard_normal(N) * 10 ** rng.uniform(-3, 3)
        sel = peaks.AutoPeakSelector(w, u, 0.0, 0.02)
        xs, ys, edges, order, M = peaks._prepare(w, u)
        W = peaks.grid_points(xs[0], xs[-1], M, np.arange(M))
        assert np.array_equal(W, sel.w)
        U = interp_np(xs, ys, W)
        assert np.array_equal(U, sel.u)
        assert np.array_equal(savgol_np(U, edges), sel.u_smoothed)


def test_the_searchsorted_form_is_not_what_scipy_computes():
    """scipy's linear interp1d calls numpy.interp, which returns ys[j] on a knot: at the last point W = w.max() the
    searchsorted form (slope from the last interval) can miss by an ulp.  The device restates numpy.interp."""
    rng = np.random.default_rng(0)
    xs = np.sort(rng.standard_normal(1000))
    ys = rng.standard_normal(1000)
    W = np.linspace(xs[0], xs[-1], 100000)
    ref = scipy.interpolate.interp1d(xs, ys)(W)
    assert np.array_equal(interp_np(xs, ys, W), ref)
    j = np.searchsorted(xs, W).clip(1, 999)
    alt = (ys[j] - ys[j - 1]) / (xs[j] - xs[j - 1]) * (W - xs[j - 1]) + ys[j - 1]
    assert not np.array_equal(alt, ref)


def test_baseline_quirks_restated():
    y = np.array([3.0, 1.0, 2.0, 0.5])
    ref = peaks.baseline(y, 0)[0]
    assert close(const_baseline_np(y), ref, 1.0)
    # the first test passes (mean within 1e-3 of 1.0): y[0] comes back
    y = 1.0 + np.array([0.3, -0.2, 1e-5, -0.1 + 1e-5])
    assert abs(y.mean() - 1.0) < 1e-3
    assert peaks.baseline(y, 0)[0] == y[0] == const_baseline_np(y)
    # NaN: 100 passes, NaN
    y = np.array([1.0, np.nan, 2.0])
    assert np.isnan(peaks.baseline(y, 0)[0]) and np.isnan(const_baseline_np(y))
    # zeros: c = 0 after the first pass, the test is NaN from then on; the result stays 0
    assert peaks.baseline(np.zeros(5), 0)[0] == 0.0 == const_baseline_np(np.zeros(5))


@pytest.mark.parametrize("N,P,descending", [(4096, 6, False), (4096, 6, True)])
def test_restated_plan_matches_the_host_mirror(N, P, descending):
    sp = synth.make_spectrum(N, P, seed=5)
    w, u = sp["w"], sp["u"]
    if descending:
        w, u = w[::-1].copy(), u[::-1].copy()
    sel = peaks.AutoPeakSelector(w, u, 0.1, 0.02)
    sel.find_peaks()
    got, B, U, S = emulate(w, u, 0.1, 0.02)
    scale = np.abs(U).max()
    assert close(B, sel.baseline, scale)
    assert len(got) == len(sel.peaks) > 0
    for g, p in zip(got, sel.peaks):
        assert g["i"] == p.i and g["loc"] == p.loc and g["width"] == p.width and g["bounds"] == p.bounds
        assert np.array_equal(np.arange(g["lo"], g["hi"] + 1), p.idx[0])
        assert close(g["baseline"], p.baseline, scale) and close(g["height"], p.height, scale)
        assert close(g["area"], p.area, scale * p.width)


def test_capacity_bounds_the_maxima():
    rng = np.random.default_rng(9)
    for M, order in ((200, 1), (1000, 3), (4096, 40), (10001, 100)):
        x = rng.standard_normal(M)
        assert peaks.argrelmax(x, order).size <= peaks.capacity(M, order)
        # the bound is reached: maxima every order + 1 points, at the slot starts after the first
        x = np.zeros(M)
        x[order + 1::order + 1] = 1.0
        x[0] = 0.0
        n = peaks.argrelmax(x, order).size
        assert n <= peaks.capacity(M, order) and n >= peaks.capacity(M, order) - 2
    assert peaks.capacity(409600, 819) == 500


def test_argument_errors_are_the_hosts_and_need_no_device():
    w = np.linspace(3.0, 4.0, 64)
    with pytest.raises(ValueError):
        peaks.find_peaks_many([w], [w[:-1]])                         # interp1d: lengths differ
    with pytest.raises(ValueError, match="Order must be an int >= 1"):
        peaks.find_peaks_many([w], [w], window=1e-9)
    with pytest.raises(ValueError, match="Order must be an int >= 1"):
        peaks.find_peaks_many([w, w], [w, w], window=[0.02, -1.0])
    with pytest.raises(OverflowError):
        peaks.find_peaks_many([np.array([1.0])], [np.array([2.0])])  # N = 1, as on the host
    with pytest.raises(OverflowError):
        peaks.AutoPeakSelector(np.array([1.0]), np.array([2.0]), 0.0, 0.02).find_peaks()
    with pytest.raises(ValueError):
        peaks.find_peaks_many([w, w], [w, w], thresh=[0.0, 0.1, 0.2])
    d = containers.Data(w, w, w)
    d.V = w
    with pytest.raises(ValueError, match="Number of peaks must be specified"):
        containers.select_peaks_many([d], method="manual")
    with pytest.raises(ValueError, match="Method must be 'auto' or 'manual'"):
        containers.select_peaks_many([d], method="brute")
    # a Data cropped by select_bounds and not re-phased: len(w) != len(V)
    d.select_bounds(3.2, 3.8)
    with pytest.raises(ValueError):
        containers.select_peaks_many([d])
    with pytest.raises(ValueError):
        d.select_peaks()


def test_library_refuses_bad_batches_before_the_device():
    L = _cabi.lib()
    N = np.array([64], dtype=np.int64)
    w = np.linspace(0.0, 1.0, 64)
    e = np.zeros(10)
    o = np.array([5], dtype=np.int64)
    t = np.zeros(1)
    b, c = np.zeros(1), np.zeros(1, dtype=np.int64)
    idx, val = np.zeros(3 * 6400, dtype=np.int64), np.zeros(5 * 6400)

    def call(N=N, w=w, o=o, S=1):
        return L.nmrfit_peaks_pick(0, S, _cabi.ptr(N), _cabi.ptr(w), _cabi.ptr(w), _cabi.ptr(e), _cabi.ptr(o),
                                   _cabi.ptr(t), _cabi.ptr(b), _cabi.ptr(c), _cabi.ptr(idx), _cabi.ptr(val))
    assert call(S=0) == _cabi.E_INVALID
    assert call(S=65536) == _cabi.E_INVALID
    assert call(o=np.array([0], dtype=np.int64)) == _cabi.E_INVALID
    assert call(N=np.array([1], dtype=np.int64)) == _cabi.E_INVALID
    assert call(w=w[::-1].copy()) == _cabi.E_INVALID                        # the caller sorts
    big = np.array([(1 << 26) // 100 + 1], dtype=np.int64)
    assert call(N=big) == _cabi.E_UNSUPPORTED                                # above the point budget
    assert L.nmrfit_peaks_pick(0, 1, _cabi.ptr(N), _cabi.ptr(w), _cabi.ptr(w), _cabi.ptr(e), _cabi.ptr(o), None,
                               _cabi.ptr(b), _cabi.ptr(c), _cabi.ptr(idx), _cabi.ptr(val)) == _cabi.E_INVALID


def test_calls_respect_the_point_budget():
    Ms = [409600] * 200 + [6553600] * 3 + [1 << 27]
    calls = list(peaks._calls(Ms))
    assert calls[0][0] == 0 and calls[-1][1] == len(Ms)
    for k0, k1 in calls:
        assert k1 > k0 and (k1 - k0 == 1 or sum(Ms[k0:k1]) <= peaks.POINT_BUDGET)
    assert list(peaks._calls([10] * 70000)) == [(0, 65535), (65535, 70000)]


def test_device_path_without_gpu_fails_loudly():
    if _cabi.device_count() != 0:
        pytest.skip("a GPU is visible: tests/test_gpu_peaks.py covers the device")
    w = np.linspace(3.0, 4.0, 64)
    with pytest.raises(_cabi.NmrfitError) as ei:
        peaks.find_peaks_many([w], [np.exp(-((w - 3.5) / 0.01) ** 2)])
    assert ei.value.code == _cabi.E_NO_DEVICE


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="hipcc not available")
def test_peaks_kernels_use_no_scratch():
    cmd = ["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=on",
           "-fno-fast-math", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.dirname(SRC), "-c", SRC,
           "-o", os.devnull, "-Rpass-analysis=kernel-resource-usage"]
    err = subprocess.run(cmd, capture_output=True, text=True, timeout=600).stderr
    names = re.findall(r"Function Name: (\S+)", err)
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", err)]
    assert len(names) == 3 and len(scratch) == 3, err[-2000:]
    assert all(s == 0 for s in scratch), list(zip(names, scratch))

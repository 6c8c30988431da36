"""
CPU tier of the device-batched peak picking (nmrfit_peaks_pick, csrc/peaks.hip): the entry points are bound, argument
errors are the host's and come before any device work, the per-spectrum capacity bound holds, and a numpy restatement
of the device's exact steps reproduces scipy / numpy bit for bit and AutoPeakSelector under the parity contract.  No GPU.
"""
import ctypes
import os
import re
import subprocess
import warnings

import numpy as np
import pytest
import scipy.integrate
import scipy.interpolate
import scipy.signal

from nmrfit_amd import _cabi, containers, peaks, synth
from tests import peaks_support
from tests.peaks_support import (ROOT, SRC, _hip_savgol, close, const_baseline_np, emulate, interp_np,  # noqa: F401
                                 nearest, savgol_np)


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
    got, B, U, S = emulate(w, u, 0.1, 0.02)[:4]
    scale = np.abs(U).max()
    assert close(B, sel.baseline, scale)
    assert len(got) == len(sel.peaks) > 0
    for g, p in zip(got, sel.peaks):
        assert g["i"] == p.i and g["loc"] == p.loc and g["width"] == p.width and g["bounds"] == p.bounds
        assert np.array_equal(np.arange(g["lo"], g["hi"] + 1), p.idx[0])
        assert close(g["baseline"], p.baseline, scale) and close(g["height"], p.height, scale)
        assert close(g["area"], p.area, scale * p.width)


# ---- the exactly summed truth and the edge cases of tests/test_gpu_peaks_edges.py -------------------------------------------

def test_restated_simpson_is_scipys():
    """The term-by-term Simpson, summed exactly, against scipy.integrate.simpson (which sums with np.sum): within a few
    ulp of the sum of the |terms|, on odd, even, 3-point, 2-point and duplicate-abscissa inputs."""
    rng = np.random.default_rng(21)
    inputs = []
    for n in (3, 4, 5, 6, 101, 256, 1001):
        inputs.append((rng.standard_normal(n), np.sort(rng.uniform(0.0, 3.0, n))))
        inputs.append((rng.standard_normal(n), np.linspace(2.0, 3.0, n)))
    inputs.append((np.array([1.0, 3.0]), np.array([0.5, 0.75])))
    for n in (5, 6, 9, 10):                       # coincident neighbours: the where= guards
        x = np.sort(rng.uniform(0.0, 1.0, n))
        for k in range(1, n, 3):
            x[k] = x[k - 1]
        inputs.append((rng.standard_normal(n), x))
    inputs.append((rng.standard_normal(6), np.array([0.0, 1.0, 2.0, 3.0, 3.0, 3.0])))      # den == 0 in the correction
    inputs.append((rng.standard_normal(6), np.array([0.0, 1.0, 2.0, 3.0, 3.0, 4.0])))
    for y, x in inputs:
        st = peaks_support.simpson_terms(y, x)
        ref = scipy.integrate.simpson(y, x=x)
        assert len(st.corr) == (3 if len(y) % 2 == 0 and len(y) > 2 else 0)
        assert abs(peaks_support.simpson_exact(st) - ref) <= 8 * peaks_support.EPS * st.mag, (len(y), x[:6])


def test_sum_bound_separates_a_compensated_sum_from_a_plain_one():
    """A long local range with cancellation: the plain left-to-right float64 sum misses the exact sum by more than
    sum_bound, the model of the device's lane-strided Neumaier sum stays inside."""
    rng = np.random.default_rng(4)
    x = rng.standard_normal(20000) * 10.0 ** rng.uniform(-3, 3, 20000)
    x = np.concatenate([x, -x[::-1] * (1.0 + 1e-9)])          # cancels to 1e-9 of its magnitude
    exact = peaks_support.exact_sum(x)
    for lanes in (peaks_support.LOCAL_LANES, peaks_support.GLOBAL_LANES):
        bound = peaks_support.sum_bound(x, lanes)
        assert abs(peaks_support.plain_sum(x) - exact) > bound
        assert abs(float(np.sum(x)) - exact) > bound                                      # numpy's pairwise sum too
        assert abs(peaks_support.neumaier_lanes(x, lanes) - exact) <= bound
    # without cancellation a plain sum of 6.5 M positive terms is outside as well (the large GPU case's global mean)
    y = rng.uniform(0.5, 1.5, 1 << 18)
    assert abs(peaks_support.plain_sum(y) - peaks_support.exact_sum(y)) > peaks_support.sum_bound(y, 1024)
    assert abs(peaks_support.neumaier_lanes(y, 1024) - peaks_support.exact_sum(y)) <= peaks_support.sum_bound(y, 1024)
    with pytest.raises(ValueError):
        peaks_support.sum_bound(np.ones(1 << 20), lanes=64)                               # outside the derivation's range


def test_margin_ok_is_about_the_tolerance_alone():
    T = peaks_support.Trace
    assert peaks_support.margin_ok(T([0.5, 2e-3, 9e-4], 2, 0.0))
    assert not peaks_support.margin_ok(T([0.5, 1e-3 * (1 + 1e-10)], 1, 0.0))
    assert not peaks_support.margin_ok(T([0.5, 1e-3 * (1 - 1e-10)], 1, 0.0))
    assert peaks_support.margin_ok(T([np.inf, np.nan], 2, 0.0))


_EMULATED = {}


def emulated(case):
    """(inputs, exact truth, host mirror) of a case at its CPU size, computed once."""
    if case.name not in _EMULATED:
        w, u, thresh, window = peaks_support.case_inputs(case, cpu=True)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            em = emulate(w, u, thresh, window)
            sel = peaks.AutoPeakSelector(w, u, thresh, window)
            sel.find_peaks()
        _EMULATED[case.name] = ((w, u, thresh, window), em, sel)
    return _EMULATED[case.name]


ALL_CASES = peaks_support.CASES + [peaks_support.LARGE]


@pytest.mark.parametrize("case", ALL_CASES, ids=lambda c: c.name)
def test_edge_case_reaches_its_path_with_margin(case):
    (w, u, thresh, window), em, sel = emulated(case)
    for tag in case.tags:
        assert peaks_support.reaches(tag, em, case), tag
    assert peaks_support.margin_ok(em.trace)
    for p in em.peaks:
        assert peaks_support.margin_ok(p["trace"]), p["i"]
    assert peaks_support.thresh_margin_ok(em, thresh)
    if case.order is not None:
        assert em.order == case.order


@pytest.mark.parametrize("case", ALL_CASES, ids=lambda c: c.name)
def test_edge_case_restatement_matches_the_host_mirror(case):
    """Count, i, loc, width, bounds and idx exactly; the sums under the 1e-12 contract, except where the HOST is the
    inaccurate side (host_sums=False: the subnormal spectrum, where pinv's 1/n times a subnormal costs the host 1e-10 of
    max|U|; shown here, and compared with the exact sums only on the GPU)."""
    (w, u, thresh, window), em, sel = emulated(case)
    assert len(em.peaks) == len(sel.peaks)
    finite = np.isfinite(em.U).all()
    scale = np.abs(em.U).max() if finite else 1.0
    if finite:
        ok_B = close(em.B, sel.baseline, scale)
    else:
        ok_B = (np.isnan(em.B) and np.isnan(sel.baseline)) or em.B == sel.baseline
    ok = [ok_B]
    for g, p in zip(em.peaks, sel.peaks):
        assert g["i"] == p.i and g["loc"] == p.loc and g["width"] == p.width and g["bounds"] == p.bounds
        assert np.array_equal(np.arange(g["lo"], g["hi"] + 1), p.idx[0]) and g["n"] == p.idx[0].size
        ok += [close(g["baseline"], p.baseline, scale), close(g["height"], p.height, scale),
               close(g["area"], p.area, scale * (p.bounds[1] - p.bounds[0]))]
    if case.host_sums:
        assert all(ok)
    else:
        assert not all(ok), "the host is accurate here after all: drop host_sums=False"
        assert 0 < scale < np.finfo(np.float64).tiny


@pytest.mark.parametrize("case", ALL_CASES, ids=lambda c: c.name)
def test_edge_case_device_sum_model_stays_inside_the_bounds(case):
    """The same plan with every sum taken by the numpy model of the device's lane-strided Neumaier sum: the exact
    fields do not move, and baseline, height and area stay inside the bounds the GPU tier holds the device to."""
    (w, u, thresh, window), em, sel = emulated(case)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        lanes = {}

        def model(a):                        # (the global baseline sums over 1024 lanes, everything else over 64)
            return peaks_support.neumaier_lanes(a, lanes.get("n", peaks_support.LOCAL_LANES))
        lanes["n"] = peaks_support.GLOBAL_LANES
        B = peaks_support.const_baseline_trace(em.S, model, peaks_support.GLOBAL_LANES)[0]
        lanes["n"] = peaks_support.LOCAL_LANES
    if not np.isfinite(em.B):
        assert (np.isnan(B) and np.isnan(em.B)) or B == em.B
        return
    assert abs(B - em.B) <= em.trace.err
    for p in em.peaks:
        y = em.U[p["lo"]:p["hi"] + 1]
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            pb = peaks_support.const_baseline_trace(y, model)[0]
            st = peaks_support.simpson_terms(y - pb, em.W[p["lo"]:p["hi"] + 1])
            area = peaks_support._device_simpson(st, model)
        assert abs(pb - p["baseline"]) <= p["base_err"]
        assert abs((em.U[p["i"]] - pb) - p["height"]) <= p["height_err"]
        assert abs(area - p["area"]) <= p["area_err"]


def test_stage_one_on_awkward_axes_restated_bit_for_bit():
    for name, w, u in peaks_support.smooth_cases():
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            xs, ys, edges, order, M = peaks._prepare(w, u)
            W = peaks.grid_points(xs[0], xs[-1], M, np.arange(M))
            ref_W = np.linspace(np.asarray(w, dtype=float).min(), np.asarray(w, dtype=float).max(), M)
            assert np.array_equal(W, ref_W), name
            ref_U = scipy.interpolate.interp1d(np.asarray(w, dtype=float), np.asarray(u, dtype=float))(ref_W)
            ref_S = scipy.signal.savgol_filter(ref_U, 11, 4)
            U = interp_np(xs, ys, W)
        assert np.array_equal(U, ref_U, equal_nan=True), name
        assert np.array_equal(savgol_np(U, edges), ref_S, equal_nan=True), name
    # the zero-step branch of the grid is reached by two of them
    assert peaks_support.grid_step(np.full(4, 2.5)) == 0.0 and peaks_support.grid_step(np.array([0.0, 5e-324])) == 0.0
    with pytest.raises(OverflowError):
        peaks._prepare(np.full(4, 2.5), np.ones(4), 0.02)


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

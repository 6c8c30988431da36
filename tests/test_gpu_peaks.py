"""
GPU tier of the device-batched peak picking (peaks.find_peaks_many, select_peaks_many; csrc/peaks.hip) against the host
mirror AutoPeakSelector(w, V, thresh, window).find_peaks() under the parity contract: count, i, loc, width, bounds and
idx exactly; the global and local baselines, height and area within 1e-12 relative (or 1e-12 max|U| where the value is
near zero); every spectrum bit-identical alone or in a batch; U and S equal to interp1d + savgol_filter bit for bit.
"""
import os

import numpy as np
import pytest

from nmrfit_amd import _cabi, containers, peaks, synth

pytestmark = pytest.mark.gpu

_HOST = {}


def host(key, w, u, thresh, window):
    """The host mirror (≈1.2 s at 4096 points, ≈8 s at 65536): computed once per case."""
    if key not in _HOST:
        sel = peaks.AutoPeakSelector(w, u, thresh, window)
        sel.find_peaks()
        _HOST[key] = sel
    return _HOST[key]


def rel_ok(a, b, scale, rel=1e-12):
    return (np.isnan(a) and np.isnan(b)) or abs(a - b) <= rel * max(abs(b), scale)


def assert_contract(got, base, sel):
    scale = np.nanmax(np.abs(sel.u)) if np.isfinite(sel.u).any() else 1.0
    assert rel_ok(base, sel.baseline, scale), (base, sel.baseline)
    assert len(got) == len(sel.peaks)
    for g, p in zip(got, sel.peaks):
        assert type(g.i) is type(np.int64(0)) and g.i == p.i
        assert g.loc == p.loc and g.width == p.width
        assert isinstance(g.bounds, list) and g.bounds == p.bounds
        assert isinstance(g.idx, tuple) and len(g.idx) == 1 and g.idx[0].dtype == np.int64
        assert np.array_equal(g.idx[0], p.idx[0])
        assert rel_ok(g.baseline, p.baseline, scale) and rel_ok(g.height, p.height, scale)
        assert rel_ok(g.area, p.area, scale * (p.bounds[1] - p.bounds[0]))


def spec(N, P, seed=1, **kw):
    sp = synth.make_spectrum(N, P, seed=seed, **kw)
    return sp["w"], sp["u"]


def _golden_data():
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "data_container.npz")
    g = np.load(path)
    d = containers.Data(g["w"], g["u"], g["v"])
    d.shift_phase(method="auto")
    return d


@pytest.mark.parametrize("N", [2, 4096, 65536])
@pytest.mark.parametrize("form", ["ascending", "descending", "nonuniform"])
def test_upsample_and_smooth_are_scipys_bit_for_bit(N, form):
    import scipy.interpolate
    import scipy.signal
    rng = np.random.default_rng(N)
    if form == "nonuniform":
        w = np.sort(rng.uniform(-1.0, 9.0, N))
    else:
        w = np.linspace(3.0, 4.0, N)
    u = rng.standard_normal(N)
    if form == "descending":
        w, u = w[::-1].copy(), u
    [(U, S)] = peaks.smooth_many([w], [u])
    W = np.linspace(w.min(), w.max(), N * 100)
    ref_U = scipy.interpolate.interp1d(w, u)(W)
    assert np.array_equal(U, ref_U)
    assert np.array_equal(S, scipy.signal.savgol_filter(ref_U, 11, 4))


def test_golden_spectrum_after_auto_phase():
    d = _golden_data()
    sel = host("golden", d.w, d.V, 0.0, 0.02)
    got, base = peaks.find_peaks_many([d.w], [d.V], thresh=0.0, window=0.02, return_baseline=True)
    assert len(sel.peaks) > 0
    assert_contract(got[0], base[0], sel)


CASES = {
    "4096/6 t0.1": (lambda: spec(4096, 6, seed=1), 0.1, 0.02),
    "4096/6 t0": (lambda: spec(4096, 6, seed=1), 0.0, 0.02),
    "16384/12": (lambda: spec(16384, 12, seed=2), 0.1, 0.02),
    "65536/24": (lambda: spec(65536, 24, seed=3), 0.1, 0.02),
    "4096 descending": (lambda: tuple(a[::-1].copy() for a in spec(4096, 6, seed=4)), 0.1, 0.02),
    "offset +1": (lambda: (lambda w, u: (w, u + 1.0))(*spec(4096, 6, seed=5)), 0.0, 0.02),
    "window > span": (lambda: spec(4096, 6, seed=6), 0.0, 2.0),
    "thresh above all": (lambda: spec(4096, 6, seed=7), 1e6, 0.02),
}


@pytest.mark.parametrize("name", list(CASES))
def test_against_the_host_mirror(name):
    make, thresh, window = CASES[name]
    w, u = make()
    sel = host(name, w, u, thresh, window)
    got, base = peaks.find_peaks_many([w], [u], thresh=thresh, window=window, return_baseline=True)
    assert_contract(got[0], base[0], sel)
    if name == "thresh above all":
        assert len(got[0]) == 0
    if name in ("4096/6 t0.1", "65536/24"):
        assert len(got[0]) > 0


@pytest.mark.parametrize("bad", ["nan", "inf", "zero"])
def test_non_finite_and_zero_spectra(bad):
    w, u = spec(4096, 6, seed=8)
    u = u.copy()
    if bad == "nan":
        u[1234] = np.nan
    elif bad == "inf":
        u[77] = np.inf
    else:
        u[:] = 0.0
    got, base = peaks.find_peaks_many([w], [u], return_baseline=True)
    assert len(got[0]) == 0
    if bad == "zero":
        assert base[0] == 0.0
    else:
        assert np.isnan(base[0])
    sel = host("bad " + bad, w, u, 0.0, 0.02)
    assert len(sel.peaks) == 0 and (np.isnan(sel.baseline) == np.isnan(base[0]))


def test_per_spectrum_thresh_and_window():
    a, b = spec(4096, 6, seed=1), spec(4096, 6, seed=6)
    got = peaks.find_peaks_many([a[0], b[0]], [a[1], b[1]], thresh=[0.1, 0.0], window=[0.02, 2.0])
    assert_contract(got[0], peaks.find_peaks_many([a[0]], [a[1]], 0.1, 0.02, return_baseline=True)[1][0],
                    host("4096/6 t0.1", *a, 0.1, 0.02))
    assert_contract(got[1], peaks.find_peaks_many([b[0]], [b[1]], 0.0, 2.0, return_baseline=True)[1][0],
                    host("window > span", *b, 0.0, 2.0))


def _same(p, q):
    return (p.i == q.i and p.loc == q.loc and p.width == q.width and p.bounds == q.bounds
            and np.array_equal(p.idx[0], q.idx[0]) and p.baseline == q.baseline and p.height == q.height
            and p.area == q.area)


def test_ragged_batch_is_bit_identical_to_lone_calls():
    specs = [spec(4096, 6, seed=1), spec(16384, 12, seed=2), spec(2048, 3, seed=9), spec(8000, 9, seed=10)]
    specs[3] = (specs[3][0][::-1].copy(), specs[3][1][::-1].copy())
    th = [0.1, 0.1, 0.0, 0.05]
    batch, bb = peaks.find_peaks_many([s[0] for s in specs], [s[1] for s in specs], thresh=th, return_baseline=True)
    for k, s in enumerate(specs):
        lone, lb = peaks.find_peaks_many([s[0]], [s[1]], thresh=th[k], return_baseline=True)
        assert lb[0] == bb[k]
        assert len(lone[0]) == len(batch[k]) and all(_same(p, q) for p, q in zip(lone[0], batch[k]))


def test_a_list_longer_than_one_call(monkeypatch):
    w, u = spec(2048, 4, seed=11)
    lone = peaks.find_peaks_many([w], [u], thresh=0.05)[0]
    monkeypatch.setattr(peaks, "POINT_BUDGET", 3 * 2048 * 100)        # three spectra per call
    calls = []
    L = _cabi.lib()

    class Spy:
        def __getattr__(self, name):
            return getattr(L, name)

        def nmrfit_peaks_pick(self, *a):
            calls.append(a[1])
            return L.nmrfit_peaks_pick(*a)
    monkeypatch.setattr(_cabi, "lib", lambda spy=Spy(): spy)
    out = peaks.find_peaks_many([w] * 8, [u] * 8, thresh=0.05)
    assert calls == [3, 3, 2]
    for got in out:
        assert len(got) == len(lone) and all(_same(p, q) for p, q in zip(got, lone))


def test_select_peaks_many_sets_peaks_and_roibounds_and_feeds_a_fit():
    from nmrfit_amd import fit_many
    w, u = spec(4096, 6, seed=1)
    v = np.zeros_like(u)
    dh, dd = containers.Data(w, u, v), containers.Data(w, u, v)
    for d in (dh, dd):
        d.shift_phase(method="manual", p0=0.0, p1=0.0)
    dh.select_peaks(method="auto", thresh=0.1, window=0.02)
    containers.select_peaks_many([dd], method="AUTO", thresh=0.1, window=0.02)
    assert len(dd.peaks) == len(dh.peaks) > 0
    assert dd.roibounds == dh.roibounds
    lo_h, up_h = dh.generate_solution_bounds()
    lo_d, up_d = dd.generate_solution_bounds()
    scale = np.abs(np.concatenate([lo_h, up_h])).max()
    assert np.allclose(lo_d, lo_h, rtol=1e-12, atol=1e-12 * scale) and np.allclose(up_d, up_h, rtol=1e-12, atol=1e-12 * scale)
    res = fit_many([(dd, lo_d, up_d)], options={"maxiter": 5, "swarmsize": 64, "seed": 1})
    assert len(res) == 1 and np.isfinite(res[0].error)

"""
GPU tier of the device-batched peak picking at its edges (csrc/peaks.hip; the cases and the truth are
tests/peaks_support.py's, their paths are asserted without a GPU in tests/test_peaks_cpu.py).  Every case asserts of
``find_peaks_many(..., return_baseline=True)``:
  (a) count, i, loc, width, bounds and idx are the host mirror's exactly, types included (test_gpu_peaks.assert_contract,
      which also holds the sums to 1e-12 of the host; a case marked host_sums=False, where the host is the inaccurate
      side, takes the exact fields alone);
  (b) global baseline, local baseline, height and area lie within peaks_support's derived bounds of the exactly summed
      truth (math.fsum), never of the device's own output;
  (c) the lone call and the same spectrum placed second in a ragged batch of three are bit-identical.
Each comparison prints ``error / bound`` before it asserts (run with -s to collect them); the worst over all cases is
recorded in DESIGN.md 4.8.  Nothing here is built to make the device fault: the non-finite cases only end cleanly (every
loop in peaks.hip is bounded), the refusals stay in the CPU tier.
"""
import warnings

import numpy as np
import pytest
import scipy.interpolate
import scipy.signal

from nmrfit_amd import peaks
from tests import peaks_support
from tests.test_gpu_peaks import _same, assert_contract

pytestmark = pytest.mark.gpu

_RUN = {}


def quiet(f, *a, **kw):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")          # (numpy's warnings on the NaN, inf, 1e200 and subnormal inputs)
        return f(*a, **kw)


def run(case):
    """(inputs, truth, lone device result, the same spectrum as the second of a ragged batch of three), once per case."""
    if case.name not in _RUN:
        w, u, thresh, window = peaks_support.case_inputs(case)
        em = quiet(peaks_support.emulate, w, u, thresh, window)
        lone = quiet(peaks.find_peaks_many, [w], [u], thresh=thresh, window=window, return_baseline=True)
        a = peaks_support.tents(7, {3: 1.0}, floor=0.05)
        c = peaks_support.lines(300, 3, seed=2)
        batch = quiet(peaks.find_peaks_many, [a[0], w, c[0]], [a[1], u, c[1]], thresh=[0.1, thresh, 0.05],
                      window=[0.3, window, 0.02], return_baseline=True)
        _RUN[case.name] = ((w, u, thresh, window), em, (lone[0][0], lone[1][0]), (batch[0][1], batch[1][1]))
    return _RUN[case.name]


def same_float(a, b):
    return (np.isnan(a) and np.isnan(b)) or a == b


def within(what, got, want, bound):
    """|got - want| <= bound, the ratio printed first; non-finite truths must be met exactly."""
    if not np.isfinite(want) or not np.isfinite(bound):
        print("RATIO %-60s exact %r %r" % (what, got, want))
        return same_float(got, want)
    err = abs(got - want)
    print("RATIO %-60s %.3f   (error %.3e, bound %.3e)" % (what, err / bound if bound > 0 else (0.0 if err == 0 else np.inf),
                                                          err, bound))
    return err <= bound


@pytest.mark.parametrize("case", peaks_support.CASES, ids=lambda c: c.name)
def test_exact_fields_are_the_host_mirrors(case):
    (w, u, thresh, window), em, (got, base), _ = run(case)
    sel = quiet(peaks.AutoPeakSelector, w, u, thresh, window)
    quiet(sel.find_peaks)
    assert peaks_support.all_margins_ok(em, thresh)                 # the condition under which device and host must agree
    if case.host_sums:
        assert_contract(got, base, sel)
    else:
        assert len(got) == len(sel.peaks)
        for g, p in zip(got, sel.peaks):
            assert type(g.i) is type(np.int64(0)) and g.i == p.i
            assert g.loc == p.loc and g.width == p.width
            assert isinstance(g.bounds, list) and g.bounds == p.bounds
            assert isinstance(g.idx, tuple) and len(g.idx) == 1 and g.idx[0].dtype == np.int64
            assert np.array_equal(g.idx[0], p.idx[0])
    # ... and the restatement's, crossings and all
    assert [g.i for g in got] == [p["i"] for p in em.peaks]
    if "peak" in case.tags:
        assert len(got) > 0
    if "nopeaks" in case.tags:
        assert len(got) == 0
    if "nan_baseline" in case.tags:
        assert np.isnan(base) and np.isnan(sel.baseline)


@pytest.mark.parametrize("case", peaks_support.CASES + [peaks_support.LARGE], ids=lambda c: c.name)
def test_sums_against_the_exactly_summed_truth(case):
    (w, u, thresh, window), em, (got, base), _ = run(case)
    assert peaks_support.all_margins_ok(em, thresh)
    ok = [within(case.name + ": global baseline", base, em.B, em.trace.err)]
    assert len(got) == len(em.peaks)
    for g, p in zip(got, em.peaks):
        assert g.i == p["i"] and g.idx[0][0] == p["lo"] and g.idx[0][-1] == p["hi"] and g.width == p["width"]
        at = "%s: peak at %d, n = %d: " % (case.name, p["i"], p["n"])
        ok.append(within(at + "baseline", g.baseline, p["baseline"], p["base_err"]))
        ok.append(within(at + "height", g.height, p["height"], p["height_err"]))
        ok.append(within(at + "area", g.area, p["area"], p["area_err"]))
    assert all(ok)


@pytest.mark.parametrize("case", peaks_support.CASES, ids=lambda c: c.name)
def test_lone_and_second_of_three_are_bit_identical(case):
    _, _, (lone, lone_base), (batch, batch_base) = run(case)
    assert same_float(lone_base, batch_base)
    assert len(lone) == len(batch) and all(_same(p, q) for p, q in zip(lone, batch))


@pytest.mark.parametrize("k", range(len(peaks_support.smooth_cases())), ids=[c[0] for c in peaks_support.smooth_cases()])
def test_stage_one_on_awkward_axes_is_scipys_bit_for_bit(k):
    name, w, u = peaks_support.smooth_cases()[k]
    [(U, S)] = quiet(peaks.smooth_many, [w], [u])
    wf, uf = np.asarray(w, dtype=float), np.asarray(u, dtype=float)
    W = np.linspace(wf.min(), wf.max(), len(wf) * 100)
    ref_U = quiet(lambda: scipy.interpolate.interp1d(wf, uf)(W))
    ref_S = quiet(scipy.signal.savgol_filter, ref_U, 11, 4)
    assert np.array_equal(U, ref_U, equal_nan=True)
    assert np.array_equal(S, ref_S, equal_nan=True)

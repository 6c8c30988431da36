"""
GPU tier of the device phase path at its edges: every rule phase.hip restates from numpy and scipy, checked against the
host mirror (proc_autophase, containers) or scipy.optimize.fmin itself at the shapes and inputs where it matters --
the ACME tile geometry and both reduction widths, NaN / inf / zero / subnormal / tied input, numpy's argmax and python's
slicing in the peak-minima window, numpy's pairwise block in the brute means, and the brute mean length of a cropped
Data.  At phase (0, 0) the rotation is exact (sincos(0) = (0, 1), fma(1, u, -(0 v)) = u for finite v), so the
peak-minima checks there are exact equalities.  Each test prints its worst deviation.
"""
import contextlib
import warnings

import numpy as np
import pytest
import scipy.optimize

from nmrfit_amd import _cabi, proc_autophase, synth
from nmrfit_amd.containers import Data, shift_phase_many

pytestmark = pytest.mark.gpu

CANDIDATES = np.array([[0.0, 0.0], [0.5, 900.0], [-1000.0, 7.0], [3.0, -640.0]])


@contextlib.contextmanager
def _quiet():
    """the host's numpy warnings on NaN / inf / 0-over-0 input (the values are what is checked)"""
    with np.errstate(all="ignore"), warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        yield


def _complex(u, v):
    """u + i v without 1j * v (which turns an inf in v into a NaN real part)"""
    z = np.empty(len(u), dtype=np.complex128)
    z.real = u
    z.imag = v
    return z


def _worst(got, want):
    """worst relative deviation where both are finite; NaN and inf must agree exactly (sign included)"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    np.testing.assert_array_equal(np.isnan(got), np.isnan(want))
    fin = np.isfinite(want)
    np.testing.assert_array_equal(got[~fin & ~np.isnan(want)], want[~fin & ~np.isnan(want)])
    assert np.all(np.isfinite(got[fin])), (got[fin], want[fin])
    if not fin.any():
        return 0.0
    return float(np.max(np.abs(got[fin] - want[fin]) / np.maximum(np.abs(want[fin]), 1e-300)))


def _same(a, b):
    np.testing.assert_array_equal(np.asarray(a), np.asarray(b))    # (NaN equals NaN here)


def _host_acme(z, cands=CANDIDATES):
    with _quiet():
        return np.array([proc_autophase._ps_acme_score(p, z) for p in cands])


# ---- ACME geometry -------------------------------------------------------------------------------------------------

def _acme_spectrum(N, rng):
    """positive real part (no penalty at (0, 0): the score is the entropy alone) except the first and the last point,
    which are negative (the penalty's j == N - 1 case); other phases give negative points anywhere"""
    u = rng.exponential(1.0, N) + 0.05
    u[0], u[-1] = -0.5, -1.0
    return _complex(u, rng.standard_normal(N))


def _acme_lengths():
    Ns = list(range(2, 201))
    for k in (1, 2, 3, 4, 5, 8, 12, 16, 64, 128, 256, 264, 272, 520, 1024):   # tiles = k +- 1 around 4 / 8 waves
        Ns += [63 * k + d for d in (0, 1, 2)]
    Ns += [16383, 16384, 16385]
    return sorted(set(Ns))


def test_acme_geometry_sweep_matches_the_host_and_the_lone_calls():
    """Every N from 2 to 200, N = 63 k + {0, 1, 2} where the tile count crosses a multiple of 4 and 8 waves, the
    256 / 512-thread switch, and 2^20 + 1 points: rtol 1e-12 against _ps_acme_score at four candidates; one ragged call
    equals the lone calls bit for bit."""
    rng = np.random.default_rng(1)
    Ns = _acme_lengths() + [(1 << 20) + 1]
    zs = [_acme_spectrum(N, rng) for N in Ns]
    got = proc_autophase.phase_scores(zs, CANDIDATES, "acme")
    worst, at = 0.0, None
    for k, z in enumerate(zs):
        w = _worst(got[k], _host_acme(z))
        if w > worst:
            worst, at = w, Ns[k]
        assert w <= 1e-12, (Ns[k], got[k], _host_acme(z))
        _same(proc_autophase.phase_scores([z], CANDIDATES, "acme")[0], got[k])
    # (0, 0): the entropy (0 for N = 2: one slope) plus the penalty of the two negative end points, 1000 (0.25 + 1)
    assert np.all(got[:, 0] >= 1250.0) and got[0, 0] == 1250.0
    print("ACME geometry: %d lengths, worst relative deviation %.3g (N = %s)" % (len(Ns), worst, at))


# ---- degenerate spectra ----------------------------------------------------------------------------------------------

def _normal(N, seed):
    sp = synth.make_spectrum(N, 3, seed=seed, physical=True)
    return _complex(sp["u"], sp["v"])


def _degenerate(N=4096):
    rng = np.random.default_rng(5)
    out = {"zeros": np.zeros(N, dtype=np.complex128), "constant": np.full(N, 1.0 + 1.0j)}
    z = _normal(N, 11)
    z.real[1000] = np.nan
    out["nan point"] = z
    z = _normal(N, 12)
    z.real[1500] = 1e200
    out["1e200 point"] = z
    out["subnormal"] = _complex(1e-320 * rng.standard_normal(N), 1e-320 * rng.standard_normal(N))
    z = _normal(N, 13)
    z.imag[700], z.imag[2000] = np.inf, -np.inf
    out["inf in v"] = z
    return out


def test_acme_scores_of_degenerate_spectra_match_the_host():
    degs = _degenerate()
    got = proc_autophase.phase_scores(list(degs.values()), CANDIDATES, "acme")
    worst = 0.0
    for k, (name, z) in enumerate(degs.items()):
        want = _host_acme(z)
        w = _worst(got[k], want)
        assert w <= 1e-12, (name, got[k], want)
        worst = max(worst, w)
        print("  %-12s device %s  host %s" % (name, got[k], want))
    assert np.all(np.isnan(got[0])) and np.isnan(got[1, 0]) and np.all(np.isnan(got[2]))
    assert np.isinf(got[3]).any() and np.all(np.isnan(got[5]))
    assert np.all(got[4] > 0) and np.all(np.isfinite(got[4]))
    print("degenerate ACME scores: worst relative deviation %.3g" % worst)


def _fmin(z, fn="acme", p0=0.0, p1=0.0):
    with _quiet():
        xs, fs, its, fev, _ = scipy.optimize.fmin(proc_autophase._SCORES[fn], [p0, p1], args=(z,), disp=False,
                                                  full_output=True)
    return xs, fs, its, fev


def test_acme_optimiser_on_degenerate_spectra_matches_fmin_and_its_lone_calls():
    """fmin(full_output=True) on each degenerate spectrum: nfev and nit equal; x equal where the host stays at the
    start, else within 1e-8 degrees; f NaN where the host's is, else rtol 1e-12.  In one batch with normal spectra
    every member equals its lone call bit for bit: a NaN neighbour changes nothing.

    The constant spectrum is compared with its lone call only: near its optimum the slopes are differences of nearly
    equal rotated values, and an ulp of the rotation moves fmin's own end point by more than xatol
    (tests/test_phase_cpu.py::test_constant_spectrum_acme_end_point_is_set_by_rounding).  The device's sincos is not
    numpy's exp to the last ulp, so no bound tighter than that holds there; its deviation is printed."""
    degs = _degenerate()
    zs = [_normal(4096, 21)] + list(degs.values()) + [_normal(20000, 22)]
    names = ["normal 4096"] + list(degs) + ["normal 20000"]
    x, f, nfev, nit = proc_autophase.estimate_many(zs, "acme")
    worst_x = worst_f = 0.0
    for k, z in enumerate(zs):
        xs, fs, its, fev = _fmin(z)
        print("  %-12s nfev %d/%d nit %d/%d x %s / %s f %r / %r" % (names[k], nfev[k], fev, nit[k], its, x[k], xs, f[k], fs))
        lone = proc_autophase.estimate_many([z], "acme")
        _same(lone[0][0], x[k])
        _same(lone[1][0], f[k])
        assert (lone[2][0], lone[3][0]) == (nfev[k], nit[k])
        if names[k] == "constant":
            continue
        assert nfev[k] == fev and nit[k] == its, names[k]
        if np.all(xs == 0.0):
            _same(x[k], xs)
        else:
            assert np.all(np.abs(x[k] - xs) <= 1e-8), names[k]
        worst_x = max(worst_x, float(np.max(np.abs(x[k] - xs))))
        worst_f = max(worst_f, _worst([f[k]], [fs]))
        assert _worst([f[k]], [fs]) <= 1e-12, names[k]
    i = names.index("zeros")
    assert np.isnan(f[i]) and nfev[i] == 400 and nit[i] == 100
    i = names.index("nan point")
    assert np.isnan(f[i]) and nfev[i] == 400
    print("degenerate ACME optimiser: worst |dx| %.3g degrees, worst relative df %.3g" % (worst_x, worst_f))
    scores = proc_autophase.phase_scores(zs, CANDIDATES, "acme")
    for k, z in enumerate(zs):
        _same(proc_autophase.phase_scores([z], CANDIDATES, "acme")[0], scores[k])


# ---- peak minima at phase (0, 0) -------------------------------------------------------------------------------------

def _minima_base(N, seed=3):
    rng = np.random.default_rng(seed + N)
    return _complex(0.1 * rng.standard_normal(N), 0.1 * rng.standard_normal(N))


def _minima_case(N, case):
    nt = 512 if N >= 16384 else 256
    z = _minima_base(N)
    u = z.real
    if case == "tie 20 / 700":
        u[20] = u[700] = 5.0
    elif case == "tie 20 / 20+nt":
        u[20] = u[20 + nt] = 5.0
    elif case == "tie 700 / 300":
        u[700] = u[300] = 5.0
    elif case == "tie 300 / 300+nt":
        u[300] = u[300 + nt] = 5.0
    elif case == "nan 150, top 20":
        u[20], u[150] = 5.0, np.nan
    elif case == "nan 50":
        u[50] = np.nan
    elif case == "top 99":
        u[99] = 5.0
    elif case == "top 100":
        u[100] = 5.0
    elif case == "top N-1":
        u[N - 1] = 5.0
    elif case == "top N-50":
        u[N - 50] = 5.0
    z.real = u
    return z


MINIMA_CASES = ["tie 20 / 700", "tie 20 / 20+nt", "tie 700 / 300", "tie 300 / 300+nt", "nan 150, top 20", "nan 50",
                "top 99", "top 100", "top N-1", "top N-50"]
MINIMA_RAISES = {"tie 20 / 700", "tie 20 / 20+nt", "nan 50", "top 99"}


@pytest.mark.parametrize("N", [4096, 20000])
@pytest.mark.parametrize("case", MINIMA_CASES)
def test_peak_minima_rules_at_phase_zero_are_exact(N, case):
    """numpy's argmax (first NaN, else the first of equal maxima, across waves and within a thread), python's
    real[i-100:i] (empty for 0 < i < 100 once N > 100: np.min raises) and the right window clipped at N."""
    z = _minima_case(N, case)
    zero = [[0.0, 0.0]]
    try:
        want = proc_autophase._ps_peak_minima_score(zero[0], z)
    except ValueError:
        want = None
    assert (want is None) == (case in MINIMA_RAISES), (case, want)
    if want is None:
        with pytest.raises(ValueError, match="spectrum 1"):
            proc_autophase.phase_scores([_minima_base(N, 9), z], zero, "peak_minima")
        print("%s, N = %d: raises on both sides" % (case, N))
        return
    got = proc_autophase.phase_scores([_minima_base(N, 9), z], zero, "peak_minima")[1, 0]
    _same(got, want)
    if case.startswith("nan"):
        assert np.isnan(got)
    print("%s, N = %d: device %r host %r (exact)" % (case, N, got, want))


def _minima_escape(seed, N=4096):
    """the tallest point at N / 2, and at index 30 a slightly lower one whose phase turns it upright as fmin moves
    p0: the left window empties partway through the optimisation"""
    rng = np.random.default_rng(seed)
    z = 0.01 * (rng.standard_normal(N) + 1j * rng.standard_normal(N))
    z[N // 2] += 1.0
    z[30] += rng.uniform(0.5, 0.99) * np.exp(-1j * rng.uniform(0.05, 1.0))
    z[N // 2 + 100:N // 2 + 300] -= 0.2 * rng.uniform()
    return z


def test_peak_minima_optimiser_stops_where_fmin_raises():
    """fmin raises inside the score once the window is empty; the device reports the spectrum's status after the same
    number of calls, and estimate_many names the first such spectrum."""
    zs = [_normal(4096, 31), _minima_escape(1), _minima_escape(7)]
    calls = []

    def counted(ph, z):
        calls.append(1)
        return proc_autophase._ps_peak_minima_score(ph, z)

    host_nfev = [None]
    for z in zs[1:]:
        calls.clear()
        with pytest.raises(ValueError):
            scipy.optimize.fmin(counted, [0.0, 0.0], args=(z,), disp=False)
        host_nfev.append(len(calls))
    assert min(host_nfev[1:]) > 3                      # (not at the starting simplex)
    with pytest.raises(ValueError, match="spectrum 1"):
        proc_autophase.estimate_many(zs, "peak_minima")
    N, u, v = proc_autophase._pack(zs)
    S = len(zs)
    x0 = np.zeros((S, 2))
    x, f = np.zeros((S, 2)), np.zeros(S)
    nfev, nit, status = (np.zeros(S, dtype=np.int32) for _ in range(3))
    p = _cabi.ptr
    _cabi.check(_cabi.lib().nmrfit_phase_estimate(0, _cabi.PHASE_PEAK_MINIMA, S, p(N), p(u), p(v), p(x0), p(x), p(f),
                                                  p(nfev), p(nit), p(status)))
    print("peak minima window empties after host calls %s, device nfev %s, status %s" % (host_nfev[1:], nfev, status))
    _same(status, [0, 1, 1])
    assert list(nfev[1:]) == host_nfev[1:]
    xs, fs, its, fev = _fmin(zs[0], "peak_minima")
    assert (nfev[0], nit[0]) == (fev, its)


# ---- brute level -----------------------------------------------------------------------------------------------------

def _host_levels(u, v, angles, n):
    out = np.empty(len(angles))
    with _quiet():
        for m, a in enumerate(angles):
            V, _ = proc_autophase.ps2(u, v, a, 0.0)
            err = np.sqrt((V[:n].mean() - V[-n:].mean()) ** 2)
            out[m] = err if np.max(V) > abs(np.min(V)) else np.nan
    return out


BRUTE_ANGLES = np.concatenate([np.arange(-np.pi, np.pi, np.pi / 8), [0.0]])


def test_brute_means_around_numpys_pairwise_block_are_the_host_loops_values():
    """N = 39999 / 40000 (mean lengths 7 / 8: the plain loop against the 8-accumulator block), 44999 / 45000 (8 / 9: the
    tail) and 639999 / 644999 (127 / 128): every angle equals the host loop's value exactly."""
    Ns = (39999, 40000, 44999, 45000, 639999, 644999)
    zs = [_normal(N, 40 + k) for k, N in enumerate(Ns)]
    got = proc_autophase.brute_levels([z.real for z in zs], [z.imag for z in zs], BRUTE_ANGLES)
    upright = 0
    for k, (N, z) in enumerate(zip(Ns, zs)):
        want = _host_levels(z.real, z.imag, BRUTE_ANGLES, max(1, int(N / 5000)))
        _same(got[k], want)
        upright += int(np.isfinite(want).sum())
    assert upright >= len(Ns)
    print("brute means: %d spectra x %d angles equal the host loop (%d upright)" % (len(Ns), len(BRUTE_ANGLES), upright))


def test_brute_level_nan_rules():
    """max(V) == |min(V)| exactly at angle 0 (a real part of +-1) is not upright: NaN, as in the host loop.  A NaN
    point makes every angle NaN, and shift_phase_many('brute') then keeps p0 = 0, as the host does."""
    rng = np.random.default_rng(8)
    N = 3000
    tie = _complex(np.where(rng.random(N) < 0.5, -1.0, 1.0), 0.01 * rng.standard_normal(N))
    tie.real[0], tie.real[1] = 1.0, -1.0
    nan = _normal(N, 50)
    nan.real[1234] = np.nan
    got = proc_autophase.brute_levels([tie.real, nan.real], [tie.imag, nan.imag], BRUTE_ANGLES)
    _same(got[0], _host_levels(tie.real, tie.imag, BRUTE_ANGLES, 1))
    assert np.isnan(got[0, -1]) and np.isfinite(got[0]).any()
    assert np.all(np.isnan(got[1]))
    d, h = Data(np.arange(N, dtype=float), nan.real.copy(), nan.imag.copy()), Data(np.arange(N, dtype=float),
                                                                                    nan.real.copy(), nan.imag.copy())
    with _quiet():
        h.shift_phase("brute", step=np.pi / 30)
    shift_phase_many([d], "brute", step=np.pi / 30)
    assert (d.p0, d.p1) == (h.p0, h.p1) == (0, 0.0)
    print("brute NaN rules: angle 0 NaN on the +-1 spectrum, %d upright angles elsewhere; NaN point: p0 = 0"
          % int(np.isfinite(got[0]).sum()))


# ---- the brute mean length of a cropped Data -------------------------------------------------------------------------

def _twins(N, seed, P=4):
    sp = synth.make_spectrum(N, P, seed=seed, physical=True)
    noise = 0.002 * np.max(sp["u"]) * np.random.default_rng(seed + 100).standard_normal((2, N))
    return [Data(sp["w"], sp["u"] + noise[0], sp["v"] + noise[1]) for _ in range(2)]


def _crop(datas, lo_pct, hi_pct):
    lo, hi = np.percentile(datas[0].w, [lo_pct, hi_pct])
    for d in datas:
        d.select_bounds(lo, hi)


def _crop_around_peak(datas, half):
    d = datas[0]
    i = int(np.argmax(d.u))
    lo, hi = d.w[i - half - 1], d.w[i + half]
    for d in datas:
        d.select_bounds(lo, hi)


def _check_twins(pairs, step=np.pi / 360):
    """shift_phase_many on the device twins against shift_phase on the host twins: p0, p1 equal, V, I bit-identical"""
    for _, h in pairs:
        h.shift_phase("brute", step=step)
    shift_phase_many([d for d, _ in pairs], "brute", step=step)
    for k, (d, h) in enumerate(pairs):
        print("  Data %d: %d points: device p0 %r, host p0 %r" % (k, len(d.u), d.p0, h.p0))
        assert (d.p0, d.p1) == (h.p0, h.p1), (k, d.p0, h.p0)
        _same(d.V, h.V)
        _same(d.I, h.I)


def test_shift_phase_many_brute_on_data_cropped_before_any_shift_phase():
    """select_bounds crops u, v and leaves V: the host's mean length comes from the 65536 points (n = 13), not from
    the 19660 left (n = 3)."""
    d, h = _twins(65536, 0)
    _crop([d, h], 20, 50)
    assert len(d.u) == 19660 and len(d.V) == 65536
    _check_twins([(d, h)])


def test_shift_phase_many_brute_on_data_cropped_after_a_shift_phase():
    """the documented workflow: shift_phase, select_bounds, shift_phase again"""
    pairs = [_twins(65536, 1), _twins(40000, 2)]
    for d, h in pairs:
        d.shift_phase("brute")
        h.shift_phase("brute")
        _crop([d, h], 30, 60)
    _check_twins(pairs)


def test_shift_phase_many_brute_where_the_mean_is_longer_than_the_spectrum():
    """len(V) = 640000 cropped to 100 points: n = 128 > N, V[:n] and V[-n:] are the whole spectrum and the error is
    exactly 0 at every upright angle; the first upright angle wins on both sides."""
    d, h = _twins(640000, 3, P=2)
    _crop_around_peak([d, h], 50)
    assert len(d.u) == 100
    angles = np.arange(-np.pi, np.pi, np.pi / 360)
    err = proc_autophase.brute_levels([d.u], [d.v], angles, n=128)[0]
    fin = np.isfinite(err)
    assert fin.any() and np.all(err[fin] == 0.0)
    _check_twins([(d, h)])
    print("mean longer than the spectrum: %d upright angles, all with error 0" % int(fin.sum()))


def test_shift_phase_many_brute_on_a_mixed_batch_of_cropped_and_whole_data():
    pairs = [_twins(65536, 4), _twins(12000, 5), _twins(30000, 6)]
    _crop(pairs[0], 20, 50)
    pairs[2][0].shift_phase("manual")
    pairs[2][1].shift_phase("manual")
    _crop(pairs[2], 10, 40)
    _crop(pairs[2], 10, 90)                      # cropped twice: V is still the 30000 points of the first shift_phase
    _check_twins(pairs, step=np.pi / 180)


def test_shift_phase_many_brute_refuses_a_mean_length_above_128():
    d, _ = _twins(645000, 7, P=2)
    _crop_around_peak([d], 500)
    with pytest.raises(_cabi.NmrfitError, match="mean length of 129") as ei:
        shift_phase_many([d], "brute")
    assert ei.value.code == _cabi.E_UNSUPPORTED


# ---- float32 input ---------------------------------------------------------------------------------------------------

def test_float32_data_is_phased_as_its_float64_upcast():
    """The device path phases float32 input in float64: shift_phase_many on a float32 Data equals shift_phase_many on
    its float64 upcast exactly.  (How far that is from the host's float32 shift_phase is printed, not asserted.)"""
    sp = synth.make_spectrum(4096, 3, seed=60, physical=True)
    u32, v32 = sp["u"].astype(np.float32), sp["v"].astype(np.float32)
    for method in ("auto", "brute"):
        d32 = Data(sp["w"], u32, v32)
        d64 = Data(sp["w"], u32.astype(np.float64), v32.astype(np.float64))
        shift_phase_many([d32, d64], method)
        assert (d32.p0, d32.p1) == (d64.p0, d64.p1), method
        h32 = Data(sp["w"], u32, v32)
        with _quiet():
            h32.shift_phase(method)
        print("float32 '%s': device (%r, %r), host float32 (%r, %r), |dp0| %.3g rad"
              % (method, d32.p0, d32.p1, h32.p0, h32.p1, abs(d32.p0 - h32.p0)))

"""
CPU tier of the FID conditioning (nmrfit_amd/fid.py, csrc/fid_cond.hip, csrc/fid_ramp.h, include/nmrfit_amd_fid_cond.h):
the ctypes table against the header, the library's refusals (made before any device work), the Python argument errors,
the numpy restatement held to the definition independently (a long-double DFT matrix at s = 64, circular shifts for an
integer g, form 2 against form 1, make_fid(grpdly=) and its removal), the ramp values' stated bound against a truth of
113 bits, and the new kernels' resources.

Measured here: the ramp values of csrc/fid_ramp.h are within 0.7067 u of the exact ones (mu = 1 u) over all five group
delays and four lengths; tables filled from an angle reduced in fp64 are off by 340 u at g = 67.9.
"""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import nmrfit_amd
from nmrfit_amd import _cabi, fid, synth
from tests import fid_cond_support as fc
from tests import fid_support as fs

ROOT = fs.ROOT
HIPCC = "/opt/rocm/bin/hipcc"
HEADER = "nmrfit_amd_fid_cond.h"


def _declared(header):
    text = open(os.path.join(ROOT, "include", header)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return set(re.findall(r"\b(nmrfit_[a-z0-9_]+)\s*\(", text))


def test_table_and_header():
    names = _declared(HEADER)
    assert names == set(_cabi.FID_COND_SIGNATURES) == {"nmrfit_fid_condition_transform"}
    for header in sorted(os.listdir(os.path.join(ROOT, "include"))):
        if header.endswith(".h") and header != HEADER:
            assert not (names & _declared(header)), header
    for table in (_cabi.ALL_SIGNATURES, _cabi.PREP_SIGNATURES, _cabi.LSQ_SIGNATURES, _cabi.LSQ_IM_SIGNATURES, _cabi.NOISE_SIGNATURES,
                  _cabi.QUALITY_SIGNATURES, _cabi.BASELINE_SIGNATURES, _cabi.COV_SIGNATURES, _cabi.COV_IM_SIGNATURES,
                  _cabi.FID_SIGNATURES):
        assert not (names & set(table))
    L = _cabi.lib()
    assert hasattr(L, "nmrfit_fid_condition_transform") and L.nmrfit_abi_version() == _cabi.ABI_VERSION == 6
    assert len(L.nmrfit_fid_condition_transform.argtypes) == 17
    text = open(os.path.join(ROOT, "include", HEADER)).read()
    for name, value in (("NONE", fid.FORM_NONE), ("FID", fid.FORM_FID), ("SPECTRUM", fid.FORM_SPECTRUM)):
        assert "#define NMRFIT_FID_FORM_%s %d" % (name, value) in text
    assert "mu = 2^-53" in text and "At most 16 launches" in text and "normative ON ITS OWN" in text
    assert fid.condition_host is nmrfit_amd.fid.condition_host


# recorded from the library before the three entry points shared one body (tests/fid_support.refusal_table)
REFUSALS = fs.refusal_table([
    (_cabi.E_INVALID,
     'nmrfit_fid_condition_transform: every spectrum needs T > 0 and n_in > 0 (spectrum 1)',
     ('T = 0',)),
    (_cabi.E_INVALID,
     'nmrfit_fid_condition_transform: every spectrum needs T > 0 and n_in > 0 (spectrum 2)',
     ('n_in = -5',)),
    (_cabi.E_INVALID,
     "nmrfit_fid_condition_transform: a transform length is at least the conditioned trace's length "
     '(spectrum 1)',
     ("n < n_in', spectrum 1",)),
    (_cabi.E_INVALID,
     "nmrfit_fid_condition_transform: a transform length is at least the conditioned trace's length "
     '(spectrum 2)',
     ("n < n_in', spectrum 2",)),
    (_cabi.E_UNSUPPORTED,
     'nmrfit_fid_condition_transform: a transform length is a power of two, 2 .. 2^22 (spectrum 2): zero '
     'fill to the next power of two',
     ('n = 12', 'n = 2^23')),
    (_cabi.E_INVALID,
     "nmrfit_fid_condition_transform: a transform length is at least the conditioned trace's length "
     '(spectrum 0)',
     ("n < n_in', spectrum 0",)),
    (_cabi.E_INVALID,
     'nmrfit_fid_condition_transform: form is 0 (none), 1 (fid) or 2 (spectrum) (spectrum 1)',
     ('form = 3', 'form = 3 and n = 12')),
    (_cabi.E_INVALID,
     'nmrfit_fid_condition_transform: form is 0 (none), 1 (fid) or 2 (spectrum) (spectrum 0)',
     ('form = -1',)),
    (_cabi.E_INVALID,
     'nmrfit_fid_condition_transform: a group delay is finite and > 0 where a form is set (spectrum 1)',
     ('g = 0.0, spectrum 1', 'g = -1.0, spectrum 1', 'g = nan, spectrum 1', 'g = inf, spectrum 1')),
    (_cabi.E_INVALID,
     'nmrfit_fid_condition_transform: a group delay is finite and > 0 where a form is set (spectrum 0)',
     ('g = 0.0, spectrum 0', 'g = -1.0, spectrum 0', 'g = nan, spectrum 0', 'g = inf, spectrum 0')),
    (_cabi.E_UNSUPPORTED,
     'nmrfit_fid_condition_transform: form 1 (fid) needs a trace length that is a power of two, 2 .. 2^22 '
     '(spectrum 0): use form 2 (spectrum)',
     ('form 1 at 48 points',)),
    (_cabi.E_INVALID,
     'nmrfit_fid_condition_transform: form 1 (fid) needs a trace of at least 2 floor(g + 2) points '
     '(spectrum 0)',
     ('g = 31 at 64 points', 'g = 1e300')),
    (_cabi.E_INVALID,
     'nmrfit_fid_condition_transform: window_of is -1 or the index of a window (spectrum 1)',
     ('window_of = 2',)),
    (_cabi.E_INVALID,
     'nmrfit_fid_condition_transform: window_of is -1 or the index of a window (spectrum 0)',
     ('window_of = -2',)),
    (_cabi.E_INVALID,
     'nmrfit_fid_condition_transform: a window has as many values as the conditioned trace has points '
     '(spectrum 0)',
     ('10 values for 57 points', '64 values for 57 points')),
    (_cabi.E_INVALID,
     'nmrfit_fid_condition_transform: a window value is not finite (window 1)',
     ('a window value is nan', 'a window value is inf', 'a window value is -inf',
      'a window value is nan and n = 12')),
    (_cabi.E_UNSUPPORTED,
     'nmrfit_fid_condition_transform: a call takes at most 65535 spectra and 67108864 transformed values '
     '(T n summed over the spectra, plus T n_in of those in form 1)',
     ('17 x 2^22 values', '9 x 2^22 values in form 1')),
    (_cabi.E_INVALID,
     'nmrfit_fid_condition_transform: the number of spectra must be > 0 and n_in, n, T, fid, form, g, '
     'window_of, u_out, v_out, rows_out non-null',
     ('argument 0 null', 'argument 1 null', 'argument 2 null', 'argument 3 null', 'argument 4 null',
      'argument 5 null', 'argument 6 null', 'argument 10 null', 'argument 11 null', 'argument 12 null', 'K = 0')),
    (_cabi.E_INVALID,
     'nmrfit_fid_condition_transform: the number of windows must be >= 0, and window_len and windows '
     'non-null when it is > 0',
     ('M = 1 without arrays', 'M = -1')),
])


def _refusal_is_the_recorded_one(key, rc, message):
    assert (rc, message.decode()) == REFUSALS[key], key


def test_argument_validation_needs_no_gpu():
    """Every refusal of the header comes back before anything touches a device, with the code and the complete message of
    REFUSALS; a valid call reports the missing device (or, with a GPU, nothing)."""
    L = _cabi.lib()
    W = [np.linspace(1.0, 0.5, 64 - 7), np.ones(10)]
    base = dict(n_in=[64, 10, 5], n=[64, 16, 8], T=[2, 1, 1], x=np.zeros(2 * (2 * 64 + 10 + 5)), form=[1, 2, 0], g=[5.0, 67.9, 0.0],
                window_of=[0, 1, -1], windows=W)

    def call(**kw):
        a = dict(base)
        a.update(kw)
        return fc.raw_call(L, a["n_in"], a["n"], a["T"], a["x"], a["form"], a["g"], a["window_of"], a["windows"],
                           device=a.get("device", 0))[0]

    def refused(key, **kw):
        _refusal_is_the_recorded_one(key, call(**kw), L.nmrfit_last_error())
    assert call() in (_cabi.OK, _cabi.E_NO_DEVICE)
    assert call(form=[0, 0, 0], window_of=[-1, -1, -1], windows=[]) in (_cabi.OK, _cabi.E_NO_DEVICE)
    assert call(device=1 << 20) == _cabi.E_NO_DEVICE
    # those of nmrfit_fid_transform, with n >= n_in' in place of n >= n_in
    refused("T = 0", T=[2, 0, 1])
    refused("n_in = -5", n_in=[64, 10, -5])
    refused("n < n_in', spectrum 1", n=[64, 8, 8])
    refused("n < n_in', spectrum 2", n_in=[64, 10, 5], n=[64, 16, 4])
    refused("n = 12", n=[64, 16, 12])
    refused("n = 2^23", n=[64, 16, 1 << 23])
    # n >= n_in' is enough: 64 - 7 = 57 points fit a transform of 64, and would fit one of 64 with n_in = 64 only
    assert call(n=[64, 16, 8]) in (_cabi.OK, _cabi.E_NO_DEVICE)
    refused("n < n_in', spectrum 0", n=[32, 16, 8])
    # the new ones
    refused("form = 3", form=[1, 3, 0])
    refused("form = -1", form=[-1, 2, 0])
    for bad in (0.0, -1.0, np.nan, np.inf):
        refused("g = %r, spectrum 1" % bad, g=[5.0, bad, 0.0])
        refused("g = %r, spectrum 0" % bad, g=[bad, 67.9, 0.0])
    assert call(g=[5.0, 67.9, np.nan]) in (_cabi.OK, _cabi.E_NO_DEVICE)              # (not read where no form is set)
    refused("form 1 at 48 points", n_in=[48, 10, 5], windows=[np.ones(48 - 7), np.ones(10)])
    refused("g = 31 at 64 points", g=[31.0, 67.9, 0.0])                                # 64 < 2 * 33
    assert call(g=[30.0, 67.9, 0.0], window_of=[-1, 1, -1]) in (_cabi.OK, _cabi.E_NO_DEVICE)      # 64 = 2 * 32
    refused("g = 1e300", g=[1e300, 67.9, 0.0])
    refused("window_of = 2", window_of=[0, 2, -1])
    refused("window_of = -2", window_of=[-2, 1, -1])
    refused("10 values for 57 points", window_of=[1, 1, -1])
    refused("64 values for 57 points", windows=[np.ones(64), np.ones(10)])             # n_in, not n_in'
    for bad in (np.nan, np.inf, -np.inf):
        w = np.ones(10)
        w[7] = bad
        refused("a window value is %r" % bad, windows=[W[0], w])
    # the limits: T n summed, with T n_in of a form-1 job on top
    one = dict(n_in=[1 << 22], x=np.zeros(2), form=[0], g=[1.0], window_of=[-1], windows=[])
    refused("17 x 2^22 values", n=[1 << 22], T=[17], **one)
    one["form"] = [1]
    refused("9 x 2^22 values in form 1", n=[1 << 22], T=[9], **one)                    # 9 (n + n_in) > 2^26
    # a call that is wrong in two ways: the first refusal of the header's order wins
    refused("form = 3 and n = 12", form=[1, 3, 0], n=[64, 16, 12])
    refused("a window value is nan and n = 12", windows=[W[0], np.full(10, np.nan)], n=[64, 16, 12])
    # null pointers
    p = _cabi.ptr
    i64, i32 = (lambda a: np.array(a, dtype=np.int64)), (lambda a: np.array(a, dtype=np.int32))
    ok = [p(i64([8])), p(i64([8])), p(i32([1])), p(np.zeros(16)), p(i32([0])), p(np.zeros(1)), p(i32([-1])), 0, None, None,
          p(np.zeros(8)), p(np.zeros(8)), p(np.zeros(fid.ROW)), None, None]
    assert L.nmrfit_fid_condition_transform(0, 1, *ok) in (_cabi.OK, _cabi.E_NO_DEVICE)
    for at in (0, 1, 2, 3, 4, 5, 6, 10, 11, 12):
        args = list(ok)
        args[at] = None
        _refusal_is_the_recorded_one("argument %d null" % at, L.nmrfit_fid_condition_transform(0, 1, *args), L.nmrfit_last_error())
    _refusal_is_the_recorded_one("K = 0", L.nmrfit_fid_condition_transform(0, 0, *ok), L.nmrfit_last_error())
    args = list(ok)
    args[7] = 1                                                                         # a window, but no arrays
    _refusal_is_the_recorded_one("M = 1 without arrays", L.nmrfit_fid_condition_transform(0, 1, *args), L.nmrfit_last_error())
    args[7] = -1
    _refusal_is_the_recorded_one("M = -1", L.nmrfit_fid_condition_transform(0, 1, *args), L.nmrfit_last_error())


def test_python_argument_errors_come_before_the_library(monkeypatch):
    monkeypatch.setattr(_cabi, "lib", lambda: pytest.fail("the library was reached"))
    x, y = fs.sample_fid(256), fs.sample_fid(300)
    with pytest.raises(ValueError, match="grpdly_mode='spectrum'"):
        fid.transform_many([y], zero_fill="pow2", grpdly=68.0)                    # 300 is no power of two
    with pytest.raises(ValueError, match="grpdly_mode"):
        fid.transform_many([x], zero_fill="pow2", grpdly=68.0, grpdly_mode="post_proc")
    with pytest.raises(ValueError, match="zero_fill"):
        fid.transform_many([x], grpdly=68.0)                                      # 256 - 70 points need a zero fill
    for bad in (0.0, -3.0, np.nan, np.inf, 0.04):                                 # (0.04 rounds to 0.0)
        with pytest.raises(ValueError, match="grpdly"):
            fid.transform_many([x], zero_fill="pow2", grpdly=bad)
    with pytest.raises(ValueError, match="at least"):
        fid.transform_many([x], zero_fill="pow2", grpdly=127.0)                   # 256 < 2 * 129
    with pytest.raises(ValueError, match="one per FID"):
        fid.transform_many([x, x], zero_fill="pow2", grpdly=[68.0, 68.0, 68.0])
    with pytest.raises(ValueError, match="as many values"):
        fid.transform_many([x], zero_fill="pow2", grpdly=68.0, window=np.ones(256))      # n_in' = 186
    with pytest.raises(ValueError, match="as many values"):
        fid.transform_many([x], window=np.ones(255))
    with pytest.raises(ValueError, match="not finite"):
        fid.transform_many([x], window=np.full(256, np.nan))
    with pytest.raises(ValueError, match="one per FID"):
        fid.transform_many([x, x], window=[np.ones(256)])
    with pytest.raises(ValueError, match="one per FID"):
        fid.spectra_from_fids([x, x], 1.0, 1.0, 0.0, grpdly=[1.0, 2.0, 3.0], grpdly_mode="spectrum")
    with pytest.raises(ValueError, match="values per call"):
        fid.transform_many([np.zeros((9, 1 << 22), dtype=np.complex64)], grpdly=5.0, zero_fill="pow2")
    assert fid.grpdly_value(67.98416137695312) == 68.0 and fid.grpdly_value(67.94) == 67.9
    assert fid.grpdly_value(67.98416137695312, truncate_grpdly=False) == 67.98416137695312
    assert fid.conditioned_length(256, 68.0) == 186 and fid.conditioned_length(256, 67.9) == 187
    assert fid.conditioned_length(300, 68.0, "spectrum") == 300 and fid.conditioned_length(300) == 300
    assert fid._calls([9 << 22, 8 << 22]) == [(0, 1), (1, 2)]


def test_the_old_entry_point_is_called_when_nothing_is_asked(monkeypatch):
    calls = []

    class Lib:
        def nmrfit_fid_transform(self, *a):
            calls.append(("plain", len(a)))
            return 0

        def nmrfit_fid_condition_transform(self, *a):
            calls.append(("cond", len(a)))
            return 0
    monkeypatch.setattr(_cabi, "lib", lambda: Lib())
    x = fs.sample_fid(64)
    fid.transform_many([x])
    fid.transform_many([x], return_transform=True, grpdly=None, window=None)
    assert calls == [("plain", 10), ("plain", 10)]
    fid.transform_many([x], window=np.ones(64))
    fid.transform_many([x], grpdly=5.0, grpdly_mode="spectrum")
    fid.transform_many([x], return_conditioned=True)
    assert calls[2:] == [("cond", 17)] * 3


def test_windows_are_their_formulas():
    j = np.arange(100)
    assert fs.same_bits(fid.window_em(100, 2.0, 500.0), np.exp(-np.pi * 2.0 * j / 500.0))
    W = fid.window_em(100, 2.0, 500.0, first_point=0.5)
    assert W[0] == 0.5 and fs.same_bits(W[1:], fid.window_em(100, 2.0, 500.0)[1:])
    G = fid.window_gauss(100, 4.0, 500.0)
    t = j / 500.0
    assert np.allclose(G, np.exp(-(np.pi * 4.0 * t) ** 2 / (4 * np.log(2))), rtol=1e-15, atol=0) and G[0] == 1.0
    # (the Fourier transform of that Gaussian has full width gb at half height: exp(-f^2 4 ln 2 / gb^2) is 1/2 at f = gb / 2)
    S = fid.window_sine(101, 0.5, 1.0, 2.0)
    assert np.allclose(S, np.cos(0.5 * np.pi * np.arange(101) / 100) ** 2, atol=1e-15) and S[0] == 1.0
    assert fid.window_sine(5, 0.0, 1.0, 1.0, first_point=0.5)[0] == 0.0 and len(fid.window_sine(1)) == 1


# ---- condition_host against the definition, independently -------------------------------------------------------------

def _dft_matrix(s):
    """exp(-2 pi i j k / s) in long double, the exponent reduced mod s in integers."""
    jk = np.outer(np.arange(s), np.arange(s)) % s
    ang = -2 * np.arctan2(np.longdouble(0), np.longdouble(-1)) * jk.astype(np.longdouble) / s
    return np.cos(ang) + 1j * np.sin(ang)


def _definition(x, g, W=None):
    """Form 1 by the DFT matrix, long double: (y before the fold, the conditioned trace)."""
    s = x.shape[-1]
    F = _dft_matrix(s)
    k = np.arange(s)
    num, den = float(g).as_integer_ratio()      # g i / s mod 1 in integers
    frac = np.array([np.longdouble((num * int(i)) % (den * s)) / np.longdouble(den * s) for i in k])
    two_pi = 2 * np.arctan2(np.longdouble(0), np.longdouble(-1))
    rho = np.cos(two_pi * frac) + 1j * np.sin(two_pi * frac)
    B = (x.astype(np.clongdouble) @ F.T) * rho
    y = (B @ np.conj(F).T) / np.longdouble(s)
    skip, add = fc.skip_add(g)
    full = y.copy()
    jj = np.arange(add)
    y[:, jj] = y[:, jj] + y[:, s - 1 - jj]
    y = y[:, :s - skip]
    if W is not None:
        y = y * np.asarray(W, dtype=np.longdouble)
    return full, y


def test_condition_host_is_the_definition_at_64_points():
    s = 64
    x = fs.sample_fid(s, T=2, seed=11)
    for g in (0.3, 4.0, 5.0, 9.7, 12.25, 30.0):
        W = fid.window_em(s - fc.skip_add(g)[0], 1.5, 64.0, first_point=0.5)
        _, want = _definition(x, g, W)
        for dtype, tol in ((np.clongdouble, 2.0 ** -58), (np.complex128, None)):
            xc, Y = fid.condition_host(x.astype(dtype), g, "fid", W.astype(np.longdouble if dtype == np.clongdouble else np.float64), 128)
            assert xc.dtype == dtype and xc.shape == (2, s - fc.skip_add(g)[0]) and Y.shape == (2, 128)
            bar_c, _ = fc.bars(x, fid.FORM_FID, g, W, 128)
            err = np.sqrt((np.abs(xc.astype(np.clongdouble) - want) ** 2).sum(axis=-1)).astype(np.float64)
            # fp64: the device's own bar with numpy's twiddles (mu = 2 u) holds the restatement too; long double: 2^-58 of it
            limit = bar_c * (fs.eta(fs.MU_NUMPY) / fc.ETA) if tol is None else tol * fc.scale(x, fid.FORM_FID, g, W)
            print("g = %g, %s: error / limit %.3g" % (g, np.dtype(dtype).name, float((err / limit).max())))
            assert np.all(err <= limit), (g, dtype, err, limit)
            # the main transform of the conditioned trace, zero filled, centred
            assert np.allclose(Y.astype(np.clongdouble), fs.truth(xc, 128), rtol=0, atol=1e-12 * np.abs(Y).max())


def test_an_integer_group_delay_is_a_circular_shift():
    for s, g in ((64, 5), (256, 68), (512, 4), (100, 7)):
        x = fs.sample_fid(s, T=2, seed=12).astype(np.clongdouble)
        xc, _ = fid.condition_host(x, float(g), "fid", None, None if s == 100 else "pow2")
        skip, add = fc.skip_add(float(g))
        want = np.roll(x, -g, axis=-1)                     # y[j] = x[(j + g) mod s]
        jj = np.arange(add)
        want[:, jj] = want[:, jj] + want[:, s - 1 - jj]
        want = want[:, :s - skip]
        err = float(np.abs(xc - want).max() / np.abs(x).max())
        print("s = %d, g = %d: |y - shift| / max|x| = %.3g" % (s, g, err))
        assert xc.shape == want.shape and err <= 2.0 ** -55       # (long double: log2(s) 2^-64 each way)
        # before the fold and the cut, through the definition by the DFT matrix
        if s <= 64:
            full, _ = _definition(np.asarray(x, dtype=np.complex128), float(g))
            assert np.abs(full - np.roll(np.asarray(x, dtype=np.complex128), -g, axis=-1)).max() <= 2.0 ** -55 * np.abs(x).max()


def test_form_2_is_form_1_without_fold_and_cut_up_to_the_stated_factor():
    """For an integer g: Y2[i] = Y1[i] e^{-i pi g} (i < n / 2), Y1[i] e^{+i pi g} (i >= n / 2) -- both (-1)^g -- where Y1 is
    the centred transform of the ramped, uncut trace.  For any g, form 2 is the exact signed-frequency shift
    exp(2 pi i g (i - n/2) / n) times e^{+i pi g}."""
    s = 256
    x = fs.sample_fid(s, T=2, seed=13).astype(np.clongdouble)
    for g in (5.0, 68.0):
        _, Y2 = fid.condition_host(x, g, "spectrum")
        y_uncut = np.roll(x, -int(g), axis=-1)             # form 1 before fold and cut (the test above)
        Y1 = fs.truth(y_uncut)
        sign = (-1.0) ** int(g)
        assert np.abs(Y2 - sign * Y1).max() <= 2.0 ** -52 * np.abs(Y1).max()
    for g in (0.3, 67.9, 67.98416137695312):
        _, Y2 = fid.condition_host(x, g, "spectrum")
        i = np.arange(s, dtype=np.longdouble)
        two_pi = 2 * np.arctan2(np.longdouble(0), np.longdouble(-1))
        ang = two_pi * np.longdouble(g) * (i - s // 2) / s
        shift = (np.cos(ang) + 1j * np.sin(ang)) * (np.cos(two_pi * np.longdouble(g) / 2) + 1j * np.sin(two_pi * np.longdouble(g) / 2))
        assert np.abs(Y2 - fs.truth(x) * shift).max() <= 2.0 ** -50 * np.abs(Y2).max()
    # any length in the spectrum form, and the window alone
    xc, Y = fid.condition_host(fs.sample_fid(100), 3.3, "spectrum", np.full(100, 0.5), 128)
    assert xc.shape == (1, 100) and Y.shape == (1, 128) and fs.same_bits(xc, fs.sample_fid(100) * 0.5)
    neg = np.array([[complex(-0.0, 0.0), complex(1.0, -0.0), complex(-2.0, 3.0)]])
    xc, _ = fid.condition_host(neg, None, "fid", np.array([1.0, 2.0, -1.0]))
    assert fs.same_bits(xc.view(np.float64), np.array([[-0.0, 0.0, 2.0, -0.0, 2.0, -3.0]]))


def test_make_fid_with_a_group_delay_and_its_removal_return_the_fid():
    """The removal inverts the delay exactly (the ramp is unitary) up to rounding; what remains is the fold, which adds
    the FID's own tail x[s - 1 - j] to its first add points.  THE BAR: the tail's size, from the lines' decays --
    sum_l a_l exp(-d_l (s - 1 - add)) -- plus the noise-free rounding of four transforms, 4 log2(s) eta_numpy max|x| sqrt(s)."""
    s = 1024
    lines = [(0.11, 0.04, 1.0, 0.3), (-0.27, 0.05, 0.6, -1.0)]
    plain = synth.make_fid(s, lines, T=2, seed=3)
    assert fs.same_bits(plain.fid, synth.make_fid(s, lines, T=2, seed=3, grpdly=None).fid)
    for g in (68.0, 67.9, 5.0, 67.98416137695312):
        delayed = synth.make_fid(s, lines, T=2, seed=3, grpdly=g)
        assert fs.same_bits(delayed.clean, plain.clean) and delayed.fid.shape == plain.fid.shape
        assert np.abs(delayed.fid - plain.fid).max() > 0.1                                   # it IS delayed
        if g == int(g):
            assert np.abs(delayed.fid - np.roll(plain.fid, int(g), axis=-1)).max() < 1e-12
        xc, _ = fid.condition_host(delayed.fid, g, "fid", None, "pow2")
        skip, add = fc.skip_add(g)
        tail = sum(a * np.exp(-d * (s - 1 - add)) for _, d, a, _ in lines)
        rounding = 4 * np.log2(s) * fs.eta(fs.MU_NUMPY) * np.sqrt(s) * np.abs(plain.fid).max()
        err = float(np.abs(xc - plain.fid[:, :s - skip]).max())
        print("g = %r: |removed - undelayed| = %.3g, bar %.3g (tail %.3g + rounding %.3g)" % (g, err, tail + rounding, tail, rounding))
        assert err <= tail + rounding and tail < 1e-15


# ---- the ramp values and the kernels -----------------------------------------------------------------------------------

@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_the_ramp_values_are_within_the_stated_bound(tmp_path):
    """csrc/fid_ramp.h compiled for the host (tests/fid/ramp_check.hip): the table filler and the double-double split
    product against a truth of 113 bits, for g in {0.3, 5.0, 67.9, 68.0, 67.98416137695312} at n in {2, 256, 2^13, 2^22}:
    every index up to 2^13, a stride plus 10^6 random indices at 2^22.  The header's mu = u holds -- and does not with
    the angle reduced in floating point."""
    exe = str(tmp_path / "ramp_check")
    cc = subprocess.run([HIPCC, "--offload-arch=gfx950", "--cuda-host-only", "-O2", "-std=c++17", "-ffp-contract=on",
                         "-I" + os.path.join(ROOT, "nmrfit_amd", "csrc"), os.path.join(ROOT, "tests", "fid", "ramp_check.hip"),
                         "-o", exe], capture_output=True, text=True, timeout=300)
    assert cc.returncode == 0, cc.stderr[-3000:]

    def table(*args):
        run = subprocess.run([exe] + list(args), capture_output=True, text=True, timeout=300)
        assert run.returncode == 0, (run.returncode, run.stderr)
        return {(float(g), int(n)): float(w) for g, n, w in (ln.split() for ln in run.stdout.splitlines())}
    got = table()
    assert set(got) == {(g, n) for g in (0.3, 5.0, 67.9, 68.0, 67.98416137695312) for n in (2, 256, 1 << 13, 1 << 22)}
    worst = max(got.values())
    print("ramp values: worst |rho^ - rho| = %.4f u (mu = 1 u); per (g, n): %s" % (worst, got))
    assert all(w <= fs.MU_DEVICE / fs.U for w in got.values()) and worst > 0.0
    naive = table("naive")
    print("angle reduced in fp64: %.1f u at g = 67.9, n = 2^22" % naive[(67.9, 1 << 22)])
    assert naive[(67.9, 1 << 22)] > fs.MU_DEVICE / fs.U and naive[(0.3, 1 << 22)] > fs.MU_DEVICE / fs.U


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_kernel_resources():
    """tools/kernel_resources.py --unit fid_cond.hip: four kernels with the prefix fidc_, none with scratch memory or
    spills."""
    run = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"), "--check", "--unit", "fid_cond.hip"],
                         capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, run.stdout[-3000:] + run.stderr[-3000:]
    lines = [ln.split() for ln in run.stdout.splitlines()[1:] if ln.strip()]
    assert sorted(ln[0] for ln in lines) == ["fidc_ramp_kernel", "fidc_spectrum_kernel", "fidc_store_kernel", "fidc_window_kernel"], run.stdout
    for ln in lines:      # kernel VGPR AGPR scratch waves LDS s-spill
        assert int(ln[3]) == 0 and int(ln[6]) == 0 and int(ln[5]) == 0, ln
    print(run.stdout)
    src = open(os.path.join(ROOT, "nmrfit_amd", "csrc", "fid_cond.hip")).read()
    assert "atomic" not in src.replace("No LDS, no atomics", "") and "fid_cond" in open(os.path.join(ROOT, "nmrfit_amd", "csrc", "build.sh")).read()

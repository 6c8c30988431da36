"""
CPU tier of the FID transform (nmrfit_amd/fid.py, csrc/fid.hip, include/nmrfit_amd_fid.h): the numpy mirror of the
finishing stage against the reference's expression bit for bit, the restated transform against the long-double truth,
the synthetic FID's second truth (a geometric series) and its orientation, the ctypes table against the header, the
library's refusals (made before any device work), the twiddles' stated bound, the LDS swizzle's bank argument and the
kernels' resources.

Measured here: np.fft's own error is 0.33 u (n = 2) to 2.7 u (n = 2^17) in the 2-norm against bars of 7.7 u and 130 u;
the twiddle tables of csrc/fid_twiddle.h are within 0.66 u (stage) and 0.71 u (split) of the exact roots.
"""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import nmrfit_amd
from nmrfit_amd import _cabi, fid, synth
from tests import fid_support as fs

ROOT = fs.ROOT
HIPCC = "/opt/rocm/bin/hipcc"


def _reference(x, n=None):
    """The lines of core.load (nmrfit/core.py:51-60) on a (T, n_in) FID, with nmrglue's fft written out."""
    data = np.fft.fftshift(np.fft.fft(x, n=n, axis=-1), axes=-1)
    Y = data
    with np.errstate(all="ignore"):
        data = data / np.max(data)
    u, v = data.real.sum(axis=0), data.imag.sum(axis=0)
    return u[::-1], v[::-1], Y


def test_finish_host_is_the_reference_expression_bit_for_bit():
    branches, seen_T = set(), set()
    for T in (1, 3, 9):
        for phi in (0.0, 0.9, 1.8, 3.3, 5.7):
            x = synth.make_fid(64, [(0.1, 0.1, 1.0, phi)], T=T, seed=2, noise=0.01).fid
            u, v, Y = _reference(x)
            gu, gv, row = fid.finish_host(Y)
            assert fs.same_bits(gu, u) and fs.same_bits(gv, v), (T, phi)
            assert row[0] == 0 and row[4] == 64 and row[5] == T
            m = Y.ravel()[int(row[3])]
            assert m == np.max(Y) and (row[1], row[2]) == (m.real, m.imag)
            branches.add("first" if abs(row[1]) >= abs(row[2]) else "second")
            seen_T.add(T)
            hu, hv = fid.transform_host(x)
            assert fs.same_bits(hu, u) and fs.same_bits(hv, v)
    assert branches == {"first", "second"} and seen_T == {1, 3, 9}
    # a tie in the real part (n = 2: the transform is exact): the larger imaginary part wins; a full tie: the first index
    x = np.array([[1 + 1j, 0], [1 + 2j, 0], [1 + 2j, 0]])
    u, v, Y = _reference(x)
    assert np.all(Y.real == 1.0)
    gu, gv, row = fid.finish_host(Y)
    assert fs.same_bits(gu, u) and fs.same_bits(gv, v) and tuple(row) == (0.0, 1.0, 2.0, 2.0, 2.0, 3.0)
    # ties among designed values, in each Smith branch: equal real parts, the larger imaginary part wins, and of two
    # equal values the first
    rng = np.random.default_rng(3)
    for c, top in ((2.0, 0.5), (0.5, 30.0)):
        Y = -np.abs(rng.standard_normal((3, 16))) + 1j * rng.standard_normal((3, 16))
        Y[0, 1], Y[0, 3], Y[1, 2], Y[2, 7] = c - 5.0j, c + top * 1j, c + (top - 1.0) * 1j, c + top * 1j
        with np.errstate(all="ignore"):
            data = Y / np.max(Y)
        gu, gv, row = fid.finish_host(Y)
        assert fs.same_bits(gu, data.real.sum(axis=0)[::-1]) and fs.same_bits(gv, data.imag.sum(axis=0)[::-1])
        assert tuple(row[:4]) == (0.0, c, top, 3.0) and np.max(Y) == c + top * 1j


def test_ppm_axis_is_the_linspace_expression():
    for n, sw, sfrq, tof in ((16, 6410.3, 399.8, 1498.5), (65536, 100.0, 100.0, -350.0), (2, 1.0, 3.0, 0.0)):
        rangeppm, offsetppm = sw / sfrq, tof / sfrq
        w = np.linspace(rangeppm - offsetppm, -offsetppm, n)
        assert fs.same_bits(fid.ppm_axis(n, sw, sfrq, tof), w[::-1])


def test_transform_host_is_inside_the_bar():
    assert fs.truth_is_long_double()
    for n in fs.LENGTHS:
        x = fs.sample_fid(n - n // 3 if n > 4 else n, T=2)
        _, _, Y = fid.transform_host(x, n, return_transform=True)
        e2, einf = fs.errors(Y, fs.truth(x, n))
        print("np.fft, n = %d: 2-norm error %.3g u, worst point %.3g u, bar %.4g u" % (n, e2, einf, fs.bar(n, fs.MU_NUMPY) / fs.U))
        assert e2 * fs.U <= fs.bar(n, fs.MU_NUMPY) and einf * fs.U <= fs.bar(n, fs.MU_NUMPY)
    # complex64 widens exactly; a length numpy takes and the device does not
    x32 = fs.sample_fid(48).astype(np.complex64)
    a, b = fid.transform_host(x32), fid.transform_host(x32.astype(np.complex128))
    assert fs.same_bits(a[0], b[0]) and a[0].dtype == np.float64 and len(a[0]) == 48
    assert len(fid.transform_host(x32, "pow2")[0]) == 64


def test_make_fid_has_a_second_truth_and_says_where_the_lines_are():
    n_in, N = 200, 256
    lines = [(0.11, 0.02, 1.0), (-0.27, 0.03, 0.6, 0.4), (0.402, 0.05, 0.8, -0.2)]
    s = synth.make_fid(n_in, lines, T=2, seed=5)
    assert s.fid.shape == (2, n_in) and fs.same_bits(s.fid[0], s.clean) and fs.same_bits(s.fid[1], s.clean)
    X = s.exact_dft(N)
    want = np.fft.fft(s.clean.astype(np.clongdouble), n=N)
    # the series is exact in the parameters; ``clean`` carries the rounding of its own fp64 evaluation: per point the
    # argument (2 pi f - d) j is rounded (|arg| u) and exp, the product and the sum are (a few u)
    budget = sum(a * n_in * ((2 * np.pi * abs(f) + d) * n_in + 8.0) for f, d, a, _ in s.lines) * 2.0 * fs.U
    err = float(np.abs(X - want).max())
    print("geometric series against the long-double transform: %.3g (budget %.3g)" % (err, budget))
    assert err <= budget
    # orientation: in the output order every line's maximum of u sits at the index the series says
    for k, (f, d, a, ph) in enumerate(s.lines):
        one = synth.make_fid(n_in, [(f, d, a)], seed=1)
        u, v = fid.transform_host(one.fid, N)
        at = synth.SynthFid.line_index(f, N)
        assert abs(int(np.argmax(u)) - at) <= 0.5, (k, int(np.argmax(u)), at)
        exact = np.fft.fftshift(one.exact_dft(N))[::-1]
        assert int(np.argmax(exact.real)) == int(np.argmax(u))
    noisy = synth.make_fid(64, lines, T=3, seed=5, noise=0.1, offset=0.5)
    assert not fs.same_bits(noisy.fid[0], noisy.fid[1]) and abs(noisy.fid.mean() - 0.5) < 0.5
    assert fs.same_bits(noisy.fid, synth.make_fid(64, lines, T=3, seed=5, noise=0.1, offset=0.5).fid)


def test_statuses_of_the_mirror():
    u, v, row = fid.finish_host(np.zeros((2, 8), dtype=complex))
    assert row[0] == fid.ZERO and np.isnan(u).all() and np.isnan(v).all() and tuple(row[1:]) == (0.0, 0.0, 0.0, 8.0, 2.0)
    Y = fs.sample_fid(16, 2)
    for bad in (np.inf, -np.inf, np.nan, 1j * np.inf):
        Z = Y.copy()
        Z[1, 3] = bad
        u, v, row = fid.finish_host(Z)
        assert row[0] == fid.NOT_FINITE and np.isnan(u).all() and np.isnan(v).all() and np.isnan(row[1:4]).all()
        assert tuple(row[4:]) == (16.0, 2.0)
    # m == 0 with other values below it is status 1 too
    Z = -np.abs(Y.real) + 0j
    Z[0, 0] = 0.0
    assert fid.finish_host(Z)[2][0] == fid.ZERO


def _declared(header):
    text = open(os.path.join(ROOT, "include", header)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return set(re.findall(r"\b(nmrfit_[a-z0-9_]+)\s*\(", text))


def test_table_and_header():
    names = _declared("nmrfit_amd_fid.h")
    assert names == set(_cabi.FID_SIGNATURES) == {"nmrfit_fid_transform"}
    for header in sorted(os.listdir(os.path.join(ROOT, "include"))):
        if header.endswith(".h") and header != "nmrfit_amd_fid.h":
            assert not (names & _declared(header)), header
    for table in (_cabi.ALL_SIGNATURES, _cabi.PREP_SIGNATURES, _cabi.LSQ_SIGNATURES, _cabi.LSQ_IM_SIGNATURES, _cabi.NOISE_SIGNATURES,
                  _cabi.QUALITY_SIGNATURES, _cabi.BASELINE_SIGNATURES, _cabi.COV_SIGNATURES, _cabi.COV_IM_SIGNATURES):
        assert not (names & set(table))
    assert len(_declared("nmrfit_amd.h")) == 46
    L = _cabi.lib()
    assert hasattr(L, "nmrfit_fid_transform") and L.nmrfit_abi_version() == _cabi.ABI_VERSION == 6
    text = open(os.path.join(ROOT, "include", "nmrfit_amd_fid.h")).read()
    assert "#define NMRFIT_FID_ROW %d" % fid.ROW in text and "#define NMRFIT_FID_MAX_LOG2 %d" % fid.MAX_LOG2 in text
    assert "#define NMRFIT_FID_LDS_LOG2 %d" % fid.LDS_LOG2 in text and fs.LDS_LOG2 == fid.LDS_LOG2
    assert "mu = 2^-53" in text and fs.MU_DEVICE == 2.0 ** -53
    assert nmrfit_amd.fid is fid and nmrfit_amd.spectra_from_fids is fid.spectra_from_fids


# recorded from the library before the three entry points shared one body (tests/fid_support.refusal_table)
REFUSALS = fs.refusal_table([
    (_cabi.E_INVALID,
     'nmrfit_fid_transform: the number of spectra must be > 0 and n_in, n, T, fid, u_out, v_out, rows_out '
     'non-null',
     ('n_in null', 'n null', 'T null', 'x null', 'u null', 'v null', 'rows null', 'K = 0', 'K = -3')),
    (_cabi.E_INVALID,
     'nmrfit_fid_transform: every spectrum needs T > 0 and n_in > 0 (spectrum 1)',
     ('T = 0', 'n_in = -8', 'T = 0 and n = 6')),
    (_cabi.E_INVALID,
     'nmrfit_fid_transform: every spectrum needs T > 0 and n_in > 0 (spectrum 0)',
     ('T = -1', 'n_in = 0')),
    (_cabi.E_INVALID,
     "nmrfit_fid_transform: a transform length is at least the trace's length (spectrum 0)",
     ('n < n_in, spectrum 0',)),
    (_cabi.E_INVALID,
     "nmrfit_fid_transform: a transform length is at least the trace's length (spectrum 1)",
     ('n < n_in, spectrum 1',)),
    (_cabi.E_UNSUPPORTED,
     'nmrfit_fid_transform: a transform length is a power of two, 2 .. 2^22 (spectrum 1): zero fill to the'
     ' next power of two',
     ('n = 6', 'n = 12', 'n = 1', 'n = 4194306', 'n = 8388608')),
    (_cabi.E_UNSUPPORTED,
     'nmrfit_fid_transform: a call takes at most 65535 spectra and 67108864 transformed values (T n summed'
     ' over the spectra)',
     ('65536 spectra', '17 x 2^22 values', '2^26 + 2 values', '2^54 values')),
])


def _refusal_is_the_recorded_one(key, rc, message):
    assert (rc, message.decode()) == REFUSALS[key], key


def test_argument_validation_needs_no_gpu():
    """Every refusal of the header comes back before anything touches a device, with the code and the complete message of
    REFUSALS; an impossible device index is answered by the shared check with the message nmrfit_weights_build gives."""
    L = _cabi.lib()
    p = _cabi.ptr
    i32, i64 = (lambda a: np.array(a, dtype=np.int32)), (lambda a: np.array(a, dtype=np.int64))
    n_in, n, T = i64([3, 8]), i64([4, 8]), i32([2, 1])
    x = np.zeros(2 * (2 * 3 + 8))
    u, v, rows, Z = np.zeros(12), np.zeros(12), np.zeros(2 * fid.ROW), np.zeros(2 * 16)

    def call(device=0, K=2, n_in=n_in, n=n, T=T, x=x, u=u, v=v, rows=rows, Z=Z):
        return L.nmrfit_fid_transform(device, K, p(n_in), p(n), p(T), p(x), p(u), p(v), p(rows), p(Z))

    def refused(key, rc):
        _refusal_is_the_recorded_one(key, rc, L.nmrfit_last_error())
    for name in ("n_in", "n", "T", "x", "u", "v", "rows"):
        refused(name + " null", call(**{name: None}))
    refused("K = 0", call(K=0))
    refused("K = -3", call(K=-3))
    refused("T = 0", call(T=i32([2, 0])))
    refused("T = -1", call(T=i32([-1, 1])))
    refused("n_in = 0", call(n_in=i64([0, 8])))
    refused("n_in = -8", call(n_in=i64([3, -8])))
    refused("n < n_in, spectrum 0", call(n_in=i64([5, 8])))
    refused("n < n_in, spectrum 1", call(n_in=i64([3, 9]), n=i64([4, 8])))
    for bad in (6, 12, 1, (1 << 22) + 2, 1 << 23):
        refused("n = %d" % bad, call(n_in=i64([1, 1]), n=i64([4, bad])))
    many = 65536
    refused("65536 spectra", L.nmrfit_fid_transform(0, many, p(np.ones(many, dtype=np.int64)), p(np.full(many, 2, dtype=np.int64)),
                                                    p(np.ones(many, dtype=np.int32)), p(x), p(u), p(v), p(rows), None))
    refused("17 x 2^22 values", call(n_in=i64([1, 1]), n=i64([1 << 22, 1 << 22]), T=i32([8, 9])))
    refused("2^26 + 2 values", call(n_in=i64([1, 1]), n=i64([2, 2]), T=i32([1 << 25, 1])))
    refused("2^54 values", call(n_in=i64([1, 1]), n=i64([1 << 22, 1 << 22]), T=i32([2 ** 31 - 1, 2 ** 31 - 1])))
    # a call that is wrong in two ways: the first refusal of the header's order wins
    refused("T = 0 and n = 6", call(T=i32([2, 0]), n_in=i64([1, 1]), n=i64([4, 6])))
    # valid calls: what is reported then is the missing device (or, with a GPU, nothing)
    assert call() in (_cabi.OK, _cabi.E_NO_DEVICE)
    assert call(Z=None) in (_cabi.OK, _cabi.E_NO_DEVICE)
    assert call(device=1 << 20) == _cabi.E_NO_DEVICE
    mine = L.nmrfit_last_error()
    out = np.zeros(7)
    assert L.nmrfit_weights_build(1 << 20, 2, p(i64([4, 3])), p(np.arange(7.0)), p(i32([0, 0])), None, None, p(out), None) == _cabi.E_NO_DEVICE
    assert mine == L.nmrfit_last_error() and mine


def test_python_argument_errors_come_before_the_library(monkeypatch):
    monkeypatch.setattr(_cabi, "lib", lambda: pytest.fail("the library was reached"))
    x = fs.sample_fid(48)
    with pytest.raises(ValueError, match="zero_fill"):
        fid.transform_many([x])                                   # 48 is no power of two
    with pytest.raises(ValueError, match="zero_fill"):
        fid.transform_many([x], zero_fill=96)
    with pytest.raises(ValueError, match="zero_fill"):
        fid.transform_many([x], zero_fill=32)                     # shorter than the trace
    with pytest.raises(ValueError, match="zero_fill"):
        fid.transform_many([x], zero_fill="next")
    with pytest.raises(ValueError, match="zero_fill"):
        fid.transform_many([fs.sample_fid(1)])                    # n = 1
    with pytest.raises(ValueError, match="zero_fill"):
        fid.transform_many([np.zeros((1 << 22) + 1, dtype=np.complex64)], zero_fill="pow2")
    with pytest.raises(ValueError):
        fid.transform_many([x.real])
    with pytest.raises(ValueError):
        fid.transform_many([np.zeros((2, 2, 8), dtype=complex)])
    with pytest.raises(ValueError):
        fid.transform_many([np.zeros((0, 8), dtype=complex)])
    with pytest.raises(ValueError, match="values per call"):
        fid.transform_many([np.zeros((17, 1), dtype=np.complex64)], zero_fill=1 << 22)
    with pytest.raises(ValueError, match="one per FID"):
        fid.spectra_from_fids([x, x], [1.0, 2.0, 3.0], 1.0, 0.0, zero_fill="pow2")
    assert fid.transform_many([]) == []
    assert [fid.transform_length(k, "pow2") for k in (1, 2, 3, 64, 65, 1 << 22)] == [2, 2, 4, 64, 128, 1 << 22]
    assert fid._calls([1 << 25, 1 << 25, 1, 1 << 26]) == [(0, 2), (2, 3), (3, 4)] and fid._calls([]) == []


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_the_twiddles_are_within_the_stated_bound(tmp_path):
    """csrc/fid_twiddle.h compiled for the host (tests/fid/twiddle_check.hip): the stage table and the double-double
    split product against cosl / sinl, over whole transforms of 2^13, 2^16, 2^17 points, a stride through 2^22 and two
    million random indices.  The header's mu = u holds; the exact roots are exact."""
    exe = str(tmp_path / "twiddle_check")
    cc = subprocess.run([HIPCC, "--offload-arch=gfx950", "--cuda-host-only", "-O1", "-std=c++17", "-ffp-contract=on",
                         "-I" + os.path.join(ROOT, "nmrfit_amd", "csrc"), os.path.join(ROOT, "tests", "fid", "twiddle_check.hip"),
                         "-o", exe], capture_output=True, text=True, timeout=300)
    assert cc.returncode == 0, cc.stderr[-3000:]
    run = subprocess.run([exe, "13", "16", "17", "22"], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, (run.returncode, run.stderr)
    stage, split = (float(t) for t in run.stdout.split())
    print("twiddles: stage table %.4f u, split product %.4f u (mu = 1 u)" % (stage, split))
    assert 0.0 < stage <= fs.MU_DEVICE / fs.U and 0.0 < split <= fs.MU_DEVICE / fs.U


def test_the_swizzle_spreads_every_store_pattern_over_the_banks():
    """csrc/fid.hip, THE LDS BLOCK (restated in tests/fid_support.swz, held to the source's constants here): a store
    group is 16 consecutive lanes on 16 eight-byte slots (32 banks), a ds_read_b64 group 32 lanes on 32 slots (64
    banks).  Every pattern the kernels store with lands its 16 lanes on 16 slots, wherever in the block it starts;
    unswizzled the same patterns collide up to 16-fold; reads are unit stride."""
    src = open(os.path.join(ROOT, "nmrfit_amd", "csrc", "fid.hip")).read()
    assert "return a ^ ((-(h & 1) & 15) ^ (-((h >> 1) & 1) & 10) ^ ((h >> 2) & 7));" in src and "const int h = a >> 4;" in src
    block = 1 << fid.LDS_LOG2
    assert sorted(fs.swz(a) for a in range(block)) == list(range(block))
    assert all(fs.swz(a) >> 4 == a >> 4 for a in range(block))          # inside an aligned block of 16: any block length
    worst_plain = 0
    for name, variants in fs.store_patterns().items():
        for pat in variants:
            span = 16
            while span <= max(pat):
                span *= 2
            for base in range(0, block, span):
                assert len(set(fs.swz(base + a) & 15 for a in pat)) == 16, (name, base)
            worst_plain = max(worst_plain, 16 // len(set(a & 15 for a in pat)))
    assert worst_plain == 16
    for base in range(0, block, 32):
        assert len(set(fs.swz(base + i) & 31 for i in range(32))) == 32


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_kernel_resources():
    """tools/kernel_resources.py --check --unit fid.hip: six kernels, none with scratch memory or spills; the three
    transform kernels within 128 VGPRs (two workgroups of four waves per CU is what 64 KiB of LDS allows anyway)."""
    run = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"), "--check", "--unit", "fid.hip"],
                         capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, run.stdout[-3000:] + run.stderr[-3000:]
    lines = [ln.split() for ln in run.stdout.splitlines() if ln.startswith("fid_")]
    assert sorted(ln[0] for ln in lines) == ["fid_finish_kernel", "fid_max_kernel", "fid_max_part_kernel", "fid_pass1_kernel",
                                             "fid_pass2_kernel", "fid_short_kernel"], run.stdout
    for ln in lines:      # kernel VGPR AGPR scratch waves LDS s-spill
        assert int(ln[3]) == 0 and int(ln[6]) == 0 and int(ln[1]) <= 128, ln
    print(run.stdout)

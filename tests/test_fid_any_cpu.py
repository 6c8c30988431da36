"""
CPU tier of the any-length FID transform (nmrfit_amd/fid.py, csrc/fid_any.hip, csrc/fid_chirp.h,
include/nmrfit_amd_fid_any.h): the numpy restatement of the chirp-z definition against numpy's own transform of the same
length within the header's bar, the centring by index for odd and even N, the chirp values' stated bound against a truth
of 113 bits, the lengths transform_length takes, the ctypes table against the header, the library's refusals (made
before any device work) and the kernels' resources.

Measured here: the chirp values of csrc/fid_chirp.h are within 0.7067 u of the exact ones (mu = 1 u) over the eight
lengths; a table filled from pi k^2 / N formed in fp64 is off by 1.3e7 u at N = 2^21 - 1.
"""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import nmrfit_amd
from nmrfit_amd import _cabi, fid
from tests import fid_any_support as fa
from tests import fid_support as fs

ROOT = fs.ROOT
HIPCC = "/opt/rocm/bin/hipcc"
HEADER = "nmrfit_amd_fid_any.h"
HOST_LENGTHS = (3, 5, 6, 7, 12, 100, 1000, 2047, 2049, 4027, 4099)


def _declared(header):
    text = open(os.path.join(ROOT, "include", header)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return set(re.findall(r"\b(nmrfit_[a-z0-9_]+)\s*\(", text))


def test_table_and_header():
    names = _declared(HEADER)
    assert names == set(_cabi.FID_ANY_SIGNATURES) == {"nmrfit_fid_transform_any"}
    for header in sorted(os.listdir(os.path.join(ROOT, "include"))):
        if header.endswith(".h") and header != HEADER:
            assert not (names & _declared(header)), header
    assert _cabi.FID_ANY_SIGNATURES["nmrfit_fid_transform_any"] == _cabi.FID_COND_SIGNATURES["nmrfit_fid_condition_transform"]
    L = _cabi.lib()
    assert hasattr(L, "nmrfit_fid_transform_any") and L.nmrfit_abi_version() == _cabi.ABI_VERSION == 6
    assert len(L.nmrfit_fid_transform_any.argtypes) == 17
    text = open(os.path.join(ROOT, "include", HEADER)).read()
    assert "#define NMRFIT_FID_ANY_MIN %d" % fid.ANY_MIN in text and "#define NMRFIT_FID_ANY_MAX %d" % fid.ANY_MAX in text
    assert "mu = 2^-53" in text and "At most 27 launches" in text and "floor(N / 2)" in text
    assert fid.bluestein_host is nmrfit_amd.fid.bluestein_host


@pytest.mark.parametrize("N", HOST_LENGTHS)
def test_bluestein_host_is_numpys_transform_of_the_same_length(N):
    """fp64, against np.fft.fftshift(np.fft.fft(x, N)), n_in' in {1, N - 1, N}, T = 2: inside the header's bar with numpy's
    twiddles (mu = 2 u: the restatement's transforms are np.fft's), in the 2-norm and at every point.  The long-double
    restatement agrees with numpy's long-double transform to 2^-58 of the spectrum's norm."""
    rng = np.random.default_rng(N)
    for n_in in (1, N - 1, N):
        x = rng.standard_normal((2, n_in)) + 1j * rng.standard_normal((2, n_in))
        want = np.fft.fftshift(np.fft.fft(x, N, axis=-1), axes=-1)
        got = fid.bluestein_host(x, N)
        assert got.dtype == np.complex128 and got.shape == (2, N)
        limit = fa.bar(x, N, mu=fs.MU_NUMPY)
        err = np.abs(got - want)
        e2 = np.sqrt((err ** 2).sum(axis=-1))
        print("N = %d, n_in' = %d: error / bar %.3g (2-norm), %.3g (worst point)" % (N, n_in, float((e2 / limit).max()),
                                                                                    float((err.max(axis=-1) / limit).max())))
        assert np.all(e2 <= limit) and np.all(err.max(axis=-1) <= limit)
        if fs.truth_is_long_double():
            long = fid.bluestein_host(x.astype(np.clongdouble), N)
            ref = fs.truth(x, N)
            assert long.dtype == np.clongdouble
            assert float(np.abs(long - ref).max()) <= 2.0 ** -58 * float(np.sqrt((np.abs(ref) ** 2).sum(axis=-1)).max())


@pytest.mark.parametrize("N", HOST_LENGTHS)
def test_centring_is_fftshift_by_index_for_odd_and_even_lengths(N):
    """A delta at point 0 transforms to all ones, so it cannot tell the order; exp(2 pi i f k / N) transforms to N at
    frequency f alone: for every f the peak sits where fftshift puts it, index (f + N // 2) mod N."""
    k = np.arange(N)
    for f in sorted({0, 1, N // 2 - 1, N // 2, (N + 1) // 2, N - 1} & set(range(N))):
        x = np.exp(2j * np.pi * ((f * k) % N) / N)
        Y = fid.bluestein_host(x, N)[0]
        want = np.fft.fftshift(np.fft.fft(x))
        at = int(np.argmax(np.abs(Y)))
        assert at == int(np.argmax(np.abs(want))) == (f + N // 2) % N, (N, f, at)
        others = np.delete(np.abs(Y), at)
        assert abs(Y[at] - N) <= 1e-9 * N and (others.size == 0 or others.max() <= 1e-9 * N)
    # and the delta itself at every place: Y[i] = exp(-2 pi i d (i - N // 2) / N)
    for d in sorted({0, 1, N - 1}):
        x = np.zeros(N, dtype=np.complex128)
        x[d] = 1.0
        Y = fid.bluestein_host(x, N)[0]
        q = (k - N // 2) % N
        assert np.abs(Y - np.exp(-2j * np.pi * ((d * q) % N) / N)).max() <= 1e-9


def test_the_mirror_gives_a_tie_to_the_first_copy():
    """The host side of tests/test_gpu_fid_any.py's tie construction (fa.TIES): of equal rows of a stacked Y, finish_host
    takes the maximum in the first, wherever the copies lie."""
    for name, n, T, placements in fa.TIES:
        row = fid.bluestein_host(fs.sample_fid(n, 1, seed=97), n)[0]
        assert (8192 // n) in placements[0] and T * n > 8192 and row.real.max() > 0.0
        for hi_at in placements:
            Y = fa.tie_stack(row, T, hi_at)
            u, v, out = fid.finish_host(Y)
            assert out[0] == 0 and int(out[3]) // n == hi_at[0] and int(out[3]) % n == int(np.argmax(row.real)), (name, hi_at)
            assert complex(out[1], out[2]) == Y[hi_at[0], int(out[3]) % n] == np.max(Y)


def test_transform_length_takes_any_length_on_request_only():
    for n in HOST_LENGTHS + (65466, (1 << 21) - 1):
        assert fid.transform_length(n, None, any_length=True) == n
        assert fid.transform_length(n - 1, n, any_length=True) == n
        with pytest.raises(ValueError, match="zero_fill"):
            fid.transform_length(n)
    for n in (2, 64, 1 << 22):
        assert fid.transform_length(n, None, any_length=True) == fid.transform_length(n) == n
    assert fid.transform_length(4027, "pow2", any_length=True) == 4096
    for n in (1, (1 << 21) + 1, (1 << 22) + 2):
        with pytest.raises(ValueError, match="zero_fill"):
            fid.transform_length(n, None, any_length=True)
    with pytest.raises(ValueError, match="shorter"):
        fid.transform_length(100, 99, any_length=True)
    assert fid.conv_length(3) == 8 and fid.conv_length(2047) == 4096 and fid.conv_length(2049) == 8192
    assert fid.conv_length((1 << 21) - 1) == 1 << 22


def test_python_argument_errors_come_before_the_library(monkeypatch):
    monkeypatch.setattr(_cabi, "lib", lambda: pytest.fail("the library was reached"))
    x = fs.sample_fid(300)
    with pytest.raises(ValueError, match="zero_fill"):
        fid.transform_many([x])                                                   # as before: refused by default
    with pytest.raises(ValueError, match="grpdly_mode='spectrum' needs"):
        fid.transform_many([x], grpdly=5.0, grpdly_mode="spectrum", any_length=True)
    with pytest.raises(ValueError, match="zero_fill"):
        fid.transform_many([fs.sample_fid(256)], grpdly=68.0)                     # as before: form 1 needs a zero fill
    with pytest.raises(ValueError, match="values per call"):
        fid.transform_many([np.zeros((9, (1 << 21) - 1), dtype=np.complex64)], any_length=True)      # 9 (n + 2 M) > 2^26
    # the cut of a list counts the filter planes once per distinct length of a call
    M = 1 << 22
    assert fid._calls([1, 1], [(7, M), (7, M)]) == [(0, 2)]
    assert fid._calls([1 << 25, 1 << 25], [(5, 1), (5, 1)]) == [(0, 1), (1, 2)]
    assert fid._calls([(1 << 25) - 1, 1 << 25], [(5, 1), (5, 1)]) == [(0, 2)]
    assert fid._calls([(1 << 25) - 1, 1 << 25], [(5, 1), (6, 1)]) == [(0, 1), (1, 2)]


def test_the_entry_points_are_chosen_by_the_lengths_of_a_call(monkeypatch):
    calls = []

    class Lib:
        def nmrfit_fid_transform(self, *a):
            calls.append(("plain", len(a)))
            return 0

        def nmrfit_fid_condition_transform(self, *a):
            calls.append(("cond", len(a)))
            return 0

        def nmrfit_fid_transform_any(self, *a):
            calls.append(("any", len(a)))
            return 0
    monkeypatch.setattr(_cabi, "lib", lambda: Lib())
    x, y = fs.sample_fid(64), fs.sample_fid(100)
    fid.transform_many([x], any_length=True)                                      # a power of two: the way it went
    fid.transform_many([x], window=np.ones(64), any_length=True)
    fid.transform_many([y], any_length=True)
    fid.transform_many([x, y], any_length=True, return_transform=True)
    fid.transform_many([x], grpdly=5.0, any_length=True)                          # 64 - 7 = 57 points, at 57
    assert calls == [("plain", 10), ("cond", 17), ("any", 17), ("any", 17), ("any", 17)]


# recorded from the library before the three entry points shared one body (tests/fid_support.refusal_table)
REFUSALS = fs.refusal_table([
    (_cabi.E_UNSUPPORTED,
     'nmrfit_fid_transform_any: form 2 (spectrum) needs a transform length that is a power of two '
     '(spectrum 1): its ramp tables are split at 2^11; use form 1 (fid), or zero fill',
     ('form 2 at n = 12',)),
    (_cabi.E_UNSUPPORTED,
     'nmrfit_fid_transform_any: a transform length is a power of two, 2 .. 2^22, or any other length, 3 ..'
     ' 2^21 - 1 (spectrum 1)',
     ('n = 2^21 + 1', 'n = 1', 'n = 2^23')),
    (_cabi.E_INVALID,
     "nmrfit_fid_transform_any: a transform length is at least the conditioned trace's length (spectrum 0)",
     ("n < n_in'",)),
    (_cabi.E_INVALID,
     'nmrfit_fid_transform_any: every spectrum needs T > 0 and n_in > 0 (spectrum 1)',
     ('T = 0',)),
    (_cabi.E_INVALID,
     'nmrfit_fid_transform_any: form is 0 (none), 1 (fid) or 2 (spectrum) (spectrum 1)',
     ('form = 3', 'form = 3 and n = 2^21 + 1')),
    (_cabi.E_UNSUPPORTED,
     'nmrfit_fid_transform_any: a call takes at most 65535 spectra and 67108864 transformed values (T n '
     'summed over the spectra, plus T n_in of those in form 1, plus 2 T M of those whose n is no power of '
     'two and 2 M per distinct such n)',
     ('6 traces of 2^21 - 1', '2^26 values and a chirp job')),
    (_cabi.E_UNSUPPORTED,
     'nmrfit_fid_condition_transform: a transform length is a power of two, 2 .. 2^22 (spectrum 0): zero '
     'fill to the next power of two',
     ('n = 12 at the old entry point',)),
])


def _refusal_is_the_recorded_one(key, rc, message):
    assert (rc, message.decode()) == REFUSALS[key], key


def test_argument_validation_needs_no_gpu():
    """Every refusal of the new entry point comes back before anything touches a device, with the code and the complete
    message of REFUSALS; a valid call reports the missing device (or, with a GPU, nothing)."""
    L = _cabi.lib()
    base = dict(n_in=[64, 10, 5], n=[57, 12, 8], T=[2, 1, 1], x=np.zeros(2 * (2 * 64 + 10 + 5)), form=[1, 0, 2], g=[5.0, 0.0, 3.3],
                window_of=[0, -1, -1], windows=[np.linspace(1.0, 0.5, 57)])

    def call(**kw):
        a = dict(base)
        a.update(kw)
        return fa.raw_call(L, a["n_in"], a["n"], a["T"], a["x"], a["form"], a["g"], a["window_of"], a["windows"],
                           device=a.get("device", 0))[0]

    def refused(key, **kw):
        _refusal_is_the_recorded_one(key, call(**kw), L.nmrfit_last_error())
    assert call() in (_cabi.OK, _cabi.E_NO_DEVICE)
    assert call(device=1 << 20) == _cabi.E_NO_DEVICE
    # form 2 at a length that is no power of two
    refused("form 2 at n = 12", form=[1, 2, 2], g=[5.0, 1.5, 3.3])
    # the lengths
    refused("n = 2^21 + 1", n=[57, (1 << 21) + 1, 8])
    refused("n = 1", n_in=[64, 1, 5], n=[57, 1, 8], x=np.zeros(2 * (2 * 64 + 1 + 5)))
    refused("n = 2^23", n=[57, 1 << 23, 8])
    assert call(n=[57, (1 << 21) - 1, 8]) in (_cabi.OK, _cabi.E_NO_DEVICE)
    # those of nmrfit_fid_condition_transform still hold
    refused("n < n_in'", n=[56, 12, 8])                                               # n < n_in' = 57
    refused("T = 0", T=[2, 0, 1])
    refused("form = 3", form=[1, 3, 2])
    # the budget: T n + 2 T M + 2 M, M = 2^22 at n = 2^21 - 1
    one = dict(n_in=[1], x=np.zeros(2), form=[0], g=[0.0], window_of=[-1], windows=[])
    refused("6 traces of 2^21 - 1", n=[(1 << 21) - 1], T=[6], **one)                   # 6 (n + 2 M) + 2 M > 2^26 = 16 M
    # (5 (n + 2 M) + 2 M < 2^26 is taken: tests/test_gpu_fid_any.py's probe sizes are run once, outside the suite)
    refused("2^26 values and a chirp job", n_in=[1, 1], n=[4099, 1 << 22], T=[1, 16], x=np.zeros(4), form=[0, 0], g=[0.0, 0.0],
            window_of=[-1, -1], windows=[])                                            # 2^26 of the second alone: the first's on top
    # a call that is wrong in two ways: the first refusal of the header's order wins
    refused("form = 3 and n = 2^21 + 1", form=[1, 3, 2], n=[57, (1 << 21) + 1, 8])
    # the old entry point refuses what it refused, in its own words
    rc = fa.raw_call(L, [10], [12], [1], np.zeros(20), [0], [0.0], [-1], [], entry="nmrfit_fid_condition_transform")[0]
    _refusal_is_the_recorded_one("n = 12 at the old entry point", rc, L.nmrfit_last_error())


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_the_chirp_values_are_within_the_stated_bound(tmp_path):
    """csrc/fid_chirp.h compiled for the host (tests/fid/chirp_check.hip): the table against a truth of 113 bits for N in
    {3, 7, 12, 1000, 4027, 4099, 65466, 2^21 - 1}: every index up to 2^13, a stride plus 10^6 random indices beyond.  The
    header's mu = u holds -- and does not with the angle formed in floating point.  fid.chirp is the same table."""
    exe = str(tmp_path / "chirp_check")
    cc = subprocess.run([HIPCC, "--offload-arch=gfx950", "--cuda-host-only", "-O2", "-std=c++17", "-ffp-contract=on",
                         "-I" + os.path.join(ROOT, "nmrfit_amd", "csrc"), os.path.join(ROOT, "tests", "fid", "chirp_check.hip"),
                         "-o", exe], capture_output=True, text=True, timeout=300)
    assert cc.returncode == 0, cc.stderr[-3000:]

    def table(*args):
        run = subprocess.run([exe] + list(args), capture_output=True, text=True, timeout=300)
        assert run.returncode == 0, (run.returncode, run.stderr)
        return {int(n): float(w) for n, w in (ln.split() for ln in run.stdout.splitlines())}
    got = table()
    assert set(got) == {3, 7, 12, 1000, 4027, 4099, 65466, (1 << 21) - 1}
    worst = max(got.values())
    print("chirp values: worst |c^ - c| = %.4f u (mu = 1 u); per N: %s" % (worst, got))
    assert all(w <= fs.MU_DEVICE / fs.U for w in got.values()) and worst > 0.0
    naive = table("naive")
    print("angle formed in fp64: %.3g u at N = 2^21 - 1" % naive[(1 << 21) - 1])
    assert naive[(1 << 21) - 1] > fs.MU_DEVICE / fs.U and naive[65466] > fs.MU_DEVICE / fs.U
    # the exact values of the numpy restatement
    c = fid.chirp(12)
    h = np.sqrt(0.5)
    assert c[0] == 1.0 and c[6] == -1.0 and c[3] == complex(-h, -h) and c.dtype == np.complex128
    assert float(np.abs(np.abs(fid.chirp(4099, np.clongdouble)) - 1).max()) < 2.0 ** -62


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_kernel_resources():
    """tools/kernel_resources.py --check --unit fid_any.hip: four kernels with the prefix fida_ (the partial maxima of its
    spectra are fid.hip's fid_max_part_kernel's), none with scratch memory, spills or LDS."""
    run = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"), "--check", "--unit", "fid_any.hip"],
                         capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, run.stdout[-3000:] + run.stderr[-3000:]
    lines = [ln.split() for ln in run.stdout.splitlines()[1:] if ln.strip()]
    assert sorted(ln[0] for ln in lines) == ["fida_filter_kernel", "fida_load_kernel", "fida_product_kernel", "fida_store_kernel"], run.stdout
    for ln in lines:      # kernel VGPR AGPR scratch waves LDS s-spill
        assert int(ln[3]) == 0 and int(ln[6]) == 0 and int(ln[5]) == 0, ln
    print(run.stdout)
    src = open(os.path.join(ROOT, "nmrfit_amd", "csrc", "fid_any.hip")).read()
    assert "atomic" not in src.replace("No LDS, no atomics", "") and "fid_any" in open(os.path.join(ROOT, "nmrfit_amd", "csrc", "build.sh")).read()

"""
The truths and bars of tests/test_gpu_fid_lengths.py, checked without a GPU (tests/fid_lengths_support.py).

  * impulse_truth agrees with np.fft.fft on np.clongdouble within 0.05 u |a| at powers of two and other lengths;
  * the references alone stay inside every bar the device is held to: np.fft.fft in fp64 on impulses inside impulse_bar
    at every two-pass length, fid.bluestein_host in fp64 on the sparse traces inside sparse_bar (mu = fs.MU_NUMPY);
  * the factorisation table of csrc/fid.hip's fid_plan restated, and the device test's lengths against it: every (C, R)
    pair of lg 13 .. 22, every parity of lg 1 .. 12;
  * a numpy restatement of csrc/fid.hip's stages and of its two passes -- the same table indices, every product and sum
    rounded once -- stays inside impulse_bar at every point: the count of products m is not short.  The same
    restatement with `ts` or `up` off by one, or with (2 k) << ts for w3, leaves both bars by many orders; with split
    twiddles turned by 64 u it leaves impulse_bar while the dense bar, at a single point as well, does not notice.
"""
import numpy as np
import pytest

from nmrfit_amd import fid
from tests import fid_any_support as fa
from tests import fid_lengths_support as fl
from tests import fid_support as fs

needs_truth = pytest.mark.skipif(not fs.truth_is_long_double(), reason="numpy's long-double transform is not available")
A = fl.AMPLITUDE


@needs_truth
@pytest.mark.parametrize("n", [8, 4096, 1 << 13, 1 << 16, 1 << 19, 12, 4099, 65467])
def test_the_impulse_truth_is_the_long_double_transform(n):
    worst = 0.0
    for p in (0, 1, n - 1, n // 2 - 1):
        x = np.zeros(n, dtype=np.clongdouble)
        x[p] = A
        d = float(np.abs(fl.impulse_truth(n, p, A) - fs.truth(x)[0]).max()) / abs(A) / fs.U
        worst = max(worst, d)
        assert d <= 0.05, (n, p, d)
    print("n = %d: impulse_truth against np.fft on clongdouble: %.3g u |a|" % (n, worst))


def test_the_bars_have_the_stated_sizes():
    assert fl.impulse_bar(1) == 0.0 and fl.products(12) == 6 and fl.products(13) == 7 and fl.products(22) == 11
    assert 22.5 < fl.impulse_bar(12) / fs.U < 23.5 and 41.5 < fl.impulse_bar(22) / fs.U < 42.5
    # the sparse bar is the header's bar at n_in' = s, and below the dense one
    x = np.zeros((1, 5000), dtype=np.complex128)
    x[0, [3, 77]] = 1.0 + 2.0j, -0.5j
    assert fl.sparse_bar(x, 5000)[0] == fa.bar(np.array([[1.0 + 2.0j, -0.5j]]), 5000)[0] < fa.bar(x, 5000)[0]


@needs_truth
@pytest.mark.parametrize("lg", range(13, 23))
def test_numpys_fp64_transform_of_an_impulse_is_inside_the_impulse_bar(lg):
    n = 1 << lg
    worst = 0.0
    for p in (1, 1 << fl.factorisation(lg)[1], n - 1):
        x = np.zeros(n, dtype=np.complex128)
        x[p] = A
        Y = np.fft.fftshift(np.fft.fft(x))
        worst = max(worst, float(np.abs(Y.astype(np.clongdouble) - fl.impulse_truth(n, p, A)).max()) / abs(A))
    print("lg = %d: np.fft fp64 on impulses %.3g u |a|, impulse_bar %.3g u" % (lg, worst / fs.U, fl.impulse_bar(lg) / fs.U))
    assert worst <= fl.impulse_bar(lg)


@needs_truth
@pytest.mark.parametrize("N", [2049, 4099, 16383, 65466, 65467, 131071, (1 << 19) - 1])
def test_the_fp64_chirp_z_restatement_of_sparse_traces_is_inside_the_sparse_bar(N):
    x, support = fl.sparse_traces(N)
    Y = fid.bluestein_host(x, N)
    bar = fl.sparse_bar(x, N, mu=fs.MU_NUMPY)
    for t, (points, values) in enumerate(support):
        d = np.abs(Y[t].astype(np.clongdouble) - fl.sparse_truth(N, points, values))
        e2 = float(np.sqrt((d ** 2).sum()))
        print("N = %d, %d point(s): error / bar %.3g" % (N, len(points), e2 / bar[t]))
        assert e2 <= bar[t], (N, t)


def test_the_device_tests_lengths_reach_every_factorisation():
    table = {13: (6, 7, 64, 32), 14: (7, 7, 32, 32), 15: (7, 8, 32, 16), 16: (8, 8, 16, 16), 17: (8, 9, 16, 8),
             18: (9, 9, 8, 8), 19: (9, 10, 8, 4), 20: (10, 10, 4, 4), 21: (10, 11, 4, 2), 22: (11, 11, 2, 2)}
    for lg, row in table.items():
        lg1 = lg // 2
        assert fl.factorisation(lg) == row == (lg1, lg - lg1, 1 << (12 - lg1), 1 << (12 - (lg - lg1)))
        assert row[0] + row[1] == lg and max(row[:2]) <= 11 and min(row[2:]) >= 2
    dense = {int(n).bit_length() - 1 for n in fs.LENGTHS} | set(fl.FACTOR_LGS)
    for lgs in (dense, set(fl.IMPULSE_LGS)):
        assert {lg for lg in lgs if lg > 12} == set(table)
        assert {lg & 1 for lg in lgs if lg <= 12} == {0, 1} and {1, 12} <= lgs
    assert len({table[lg][2:] for lg in table}) == 10
    # the chirp-z lengths reach every M above the existing tests' 2^14, and the Bruker lengths sit at 2^17
    assert sorted({fid.conv_length(N) for N in fl.CHIRP_LENGTHS}) == [1 << m for m in range(15, 23)]
    assert fid.conv_length(65466) == fid.conv_length(65467) == 1 << 17 and max(fl.CHIRP_LENGTHS) == fid.ANY_MAX
    for lg in fl.IMPULSE_LGS:
        ps = fl.impulse_positions(lg)
        assert len(set(ps)) == len(ps) and all(0 <= p < 1 << lg for p in ps) and len(ps) << lg <= fid.MAX_VALUES


# ---- csrc/fid.hip's stages restated ------------------------------------------------------------------------------------

def _times(a, w):
    out = np.empty_like(a)
    out.real = a.real * w.real - a.imag * w.imag
    out.imag = a.real * w.imag + a.imag * w.real
    return out


def _stage(x, tw, lgC, lgNs, R, ts_off, w3):
    """lds_stage<R> on the last axis of x: butterfly b reads b + r nb and writes out + r step."""
    lgR = 2 if R == 4 else 1
    nb = x.shape[-1] >> lgR
    b = np.arange(nb)
    j, c = b >> lgC, b & ((1 << lgC) - 1)
    k = j & ((1 << lgNs) - 1)
    out, step = ((((j - k) << lgR) + k) << lgC) + c, 1 << (lgNs + lgC)
    xs = [x[..., b + r * nb] for r in range(R)]
    y = np.empty_like(x)
    if R == 2:
        y[..., out], y[..., out + step] = xs[0] + xs[1], xs[0] - xs[1]
        return y
    ts = fs.LDS_LOG2 - 2 - lgNs + ts_off
    z1, z2, z3 = (_times(xs[r], tw[((f * k) << ts) % len(tw)]) for r, f in ((1, 1), (2, 2), (3, w3)))
    s02, d02, s13, d13 = xs[0] + z2, xs[0] - z2, z1 + z3, z1 - z3
    mi = d13.imag - 1j * d13.real
    y[..., out], y[..., out + step], y[..., out + 2 * step], y[..., out + 3 * step] = s02 + s13, d02 + mi, s02 - s13, d02 - mi
    return y


def _block(x, tw, lgC, lgL, ts_off, w3):
    """lds_fft: 2^lgC interleaved transforms of 2^lgL points."""
    lgNs = 0
    if lgL & 1:
        x, lgNs = _stage(x, tw, lgC, 0, 2, ts_off, w3), 1
    for lgNs in range(lgNs, lgL, 2):
        x = _stage(x, tw, lgC, lgNs, 4, ts_off, w3)
    return x


def restated_transform(x, lg, ts_off=0, up_off=0, w3=3, split_turn=0.0):
    """Y of x (T, 2^lg) by the kernels' own steps.  A workgroup's interleaved columns (rows) are independent, so each pass
    is made on all of them at once: C = n2 in pass 1, R = n1 in pass 2.  The knobs break it: `ts_off`, `up_off` shift
    the table index of a stage and of the split twiddle, `w3` is the factor of k in the third twiddle's index,
    `split_turn` turns every split twiddle by that angle."""
    tw = fl.unit_root(np.arange(1 << fs.LDS_LOG2), 1 << fs.LDS_LOG2).astype(np.complex128)
    n = 1 << lg
    if lg <= fs.LDS_LOG2:
        return np.fft.fftshift(_block(x, tw, 0, lg, ts_off, w3), axes=-1)
    lg1, lg2 = fl.factorisation(lg)[:2]
    work = _block(x, tw, lg2, lg1, ts_off, w3)                        # point q1 of column j2 at q1 n2 + j2
    q1, j2 = np.divmod(np.arange(n, dtype=np.int64), 1 << lg2)
    split = fl.unit_root(((j2 * q1) << (fid.MAX_LOG2 - lg + up_off)) % (1 << fid.MAX_LOG2), 1 << fid.MAX_LOG2)
    split = (split * np.exp(np.clongdouble(1j * split_turn))).astype(np.complex128)
    work = _times(work, split)
    rows = work.reshape(-1, 1 << lg1, 1 << lg2).transpose(0, 2, 1).reshape(-1, n)      # point j2 of row q1 at j2 n1 + q1
    return np.fft.fftshift(_block(rows, tw, lg1, lg2, ts_off, w3), axes=-1)             # entry q2 n1 + q1 is X[q1 + n1 q2]


def _ratios(lg, **knobs):
    """(worst point of the impulses / impulse_bar, dense error / fs.bar) of the restatement."""
    n = 1 << lg
    ps = fl.impulse_positions(lg)
    x = np.zeros((len(ps), n), dtype=np.complex128)
    x[np.arange(len(ps)), ps] = A
    want = np.stack([fl.impulse_truth(n, p, A) for p in ps])
    imp = float(np.abs(restated_transform(x, lg, **knobs).astype(np.clongdouble) - want).max()) / (fl.impulse_bar(lg) * abs(A))
    xd = fs.sample_fid(n, 1, seed=3)
    e2, einf = fs.errors(restated_transform(xd, lg, **knobs), fs.truth(xd))
    return imp, max(e2, einf) * fs.U / fs.bar(n, fs.MU_DEVICE)


@needs_truth
@pytest.mark.parametrize("lg", [3, 4, 11, 12, 13, 14, 15, 16, 17])
def test_the_restated_stages_are_inside_both_bars(lg):
    imp, dense = _ratios(lg)
    print("lg = %d: the restatement: impulses %.3g of impulse_bar, dense %.3g of its bar" % (lg, imp, dense))
    assert imp <= 1.0 and dense <= 1.0


@needs_truth
def test_broken_restatements_leave_the_impulse_bar():
    for knobs in (dict(ts_off=1), dict(up_off=1), dict(up_off=-1), dict(w3=2)):
        imp, dense = _ratios(15, **knobs)
        print("lg = 15, %r: impulses %.3g of impulse_bar, dense %.3g of its bar" % (knobs, imp, dense))
        assert imp > 1e6
    # a loss of accuracy the dense bar cannot see: every split twiddle off by 64 u
    imp, dense = _ratios(16, split_turn=64 * fs.U)
    print("lg = 16, split twiddles turned by 64 u: impulses %.3g of impulse_bar, dense %.3g of its bar" % (imp, dense))
    assert imp > 1.0 and dense <= 1.0

"""
The FID transforms on the device at every length class they serve (csrc/fid.hip, csrc/fid_cond.hip, csrc/fid_any.hip).
tests/test_gpu_fid.py stops at 2^14 and adds 2^17, tests/test_gpu_fid_any.py at N = 5000 (M = 2^14); here:

  * every two-pass factorisation they leave out, lg in {15, 16, 18, .. 22}: dense FIDs inside fs.bar against the
    long-double truth, in the 2-norm and at every point; u, v, row equal fid.finish_host(Y) bit for bit; zero filling
    at 2^16 and 2^19 gives the bits of the padded input;
  * impulses a delta_p at every lg of both lists: EVERY point within impulse_bar(lg) |a| of the closed form -- 0 at
    n = 2, 23 u at 2^12, 42 u at 2^22, where the dense bar allows a point sqrt(n) times more; p = 0 alone gives Y == a
    exactly and the maximum's full tie goes to index 0;
  * the chirp-z path at every M it can reach, 2^15 .. 2^22, and at the two lengths of a 64k Bruker FID: dense FIDs
    inside fa.bar, traces of one and four non-zero points inside sparse_bar against the sum of their impulses (no
    transform in that truth);
  * the Bruker path of core.load at s = 65536: 65467 and 65466 points, the conditioned traces the zero-filled call's
    bit for bit;
  * launches of more than 32768 work items (the second grid row of fid_item_grid): 33 000 tiny spectra in one call,
    each the bits of its pool member alone, and one spectrum of 40 000 traces.

The bars are derived (tests/fid_lengths_support.py); the printed ratios are recorded in DESIGN.md 4.15.3, not asserted.
"""
import numpy as np
import pytest

from nmrfit_amd import fid
from tests import fid_any_support as fa
from tests import fid_cond_support as fc
from tests import fid_lengths_support as fl
from tests import fid_support as fs

pytestmark = pytest.mark.gpu

needs_truth = pytest.mark.skipif(not fs.truth_is_long_double(), reason="numpy's long-double transform is not available")
A = fl.AMPLITUDE


def _finish_is_the_hosts(u, v, row, Y):
    mu, mv, mrow = fid.finish_host(Y)
    assert fs.same_values(u, mu) and fs.same_values(v, mv) and fs.same_values(row, mrow), (row, mrow)


def _held(Y, want, limit, what):
    """The 2-norm of every trace's error and its worst point against the absolute bar: the worst ratio."""
    d = np.abs(np.asarray(Y).astype(np.clongdouble) - want)
    e2 = np.sqrt((d ** 2).sum(axis=-1)).astype(np.float64)
    worst = d.max(axis=-1).astype(np.float64)
    print("%s: error / bar %.3g (2-norm), %.3g (worst point)" % (what, float((e2 / limit).max()), float((worst / limit).max())))
    assert np.all(e2 <= limit) and np.all(worst <= limit), what
    return float((e2 / limit).max())


# ---- C1: every factorisation, dense input ------------------------------------------------------------------------------

@needs_truth
@pytest.mark.parametrize("lg", fl.FACTOR_LGS)
def test_each_factorisation_is_inside_the_bar(lg):
    n = 1 << lg
    x = fs.sample_fid(n, T=1 if lg >= 20 else 2, seed=3)
    u, v, row, Y = fid.transform_many([x], return_transform=True)[0]
    assert Y.shape == x.shape and row[0] == 0 and row[4] == n and row[5] == len(x)
    e2, einf = fs.errors(Y, fs.truth(x))
    limit = fs.bar(n, fs.MU_DEVICE) / fs.U
    print("lg = %d (lg1, lg2, C, R = %r): 2-norm error %.3g u, worst point %.3g u, bar %.4g u, ratio %.3g"
          % ((lg, fl.factorisation(lg), e2, einf, limit, max(e2, einf) / limit)))
    assert e2 <= limit and einf <= limit, (lg, e2, einf, limit)
    _finish_is_the_hosts(u, v, row, Y)


@pytest.mark.parametrize("lg", [16, 19])
def test_zero_filling_is_the_padded_input(lg):
    n = 1 << lg
    x = fs.sample_fid(n, T=2, seed=5)
    for n_in in (n // 2 + 1, n - 1):
        full = np.zeros((2, n), dtype=np.complex128)
        full[:, :n_in] = x[:, :n_in]
        want = fid.transform_many([full], return_transform=True)[0]
        got = fid.transform_many([x[:, :n_in].copy()], zero_fill=n, return_transform=True)[0]
        assert fs.same_result(got, want), (lg, n_in)


# ---- C2: impulses, pointwise -------------------------------------------------------------------------------------------

@needs_truth
@pytest.mark.parametrize("lg", fl.IMPULSE_LGS)
def test_an_impulse_is_inside_the_impulse_bar_at_every_point(lg):
    n = 1 << lg
    ps = fl.impulse_positions(lg)
    x = np.zeros((len(ps), n), dtype=np.complex128)
    x[np.arange(len(ps)), ps] = A
    u, v, row, Y = fid.transform_many([x], return_transform=True)[0]
    assert Y.shape == x.shape and row[0] == 0
    limit = fl.impulse_bar(lg) * abs(A)
    worst = 0.0
    for t, p in enumerate(ps):
        err = float(np.abs(Y[t].astype(np.clongdouble) - fl.impulse_truth(n, p, A)).max())
        worst = max(worst, err)
        assert err <= limit, (lg, p, err / abs(A) / fs.U, limit / abs(A) / fs.U)
    print("lg = %d: impulses at %r: worst point %.3g u |a|, impulse_bar %.3g u, ratio %.3g"
          % (lg, ps, worst / abs(A) / fs.U, limit / abs(A) / fs.U, worst / limit if limit else 0.0))
    _finish_is_the_hosts(u, v, row, Y)


@pytest.mark.parametrize("lg", fl.IMPULSE_LGS)
def test_an_impulse_at_zero_is_a_constant_exactly_and_the_tie_goes_to_index_zero(lg):
    n = 1 << lg
    x = np.zeros((1, n), dtype=np.complex128)
    x[0, 0] = A
    u, v, row, Y = fid.transform_many([x], return_transform=True)[0]
    assert fs.same_bits(Y, np.full((1, n), A))            # (every twiddle met is 1, every sum has a zero operand)
    assert tuple(row) == (0.0, A.real, A.imag, 0.0, float(n), 1.0)
    _finish_is_the_hosts(u, v, row, Y)


# ---- C3: chirp-z at every M it can reach -------------------------------------------------------------------------------

def _chirp_traces(N):
    """T of the dense job: 1 from M = 2^20 up, 3 at 65467 (a chunk of fid_max_part_kernel's 8192 values straddles two
    traces at every boundary: 65467 is odd), else 2."""
    return 1 if fid.conv_length(N) >= 1 << 20 else (3 if N == 65467 else 2)


@needs_truth
@pytest.mark.parametrize("N", fl.CHIRP_LENGTHS)
def test_each_chirp_length_is_inside_the_bar(N):
    x = fs.sample_fid(N, _chirp_traces(N), seed=90)
    u, v, row, Y = fid.transform_many([x], any_length=True, return_transform=True)[0]
    assert Y.shape == x.shape and u.shape == v.shape == (N,) and row[0] == 0 and row[4] == N and row[5] == len(x)
    _held(Y, fa.truth(x, N), fa.bar(x, N), "N = %d, M = 2^%d, T = %d, dense" % (N, fid.conv_length(N).bit_length() - 1, len(x)))
    _finish_is_the_hosts(u, v, row, Y)


@needs_truth
@pytest.mark.parametrize("N", fl.CHIRP_LENGTHS)
def test_sparse_traces_at_each_chirp_length_are_inside_the_sparse_bar(N):
    x, support = fl.sparse_traces(N)
    # (one job of three traces; from M = 2^20 up a job per trace)
    jobs = [x[t:t + 1] for t in range(3)] if fid.conv_length(N) >= 1 << 20 else [x]
    got = fid.transform_many(jobs, any_length=True, return_transform=True)
    Y = np.concatenate([g[3] for g in got])
    assert Y.shape == x.shape and all(g[2][0] == 0 and g[2][4] == N for g in got)
    want = np.stack([fl.sparse_truth(N, points, values) for points, values in support])
    d = np.abs(Y.astype(np.clongdouble) - want)
    e2 = np.sqrt((d ** 2).sum(axis=-1)).astype(np.float64)
    bar = fl.sparse_bar(x, N)
    print("N = %d, M = 2^%d, sparse (1, 1, 4 points): error / bar %s" % (N, fid.conv_length(N).bit_length() - 1, np.round(e2 / bar, 5)))
    assert np.all(e2 <= bar), (N, e2 / bar)
    for u, v, row, Yk in got:
        _finish_is_the_hosts(u, v, row, Yk)


# ---- C4: the Bruker path at its real size ------------------------------------------------------------------------------

@needs_truth
@pytest.mark.parametrize("g", [67.98416137695312, 68.0])
def test_the_bruker_path_at_64k_comes_out_at_its_own_length(g):
    s = 1 << 16
    N = s - fc.skip_add(g)[0]
    assert N == (65467 if g < 68.0 else 65466)
    x = fs.sample_fid(s, 1, seed=93)
    for window in (None, fid.window_em(N, 3.0, 65536.0, first_point=0.5)):
        u, v, row, Y, xc = fid.transform_many([x], grpdly=g, window=window, truncate_grpdly=False, any_length=True, return_transform=True,
                                              return_conditioned=True)[0]
        old = fid.transform_many([x], grpdly=g, window=window, truncate_grpdly=False, zero_fill=s, return_conditioned=True)[0]
        assert Y.shape == (1, N) and xc.shape == (1, N) and row[0] == 0 and row[4] == N
        assert fs.same_bits(xc.view(np.float64), old[3].view(np.float64))
        xc_t, Y_t = fc.truth(x, g, "fid", window, None)
        bar_c, _ = fc.bars(x, fid.FORM_FID, g, window, N)
        assert Y_t.shape == Y.shape
        _held(Y, Y_t, fa.bar(xc_t, N, conditioned_bar=bar_c), "Bruker s = 65536, g = %r%s" % (g, ", window" if window is not None else ""))
        _finish_is_the_hosts(u, v, row, Y)


# ---- C5: more than 32768 work items ------------------------------------------------------------------------------------

def test_a_call_of_33000_spectra_gives_each_its_own_bits():
    pool = fl.tiny_pool()
    alone = [fid.transform_many([x], return_transform=True)[0] for x in pool]
    assert sorted({int(a[2][0]) for a in alone}) == [0, 1, 2] and [int(a[2][0]) for a in alone[-2:]] == [1, 2]
    K = 33000
    got = fid.transform_many([pool[k % len(pool)] for k in range(K)], return_transform=True)
    assert len(got) == K
    for m, a in enumerate(alone):                  # (spectra 32767, 32768 and the last are members 15, 0 and 7)
        assert fl.stacked_same(got[m::len(pool)], a), m
    for k in (0, 32767, 32768, K - 1):
        assert fs.same_result(got[k], alone[k % len(pool)]), k


@needs_truth
def test_a_spectrum_of_40000_traces():
    T, n = 40000, 4
    x = fs.sample_fid(n, T, seed=7)
    u, v, row, Y = fid.transform_many([x], return_transform=True)[0]
    assert Y.shape == (T, n) and row[0] == 0 and row[5] == T
    e2, einf = fs.errors(Y, fs.truth(x))
    limit = fs.bar(n, fs.MU_DEVICE) / fs.U
    print("T = %d, n = %d: worst trace: 2-norm error %.3g u, worst point %.3g u, bar %.4g u" % (T, n, e2, einf, limit))
    assert e2 <= limit and einf <= limit
    _finish_is_the_hosts(u, v, row, Y)

"""
The any-length FID transform on the device (csrc/fid_any.hip, include/nmrfit_amd_fid_any.h): a chirp-z transform for
the lengths that are not powers of two, in the library call that conditions and transforms.

  * every length of fa.LENGTHS -- 2047 is the last whose M = 4096 is one LDS-resident transform, 2049 the first with the
    two-pass M = 8192, 4099 a prime -- with T in {1, 3} and zero fill from n_in' < N, against the truth
    (fid.bluestein_host in long double) within the header's first-order bar (tests/fid_any_support.py), in the 2-norm and
    at every point; u, v and the row equal fid.finish_host of the returned Y bit for bit;
  * the Bruker case of core.load: s = 4096, g = 67.98416137695312 and 68.0, form 1, with and without an exponential
    window, no zero_fill: 4027 points (4026 at 68.0), the conditioned traces bit-identical to the zero-filled call's, Y inside the bar
    with the conditioned trace's own bar carried by beta;
  * a spectrum gives the same bits alone, in a mixed batch, in the batch reversed and from a second call, and the
    power-of-two jobs of the batch are nmrfit_fid_condition_transform's bit for bit;
  * three child processes -- NMRFIT_POISON_ALLOC unset, 255, 63 -- give byte-identical outputs over the mixed batch;
  * an all-zero FID gives row status 1, a NaN input status 2 with u, v NaN, at N = 12.
  * ties across the chunks of the partial maxima (fid_max_part_kernel serves the finish-only jobs by a remainder and the
    others by a mask, in one launch): equal traces on both sides of a chunk boundary and across it, the first one wins.

Measured on the MI355X (the worst ratio error / bar): see DESIGN.md 4.15.2.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import nmrfit_amd
from nmrfit_amd import fid
from tests import fid_any_support as fa
from tests import fid_cond_support as fc
from tests import fid_support as fs

pytestmark = pytest.mark.gpu

needs_truth = pytest.mark.skipif(not fs.truth_is_long_double(), reason="numpy's long-double transform is not available")


def _held(Y, want, limit, what):
    """The 2-norm of every trace's error and its worst point against the bar; returns the worst ratio."""
    d = np.abs(np.asarray(Y).astype(np.clongdouble) - want)
    e2 = np.sqrt((d ** 2).sum(axis=-1)).astype(np.float64)
    worst = d.max(axis=-1).astype(np.float64)
    ratio = float((e2 / limit).max())
    print("%s: error / bar %.3g (2-norm), %.3g (worst point); error %.3g u of ||Y||_2"
          % (what, ratio, float((worst / limit).max()), float((e2 / np.sqrt((np.abs(want) ** 2).sum(axis=-1)).astype(np.float64)).max() / fs.U)))
    assert np.all(e2 <= limit) and np.all(worst <= limit), what
    return ratio


def _finish_is_the_hosts(u, v, row, Y):
    mu, mv, mrow = fid.finish_host(Y)
    assert fs.same_values(u, mu) and fs.same_values(v, mv) and fs.same_values(row, mrow)


@needs_truth
@pytest.mark.parametrize("N", fa.LENGTHS)
def test_each_length_is_inside_the_bar(N):
    short = max(1, N - max(1, N // 3))
    jobs = [fs.sample_fid(N, 1, seed=90), fs.sample_fid(short, 3, seed=91), fs.sample_fid(1, 1, seed=92)]
    got = fid.transform_many(jobs, zero_fill=N, any_length=True, return_transform=True)
    bare = fid.transform_many(jobs, zero_fill=N, any_length=True)
    for k, (x, (u, v, row, Y), b) in enumerate(zip(jobs, got, bare)):
        assert Y.shape == (len(x), N) and u.shape == v.shape == (N,) and row[0] == 0 and row[4] == N and row[5] == len(x)
        _held(Y, fa.truth(x, N), fa.bar(x, N), "N = %d, T = %d, n_in' = %d" % (N, len(x), x.shape[1]))
        _finish_is_the_hosts(u, v, row, Y)
        assert fs.same_result(b, (u, v, row)), k
        # the reference's own lines with numpy's transform of the same length land on the same grid
        hu, hv = fid.transform_host(x, zero_fill=N)
        assert np.abs(u - hu).max() <= 1e-10 and np.abs(v - hv).max() <= 1e-10


@needs_truth
@pytest.mark.parametrize("g", [67.98416137695312, 68.0])
def test_the_bruker_path_of_core_load_comes_out_at_its_own_length(g):
    s = 4096
    skip = fc.skip_add(g)[0]
    N = s - skip
    assert N == (4027 if g < 68.0 else 4026)          # (floor(g + 2) = 69 for the unrounded value, 70 for 68.0: odd and even)
    W = fid.window_em(N, 3.0, 4096.0, first_point=0.5)
    xs = [fs.sample_fid(s, 1, seed=93), fs.sample_fid(s, 3, seed=94)]
    for window in (None, W):
        got = fid.transform_many(xs, grpdly=g, window=window, truncate_grpdly=False, any_length=True, return_transform=True,
                                 return_conditioned=True)
        old = fid.transform_many(xs, grpdly=g, window=window, truncate_grpdly=False, zero_fill=4096, return_conditioned=True)
        for x, (u, v, row, Y, xc), o in zip(xs, got, old):
            assert Y.shape == (len(x), N) and xc.shape == (len(x), N) and row[0] == 0 and row[4] == N
            assert fs.same_bits(xc.view(np.float64), o[3].view(np.float64))
            xc_t, Y_t = fc.truth(x, g, "fid", window, None)
            bar_c, _ = fc.bars(x, fid.FORM_FID, g, window, N)
            assert Y_t.shape == Y.shape
            _held(Y, Y_t, fa.bar(xc_t, N, conditioned_bar=bar_c), "Bruker g = %r, T = %d%s" % (g, len(x), ", window" if window is not None else ""))
            _finish_is_the_hosts(u, v, row, Y)
    datas = nmrfit_amd.spectra_from_fids(xs, 4096.0, 100.0, 0.0, grpdly=g, truncate_grpdly=False, any_length=True)
    assert all(len(d.w) == len(d.u) == len(d.v) == N for d in datas)
    assert fs.same_bits(datas[0].w, fid.ppm_axis(N, 4096.0, 100.0, 0.0))


@pytest.fixture(scope="module")
def mixed():
    jobs = fa.mixed_jobs()
    alone = [fa.run_jobs([j])[0] for j in jobs]
    return jobs, alone


def test_a_spectrum_is_the_same_alone_in_the_batch_reversed_and_again(mixed):
    jobs, alone = mixed
    lengths = [a[3].shape[1] for a in alone]
    assert lengths.count(1000) == 2 and {4027, 2047, 5000, 7, 300, 512, 8192, 1024} <= set(lengths)
    batch = fa.run_jobs(jobs)
    back = fa.run_jobs(jobs[::-1])[::-1]
    again = fa.run_jobs(jobs)
    for k, (b, r, g, a) in enumerate(zip(batch, back, again, alone)):
        assert fs.same_result(b, a) and fs.same_result(r, a) and fs.same_result(g, a), k
        _finish_is_the_hosts(b[0], b[1], b[2], b[3])
    # the power-of-two jobs are nmrfit_fid_condition_transform's, bit for bit
    pow2 = [k for k, n in enumerate(lengths) if not n & (n - 1)]
    assert len(pow2) == 3
    for k in pow2:
        x, g, mode, W, zf = jobs[k]
        old = fid.transform_many([x], zero_fill=zf, grpdly=g, grpdly_mode=mode, window=W, truncate_grpdly=False, return_transform=True,
                                 return_conditioned=True)[0]
        assert fs.same_result(batch[k], old), k
        same = fa.run_lengths([jobs[k]], [lengths[k]], entry="nmrfit_fid_condition_transform")[0]
        assert fs.same_result(batch[k], same), k


def test_results_do_not_depend_on_fresh_device_memory(tmp_path):
    files = {}
    for tag, poison in (("unset", None), ("255", "255"), ("63", "63")):
        out = str(tmp_path / ("fid_any_%s.npz" % tag))
        env = dict(os.environ)
        env.pop("NMRFIT_POISON_ALLOC", None)
        if poison is not None:
            env["NMRFIT_POISON_ALLOC"] = poison
        try:
            run = subprocess.run([sys.executable, "-m", "tests.fid_any_support", "poison", out], cwd=fs.ROOT, env=env,
                                 capture_output=True, text=True, timeout=60)
        except subprocess.TimeoutExpired as e:      # (no further child)
            pytest.fail("pattern %s: no exit within 60 s\n%s" % (tag, (e.stderr or b"")[-3000:]))
        # (a signal shows as a negative code: the same stop, and no further child)
        assert run.returncode == 0, "pattern %s: exit %d\n%s\n%s" % (tag, run.returncode, run.stdout[-1500:], run.stderr[-3000:])
        with np.load(out, allow_pickle=False) as z:
            files[tag] = {k: z[k] for k in z.files}
    base = files["unset"]
    assert len(base) == 5 * len(fa.mixed_jobs()) + 1
    for tag, poison in (("255", "255"), ("63", "63")):
        got = files[tag]
        assert str(got["__poison__"]) == poison and str(base["__poison__"]) == ""      # (the child did see the knob)
        assert set(got) == set(base)
        differ = [k for k in base if not k.startswith("__")
                  and (base[k].dtype != got[k].dtype or base[k].shape != got[k].shape or base[k].tobytes() != got[k].tobytes())]
        assert not differ, "pattern %s: arrays differ from the unpoisoned run's: %s" % (tag, differ)


def test_statuses_at_twelve_points():
    zero = np.zeros((2, 10), dtype=np.complex128)
    bad = fs.sample_fid(12, 2, seed=95)
    bad[1, 5] = np.nan
    good = fs.sample_fid(12, 1, seed=96)
    got = fid.transform_many([zero, bad, good], zero_fill=12, any_length=True, return_transform=True)
    assert [int(g[2][0]) for g in got] == [fid.ZERO, fid.NOT_FINITE, fid.OK]
    for u, v, row, Y in got[:2]:
        assert u.shape == v.shape == (12,) and np.isnan(u).all() and np.isnan(v).all() and row[4] == 12
        _finish_is_the_hosts(u, v, row, Y)
    assert fs.same_result(got[2], fid.transform_many([good], any_length=True, return_transform=True)[0])
    with pytest.raises(ValueError, match="FID 0 is all zero"):
        nmrfit_amd.spectra_from_fids([zero], 1.0, 1.0, 0.0, zero_fill=12, any_length=True)


def test_ties_across_the_chunks_of_the_partial_maxima():
    """fa.TIES: N = 12 (a finish-only job) and n = 8 in one call, each a stack of two sample traces lo and hi = 3 lo.  The
    copies of hi transform to the same bits (asserted on the returned Y), so the maximum ties between them: the row is
    the mirror's on that Y bit for bit, its index lies in the first copy -- before the chunk boundary, in the trace that
    straddles it, behind it -- and a FID alone gives what it gives in the pair."""
    los = [fs.sample_fid(n, 1, seed=97) for _, n, _, _ in fa.TIES]
    for case in range(3):
        xs = [fa.tie_stack(lo, T, placements[case]) for lo, (_, _, T, placements) in zip(los, fa.TIES)]
        pair = fid.transform_many(xs, any_length=True, return_transform=True)
        for x, (name, n, T, placements), (u, v, row, Y) in zip(xs, fa.TIES, pair):
            hi_at = placements[case]
            assert Y.shape == (T, n) and row[0] == 0 and row[4] == n and row[5] == T
            assert all(fs.same_bits(Y[t], Y[hi_at[0]]) for t in hi_at), (name, hi_at)
            lo_at = [t for t in range(T) if t not in hi_at]
            assert all(fs.same_bits(Y[t], Y[lo_at[0]]) for t in (lo_at[1], 8192 // n - 1, lo_at[-1])) and not fs.same_bits(Y[0], Y[hi_at[0]])
            _finish_is_the_hosts(u, v, row, Y)
            assert int(row[3]) // n == hi_at[0], (name, hi_at, row)
            alone = fid.transform_many([x], any_length=True, return_transform=True)[0]
            assert fs.same_result(alone, (u, v, row, Y)), (name, hi_at)

"""
The FID transform on the device (csrc/fid.hip, include/nmrfit_amd_fid.h).

  * the centred transform Y of every trace is inside the first-order bound of a radix-2-equivalent fp64 FFT against the
    long-double truth (tests/fid_support.py: the bar, with the header's mu), in the 2-norm and at every single point, at
    lengths below a wave, at wave and workgroup edges, on both sides of the LDS-resident / two-pass switch, at a two-pass
    length of either parity and at the workload's own 2^17;
  * zero filling on the device gives the bits of the explicitly padded input;
  * u, v and the rows equal fid.finish_host(Y) of the device's own Y bit for bit -- which ties them to the truth through
    Y exactly -- for T in {1, 2, 5}, both branches of Smith's rule, a tie, an all-zero FID and one that is not finite;
  * a spectrum gives the same bits alone, in any ragged batch and from call to call;
  * three child processes -- NMRFIT_POISON_ALLOC unset, 255, 63 -- give byte-identical outputs;
  * spectra_from_fids hands shift_phase_many / select_peaks_many spectra whose peaks sit where the FID's lines are.

Measured on the MI355X (the worst ratio error / bar over the lengths): see DESIGN.md 4.15.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import nmrfit_amd
from nmrfit_amd import fid, synth
from tests import fid_support as fs

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pool():
    """The ragged jobs of the batch tests and each one's result alone (a library call per job)."""
    jobs = fs.poison_jobs()
    alone = [fid.transform_many([x], zero_fill="pow2", return_transform=True)[0] for x in jobs]
    return jobs, alone


def test_the_transform_is_inside_the_bar():
    xs = [fs.sample_fid(n, T=1 if n >= 1 << 17 else 2, seed=3) for n in fs.LENGTHS]
    got = fid.transform_many(xs, return_transform=True)
    worst = 0.0
    for n, x, (u, v, row, Y) in zip(fs.LENGTHS, xs, got):
        assert Y.shape == x.shape and row[0] == 0 and row[4] == n and row[5] == len(x)
        e2, einf = fs.errors(Y, fs.truth(x))
        limit = fs.bar(n, fs.MU_DEVICE) / fs.U
        print("n = %d: 2-norm error %.3g u, worst point %.3g u, bar %.4g u, ratio %.3g" % (n, e2, einf, limit, max(e2, einf) / limit))
        worst = max(worst, max(e2, einf) / limit)
        assert e2 <= limit and einf <= limit, (n, e2, einf, limit)
    print("worst ratio error / bar: %.3g" % worst)


def test_zero_filling_is_the_padded_input():
    short, padded = [], []
    for n in (8, 64, 1 << 12, 1 << 13, 1 << 14):
        x = fs.sample_fid(n, T=2, seed=5)
        for n_in in (1, n // 2 + 1, n - 1, n):
            full = np.zeros((2, n), dtype=np.complex128)
            full[:, :n_in] = x[:, :n_in]
            short.append((x[:, :n_in].copy(), n))
            padded.append(full)
    want = fid.transform_many(padded, return_transform=True)
    for (x, n), w in zip(short, want):
        got = fid.transform_many([x], zero_fill=n, return_transform=True)[0]
        assert fs.same_result(got, w), (n, x.shape)
    # "pow2" in one ragged call
    xs = [x for x, _ in short]
    got = fid.transform_many(xs, zero_fill="pow2", return_transform=True)
    for (x, n), g, w in zip(short, got, want):
        if fid.transform_length(x.shape[1], "pow2") == n:
            assert fs.same_result(g, w), (n, x.shape)


def test_the_finishing_stage_is_the_mirror_bit_for_bit():
    jobs, branches = [], set()
    for T in (1, 2, 5):
        for phi in (0.0, 1.8, 3.3):
            jobs.append(synth.make_fid(64, [(0.1, 0.1, 1.0, phi)], T=T, seed=2, noise=0.01).fid)
        jobs.append(fs.sample_fid(1 << 13, T=T, seed=T))            # several partial maxima, several finishing workgroups
    jobs.append(fs.sample_fid(4096, T=5, seed=9))
    jobs.append(np.array([[1 + 1j, 0], [1 + 2j, 0], [1 + 2j, 0]]))  # n = 2 is exact: a tie in the real part, then a full tie
    jobs.append(np.zeros((2, 16), dtype=np.complex128))             # status 1
    bad = fs.sample_fid(128, T=2, seed=7)
    bad[1, 5] = np.inf
    jobs.append(bad)                                                # status 2
    nan = fs.sample_fid(1 << 13, T=1, seed=8)
    nan[0, 77] = np.nan
    jobs.append(nan)
    got = fid.transform_many(jobs, return_transform=True)
    for k, (u, v, row, Y) in enumerate(got):
        mu, mv, mrow = fid.finish_host(Y)
        assert fs.same_values(u, mu) and fs.same_values(v, mv) and fs.same_values(row, mrow), (k, row, mrow)
        if row[0] == 0:
            branches.add("first" if abs(row[1]) >= abs(row[2]) else "second")
    assert branches == {"first", "second"}
    assert [int(g[2][0]) for g in got[-4:]] == [0, 1, 2, 2]
    assert tuple(got[-4][2]) == (0.0, 1.0, 2.0, 2.0, 2.0, 3.0)
    # without the transform output: the same u, v, rows
    plain = fid.transform_many(jobs)
    assert all(fs.same_result(p, g[:3]) for p, g in zip(plain, got))


def test_a_spectrum_is_the_same_alone_in_any_batch_and_from_call_to_call(pool):
    jobs, alone = pool
    rng = np.random.default_rng(17)
    assert {x.shape[1] > 1 << fs.LDS_LOG2 for x in jobs} == {True, False} and len({len(x) for x in jobs}) >= 3
    for trial in range(6):
        K = int(rng.integers(2, 13))
        idx = [int(i) for i in rng.integers(0, len(jobs), K)]
        if trial == 0:
            idx = list(range(len(jobs)))[::-1]
        got = fid.transform_many([jobs[i] for i in idx], zero_fill="pow2", return_transform=True)
        for pos, (i, g) in enumerate(zip(idx, got)):      # (the first and the last job of the batch among them)
            assert fs.same_result(g, alone[i]), (trial, pos, i)
        again = fid.transform_many([jobs[i] for i in idx], zero_fill="pow2", return_transform=True)
        assert all(fs.same_result(a, g) for a, g in zip(again, got))


def test_results_do_not_depend_on_fresh_device_memory(tmp_path):
    files = {}
    for tag, poison in (("unset", None), ("255", "255"), ("63", "63")):
        out = str(tmp_path / ("fid_%s.npz" % tag))
        env = dict(os.environ)
        env.pop("NMRFIT_POISON_ALLOC", None)
        if poison is not None:
            env["NMRFIT_POISON_ALLOC"] = poison
        try:
            run = subprocess.run([sys.executable, "-m", "tests.fid_support", "poison", out], cwd=fs.ROOT, env=env,
                                 capture_output=True, text=True, timeout=60)
        except subprocess.TimeoutExpired as e:      # (no further child)
            pytest.fail("pattern %s: no exit within 60 s\n%s" % (tag, (e.stderr or b"")[-3000:]))
        # (a signal shows as a negative code: the same stop, and no further child)
        assert run.returncode == 0, "pattern %s: exit %d\n%s\n%s" % (tag, run.returncode, run.stdout[-1500:], run.stderr[-3000:])
        with np.load(out, allow_pickle=False) as z:
            files[tag] = {k: z[k] for k in z.files}
    base = files["unset"]
    assert len(base) >= 41
    for tag, poison in (("255", "255"), ("63", "63")):
        got = files[tag]
        assert str(got["__poison__"]) == poison and str(base["__poison__"]) == ""      # (the child did see the knob)
        assert set(got) == set(base)
        differ = [k for k in base if not k.startswith("__")
                  and (base[k].dtype != got[k].dtype or base[k].shape != got[k].shape or base[k].tobytes() != got[k].tobytes())]
        assert not differ, "pattern %s: arrays differ from the unpoisoned run's: %s" % (tag, differ)


def test_spectra_from_fids_feeds_the_device_pipeline():
    n_in, N = 2048, 4096
    sfrq, sw, tof = 100.0, 100.0, -350.0
    freqs, amps = (-0.2, 0.05, 0.31), (1.0, 0.7, 0.5)
    fids = []
    for k in range(2):
        s = synth.make_fid(n_in, [(f, 20 * np.pi / N, a) for f, a in zip(freqs, amps)], T=2, seed=4 + k, noise=0.002)
        x = s.fid.copy()
        x[:, 0] *= 0.5          # the usual first-point weight: without it the transform of a one-sided FID rides on a/2
        fids.append(x)
    datas = nmrfit_amd.spectra_from_fids(fids, sw, [sfrq, sfrq], tof, zero_fill=N)
    plain = fid.transform_many(fids, zero_fill=N)
    for d, (u, v, row) in zip(datas, plain):
        assert isinstance(d, nmrfit_amd.Data) and fs.same_bits(d.w, fid.ppm_axis(N, sw, sfrq, tof))
        assert fs.same_bits(d.u, u) and fs.same_bits(d.v, v) and d.w[0] < d.w[-1]
    nmrfit_amd.shift_phase_many(datas, method="auto")
    nmrfit_amd.select_peaks_many(datas, thresh=0.1)
    step = datas[0].w[1] - datas[0].w[0]
    want = sorted(datas[0].w[0] + synth.SynthFid.line_index(f, N) * step for f in freqs)
    for d in datas:
        locs = sorted(float(p.loc) for p in d.peaks)
        print("phase (%.4f, %.4f); peaks %s; lines %s; step %.3g" % (d.p0, d.p1, np.round(locs, 5), np.round(want, 5), step))
        assert len(locs) == 3 and all(abs(a - b) <= step for a, b in zip(locs, want)), (locs, want)
    with pytest.raises(ValueError, match="all zero"):
        nmrfit_amd.spectra_from_fids([fids[0], np.zeros(64, dtype=np.complex64)], sw, sfrq, tof, zero_fill="pow2")

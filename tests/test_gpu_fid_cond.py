"""
The FID conditioning on the device (csrc/fid_cond.hip, include/nmrfit_amd_fid_cond.h): Bruker group-delay removal in
its two forms and windows, in the library call that transforms.

  * nothing asked, nothing changed: form 0 without a window gives the bits of nmrfit_fid_transform;
  * a window alone: the conditioned trace is x * W per part bit for bit (signed zeros included), and jobs sharing a
    window agree with their lone calls;
  * everything after the conditioning is the existing path: u, v, rows and Y equal nmrfit_fid_transform applied to the
    returned conditioned traces bit for bit (forms 0 and 1); in form 2 Y is within the product's bar of the plain Y times
    the true ramp at every point, and u, v, rows equal fid.finish_host of the device's Y bit for bit;
  * form 1 and form 2 against the truth (fid.condition_host in long double) within the header's first-order bars
    (tests/fid_cond_support.py) -- the 2-norm of a trace's error, which bounds every single point's error too -- over
    s in {256, 512, 4096, 8192, 16384}, six group delays, T in {1, 3}, n = s and 2 s; an integer g is also held to the
    circular shift of x;
  * a spectrum gives the same bits alone, in a mixed batch, in the batch reversed and from a second call;
  * three child processes -- NMRFIT_POISON_ALLOC unset, 255, 63 -- give byte-identical outputs over the mixed batch;
  * spectra_from_fids(grpdly=) hands shift_phase_many / select_peaks_many a spectrum whose peaks sit where the lines are;
    without grpdly= the same FID does not get there.

Measured on the MI355X (the worst ratio error / bar): see DESIGN.md 4.15.1.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import nmrfit_amd
from nmrfit_amd import fid, synth
from tests import fid_cond_support as fc
from tests import fid_support as fs

pytestmark = pytest.mark.gpu

needs_truth = pytest.mark.skipif(not fs.truth_is_long_double(), reason="numpy's long-double transform is not available")


def _many(jobs, zero_fill="pow2"):
    """(x, g, mode, W) jobs in one call: (u, v, row, Y, xc) each."""
    return fid.transform_many([j[0] for j in jobs], zero_fill=zero_fill, grpdly=[j[1] for j in jobs], grpdly_mode=[j[2] for j in jobs],
                              window=[j[3] for j in jobs], truncate_grpdly=False, return_transform=True, return_conditioned=True)


def test_nothing_asked_nothing_changed():
    jobs = fs.poison_jobs()
    old = fid.transform_many(jobs, zero_fill="pow2", return_transform=True)
    new = fid.transform_many(jobs, zero_fill="pow2", return_transform=True, return_conditioned=True)
    for k, (o, nw, x) in enumerate(zip(old, new, jobs)):
        assert fs.same_result(nw[:4], o), k
        assert fs.same_values(nw[4].view(np.float64), x.view(np.float64)), k
    # without the optional outputs
    bare = fid.transform_many(jobs, zero_fill="pow2", grpdly=[None] * len(jobs))
    assert all(fs.same_result(b, o[:3]) for b, o in zip(bare, old))


def test_a_window_is_one_product_per_part():
    rng = np.random.default_rng(5)
    x = fs.sample_fid(1000, T=2, seed=31)
    x[0, :4] = [complex(-0.0, 0.0), complex(0.0, -0.0), complex(-0.0, -0.0), complex(1.0, -0.0)]
    x[1, 7] = complex(-0.0, 2.0)
    W = fid.window_em(1000, 2.0, 1000.0, first_point=0.5)
    W[1], W[2], W[3], W[9] = -1.0, 0.0, -0.0, -2.5
    y = fs.sample_fid(5000, T=1, seed=32)
    V = rng.standard_normal(5000)
    jobs = [(x, None, "fid", W), (x[:1] * 2.0, None, "fid", W.copy()), (y, None, "fid", V)]
    got = _many(jobs)
    for k, ((xx, _, _, ww), g) in enumerate(zip(jobs, got)):
        want = np.empty_like(xx)
        want.real, want.imag = xx.real * ww, xx.imag * ww
        assert fs.same_bits(g[4].view(np.float64), want.view(np.float64)), k          # (bits: the signed zeros too)
        assert fs.same_result(g, _many([jobs[k]])[0]), k                               # shared or not: the lone call's bits
        plain = fid.transform_many([g[4]], zero_fill="pow2", return_transform=True)[0]
        assert fs.same_result(g[:4], plain), k
    assert np.signbit(got[0][4].view(np.float64)).any()


def _check_against_truth(jobs, got, n_of, worst):
    for k, ((x, g, mode, W), (u, v, row, Y, xc)) in enumerate(zip(jobs, got)):
        n = n_of[k]
        form = fid._MODES[mode] if g is not None else fid.FORM_NONE
        xc_t, Y_t = fc.truth(x, g, mode, W, n)
        bar_c, bar_y = fc.bars(x, form, g, W, n)
        assert xc.shape == xc_t.shape and Y.shape == Y_t.shape == (len(x), n) and row[0] == 0
        rc = fc.ratio(xc, xc_t, bar_c) if form == fid.FORM_FID or W is not None else 0.0
        ry = fc.ratio(Y, Y_t, bar_y)
        print("s = %d, n = %d, T = %d, g = %r, %s%s: conditioned error / bar %.3g, spectrum error / bar %.3g"
              % (x.shape[1], n, len(x), g, mode, ", window" if W is not None else "", rc, ry))
        worst[0], worst[1] = max(worst[0], rc), max(worst[1], ry)
        assert rc <= 1.0 and ry <= 1.0, (k, rc, ry)
        if form == fid.FORM_FID and g == int(g):          # the circular shift of x, folded, cut, windowed
            s = x.shape[1]
            skip, add = fc.skip_add(g)
            want = np.roll(x.astype(np.clongdouble), -int(g), axis=-1)
            jj = np.arange(add)
            want[:, jj] = want[:, jj] + want[:, s - 1 - jj]
            want = want[:, :s - skip] * (1.0 if W is None else np.asarray(W, dtype=np.longdouble))
            assert fc.ratio(xc, want, bar_c) <= 1.0, k
        mu, mv, mrow = fid.finish_host(Y)
        assert fs.same_values(u, mu) and fs.same_values(v, mv) and fs.same_values(row, mrow), k


@needs_truth
@pytest.mark.parametrize("s", [256, 512, 4096, 8192, 16384])
def test_form_1_is_inside_the_bar_and_feeds_the_existing_path(s):
    """Short with even and odd log2, the full LDS block, two-pass odd and even; T = 3 jobs carry a window."""
    jobs = []
    for i, g in enumerate(fc.G_VALUES):
        n_out = s - fc.skip_add(g)[0]
        jobs.append((fs.sample_fid(s, 1, seed=40 + i), g, "fid", None))
        jobs.append((fs.sample_fid(s, 3, seed=50 + i), g, "fid", fid.window_em(n_out, 4.0, float(s), first_point=0.5)))
    worst = [0.0, 0.0]
    for zero_fill, n in (("pow2", s), (2 * s, 2 * s)):
        got = _many(jobs, zero_fill)
        _check_against_truth(jobs, got, [n] * len(jobs), worst)
        # everything after the conditioning is the existing path
        plain = fid.transform_many([g[4] for g in got], zero_fill=n, return_transform=True)
        for k, (g, p) in enumerate(zip(got, plain)):
            assert fs.same_result(g[:4], p), (n, k)
    print("s = %d: worst conditioned error / bar %.3g, worst spectrum error / bar %.3g" % (s, worst[0], worst[1]))


@needs_truth
def test_form_2_is_inside_the_bar():
    jobs, n_of = [], []
    for i, (n_in, n) in enumerate(((1, 2), (1, 1024), (1, 8192), (1000, 1024), (1000, 8192), (5000, 8192))):
        for j, g in enumerate(fc.G_VALUES):
            T = 3 if (i + j) % 2 else 1
            W = fid.window_sine(n_in, 0.0, 0.9, 2.0, first_point=0.5) if j % 3 == 0 and n_in > 1 else None
            jobs.append((fs.sample_fid(n_in, T, seed=60 + 7 * i + j), g, "spectrum", W))
            n_of.append(n)
    worst = [0.0, 0.0]
    for n in (2, 1024, 8192):
        sel = [k for k in range(len(jobs)) if n_of[k] == n]
        got = _many([jobs[k] for k in sel], n)
        _check_against_truth([jobs[k] for k in sel], got, [n] * len(sel), worst)
        # Y is the plain call's Y times the true ramp, at every point within the product's bar
        plain = fid.transform_many([g[4] for g in got], zero_fill=n, return_transform=True)
        for k, g, p in zip(sel, got, plain):
            rho = fid.ramp(jobs[k][1], n, np.clongdouble)
            d = np.abs(g[3].astype(np.clongdouble) - p[3].astype(np.clongdouble) * rho).astype(np.float64)
            assert np.all(d <= fc.KAPPA * np.abs(p[3])), k
    print("form 2: worst spectrum error / bar %.3g" % worst[1])


@pytest.fixture(scope="module")
def mixed():
    jobs = fc.mixed_jobs()
    alone = [fc.run_mixed([j])[0] for j in jobs]
    return jobs, alone


def test_a_spectrum_is_the_same_alone_in_the_batch_reversed_and_again(mixed):
    jobs, alone = mixed
    forms = {(j[1] is not None, j[2]) for j in jobs}
    assert {(True, "fid"), (True, "spectrum"), (False, "fid")} <= forms and {len(j[0]) for j in jobs} >= {1, 3}
    assert {j[0].shape[1] > 1 << fs.LDS_LOG2 for j in jobs} == {True, False}
    batch = fc.run_mixed(jobs)
    for k, (b, a) in enumerate(zip(batch, alone)):
        assert fs.same_result(b, a), k
    back = fc.run_mixed(jobs[::-1])[::-1]
    again = fc.run_mixed(jobs)
    for k, (r, g, a) in enumerate(zip(back, again, alone)):
        assert fs.same_result(r, a) and fs.same_result(g, a), k
    # the job with nothing asked is the plain call's
    plain = fid.transform_many([jobs[0][0]], zero_fill="pow2", return_transform=True)[0]
    assert fs.same_result(alone[0][:4], plain)


def test_results_do_not_depend_on_fresh_device_memory(tmp_path):
    files = {}
    for tag, poison in (("unset", None), ("255", "255"), ("63", "63")):
        out = str(tmp_path / ("fid_cond_%s.npz" % tag))
        env = dict(os.environ)
        env.pop("NMRFIT_POISON_ALLOC", None)
        if poison is not None:
            env["NMRFIT_POISON_ALLOC"] = poison
        try:
            run = subprocess.run([sys.executable, "-m", "tests.fid_cond_support", "poison", out], cwd=fs.ROOT, env=env,
                                 capture_output=True, text=True, timeout=60)
        except subprocess.TimeoutExpired as e:      # (no further child)
            pytest.fail("pattern %s: no exit within 60 s\n%s" % (tag, (e.stderr or b"")[-3000:]))
        # (a signal shows as a negative code: the same stop, and no further child)
        assert run.returncode == 0, "pattern %s: exit %d\n%s\n%s" % (tag, run.returncode, run.stdout[-1500:], run.stderr[-3000:])
        with np.load(out, allow_pickle=False) as z:
            files[tag] = {k: z[k] for k in z.files}
    base = files["unset"]
    assert len(base) == 5 * len(fc.mixed_jobs()) + 1
    for tag, poison in (("255", "255"), ("63", "63")):
        got = files[tag]
        assert str(got["__poison__"]) == poison and str(base["__poison__"]) == ""      # (the child did see the knob)
        assert set(got) == set(base)
        differ = [k for k in base if not k.startswith("__")
                  and (base[k].dtype != got[k].dtype or base[k].shape != got[k].shape or base[k].tobytes() != got[k].tobytes())]
        assert not differ, "pattern %s: arrays differ from the unpoisoned run's: %s" % (tag, differ)


def test_spectra_from_fids_removes_the_group_delay_for_the_device_pipeline():
    """The FIDs of test_gpu_fid.py's pipeline test, delayed by a Bruker group delay: with grpdly= the peaks are found where
    the lines are, to that test's tolerance (one grid step); without it the same FIDs do not get there."""
    n_in, N, g = 2048, 4096, 67.98416137695312          # (rounded to 68.0 by spectra_from_fids, as make_fid is given it)
    sfrq, sw, tof = 100.0, 100.0, -350.0
    freqs, amps = (-0.2, 0.05, 0.31), (1.0, 0.7, 0.5)
    lines = [(f, 20 * np.pi / N, a) for f, a in zip(freqs, amps)]
    delayed = [synth.make_fid(n_in, lines, T=2, seed=4 + k, noise=0.002, grpdly=68.0).fid for k in range(2)]
    n_out = fid.conditioned_length(n_in, 68.0)
    W = fid.window_em(n_out, 0.0, sw, first_point=0.5)   # the usual first-point weight alone
    step = None

    def peaks_of(datas):
        nmrfit_amd.shift_phase_many(datas, method="auto")
        nmrfit_amd.select_peaks_many(datas, thresh=0.1)
        return [sorted(float(p.loc) for p in d.peaks) for d in datas]

    datas = nmrfit_amd.spectra_from_fids(delayed, sw, sfrq, tof, zero_fill=N, grpdly=g, window=W)
    step = datas[0].w[1] - datas[0].w[0]
    want = sorted(datas[0].w[0] + synth.SynthFid.line_index(f, N) * step for f in freqs)
    for d, locs in zip(datas, peaks_of(datas)):
        print("with grpdly: phase (%.4f, %.4f); peaks %s; lines %s; step %.3g" % (d.p0, d.p1, np.round(locs, 5), np.round(want, 5), step))
        assert len(locs) == 3 and all(abs(a - b) <= step for a, b in zip(locs, want)), (locs, want)
    # the undelayed FIDs, cut to the same points and windowed alike, get there as well (what the removal leaves besides
    # rounding is the fold: the FID's last 62 points, noise included, added to its first)
    clean = [synth.make_fid(n_in, lines, T=2, seed=4 + k, noise=0.002).fid[:, :n_out] for k in range(2)]
    same = nmrfit_amd.spectra_from_fids(clean, sw, sfrq, tof, zero_fill=N, window=W)
    for d, e, locs in zip(datas, same, peaks_of(same)):
        print("undelayed: phase (%.4f, %.4f) against (%.4f, %.4f) after the removal" % (e.p0, e.p1, d.p0, d.p1))
        assert len(locs) == 3 and all(abs(a - b) <= step for a, b in zip(locs, want)), (locs, want)
    # without grpdly= the delayed FIDs keep 68 turns of first-order phase, which (p0, p1) in [-pi, pi] cannot repair
    raw = nmrfit_amd.spectra_from_fids(delayed, sw, sfrq, tof, zero_fill=N, window=np.concatenate((W, np.ones(n_in - n_out))))
    for d, locs in zip(raw, peaks_of(raw)):
        print("without grpdly: phase (%.4f, %.4f); %d peaks %s" % (d.p0, d.p1, len(locs), np.round(locs[:6], 5)))
        assert not (len(locs) == 3 and all(abs(a - b) <= step for a, b in zip(locs, want))), locs

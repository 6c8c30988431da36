"""
The polynomial baselines on the device (csrc/baseline.hip, include/nmrfit_amd_baseline.h).

  * the device's rows and baselines equal the numpy mirror (baseline.fit_host: the definition's order and solve) bit for
    bit over the whole case list of tests/baseline_support.py -- so the bounds that tests/test_baseline_cpu.py holds the
    mirror to against the exact polynomial are the device's;
  * a job gives the same bits alone, in any ragged batch and as either channel;
  * the resident call on a device batch gives the rows of baseline.fit_many on generate()'s data_V - V and leaves the
    swarms alone;
  * the user-level calls: sample_noise_many against the exact sigma, correct_baseline_many against the exact polynomial,
    fit_many(residual_baseline=...) against the lone path;
  * three child processes -- NMRFIT_POISON_ALLOC unset, 255, 63 -- give byte-identical outputs.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import nmrfit_amd
from nmrfit_amd import _cabi, baseline, containers, synth
from tests import baseline_support as bs

pytestmark = pytest.mark.gpu
BOUND_E = bs.BOUND_E


@pytest.fixture(scope="module")
def case_list():
    return bs.cases()


@pytest.fixture(scope="module")
def mirrored(case_list):
    return [baseline.fit_host(c.w, c.y, c.deg, c.intervals, c.complement) for c in case_list]


def test_the_device_equals_the_mirror_bit_for_bit(case_list, mirrored):
    got = bs.device_fits(case_list)
    differ = [c.name for c, g, m in zip(case_list, got, mirrored)
              if not (bs.same_row(g.row, m.row) and bs.same_row(g.baseline, m.baseline))]
    assert not differ, "%d of %d jobs differ from the mirror: %s" % (len(differ), len(case_list), differ[:12])
    assert sorted(set(g.status for g in got)) == [0, 1, 2]
    # without the baseline output: the same rows
    rows_only = bs.device_fits(case_list[::7], return_baseline=False)
    assert all(r.baseline is None and bs.same_row(r.row, g.row) for r, g in zip(rows_only, got[::7]))


def test_a_job_is_the_same_alone_in_any_batch_and_as_either_channel(case_list, mirrored):
    rng = np.random.default_rng(21)
    pick = [int(i) for i in rng.choice(len(case_list), 24, replace=False)]
    for i in pick[:6]:
        lone = bs.device_fits([case_list[i]])[0]
        assert bs.same_row(lone.row, mirrored[i].row) and bs.same_row(lone.baseline, mirrored[i].baseline), case_list[i].name
    for _ in range(6):
        K = int(rng.integers(2, 13))
        idx = [pick[j] for j in rng.permutation(len(pick))[:K]]
        got = bs.device_fits([case_list[i] for i in idx])
        for i, g in zip(idx, got):
            assert bs.same_row(g.row, mirrored[i].row) and bs.same_row(g.baseline, mirrored[i].baseline), case_list[i].name
    # as channel 0 and as channel 1 of two-channel spectra (the partner: the reversed values), mixed with lone channels
    idx = pick[:12]
    cl = [case_list[i] for i in idx]
    ys = [np.array([c.y, c.y[::-1]]) if k % 3 == 0 else (np.array([c.y[::-1], c.y]) if k % 3 == 1 else c.y) for k, c in enumerate(cl)]
    got = baseline.fit_many([c.w for c in cl], ys, deg=[c.deg for c in cl], intervals=[c.intervals for c in cl],
                            complement=[c.complement for c in cl])
    for k, (i, g) in enumerate(zip(idx, got)):
        mine = g[0] if k % 3 == 0 else (g[1] if k % 3 == 1 else g)
        assert bs.same_row(mine.row, mirrored[i].row) and bs.same_row(mine.baseline, mirrored[i].baseline), case_list[i].name


def test_the_resident_call_on_a_device_batch():
    sps, intervals = bs.resident_problem()
    degs = [1, 2, 4]
    with bs.make_batch(sps) as a, bs.make_batch(sps) as b:
        with pytest.raises(_cabi.NmrfitError) as ei:
            a.residual_baseline(deg=1, intervals=intervals)
        assert ei.value.code == _cabi.E_STATE
        X0 = [0.5 * (sp["lower"] + sp["upper"]) for sp in sps]
        assert [f.status for f in a.residual_baseline(X0, deg=degs, intervals=intervals)] == [0, 0, 0]      # any state with X
        a.run(5, 5)
        mid = a.residual_baseline(deg=degs, intervals=intervals, return_baseline=True)
        X = [x for x, _ in a.best()]
        at_x = a.residual_baseline(X, deg=degs, intervals=intervals, return_baseline=True)
        gen = a.generate()
        host = baseline.fit_many([sp["w"] for sp in sps], [g["data_V"] - g["V"] for g in gen], deg=degs, intervals=intervals,
                                 complement=True)
        for k in range(3):
            assert mid[k].status == 0 and mid[k].deg == degs[k]
            for got in (mid[k], at_x[k]):
                assert bs.same_row(got.row, host[k].row) and bs.same_bits(got.baseline, host[k].baseline), k
            mirror = baseline.fit_host(sps[k]["w"], gen[k]["data_V"] - gen[k]["V"], degs[k], intervals[k], True)
            assert bs.same_row(mid[k].row, mirror.row)
        # intervals as they are (no complement), one degree for all, no baseline output
        inside = a.residual_baseline(deg=0, intervals=intervals, complement=False)
        assert all(f.baseline is None and f.status == 0 and f.n < len(sp["w"]) for f, sp in zip(inside, sps))
        a.run(5, 5)
        b.run(10, 5)
        for (xa, fa), (xb, fb) in zip(a.best(), b.best()):
            assert np.array_equal(xa, xb) and fa == fb
        for k in range(3):
            sa, sb = a.state(k), b.state(k)
            assert all(np.array_equal(sa[name], sb[name]) for name in sa)
        assert [s["iteration"] for s in a.status()] == [s["iteration"] for s in b.status()]


def test_sample_noise_many_against_the_exact_sigma():
    rng = np.random.default_rng(8)
    ws, ys, regions, want = [], [], [], []
    for k, N in enumerate((320, 1000, 4096)):
        w = np.linspace(3.0, 4.0, N)[::-1].copy()
        u = 0.3 * (w - 3.2) ** 2 + 0.02 * rng.standard_normal(N)
        v = -0.1 * (w - 3.0) + 0.05 * rng.standard_normal(N)
        ws.append(w)
        ys.append(np.array([u, v]))
        regions.append((3.05 + 0.01 * k, 3.3))
        want.append([bs.exact_fit(bs.Case("noise", w, y, 2, [regions[-1]], False))[1] for y in (u, v)])
    got = baseline.sample_noise_many(ws, ys, regions)
    for k in range(3):
        n = int(((ws[k] >= regions[k][0]) & (ws[k] <= regions[k][1])).sum())
        for ch in range(2):
            frac = abs(got[k][ch] - want[k][ch]) / (n * bs.EPS * want[k][ch])
            print("sample_noise_many: spectrum %d channel %d sigma %.6g, used fraction of the bound %.3g" % (k, ch, got[k][ch], frac))
            assert frac <= 1.0
            # the reference's number, to the accuracy np.polyfit has on raw ppm values at degree 2
            host = nmrfit_amd.peaks.sample_noise(ws[k], ys[k][ch], *regions[k])
            assert abs(host - got[k][ch]) <= 1e-9 * got[k][ch]
    one = baseline.sample_noise_many(ws[:1], [ys[0][0]], regions[0])
    assert one == [got[0][0]]


def test_correct_baseline_many_recovers_a_known_quadratic():
    datas, held, rolls = [], [], []
    for k, N in enumerate((700, 1000)):
        sp = synth.make_spectrum(N, 2, seed=40 + k, physical=True)
        d = containers.Data(sp["w"], sp["u"].copy(), sp["v"].copy())
        d.shift_phase(method="manual", p0=0.1 * k, p1=0.05)
        roll = 0.04 - 0.03 * (sp["w"] - 3.5) + 0.2 * (sp["w"] - 3.4) ** 2
        d.V = d.V + roll
        d.peaks = sp["peaks"]
        datas.append(d)
        rolls.append(roll)
        held.append((d.u, d.v, d.V, d.I, d.V.copy(), d.u.copy(), d.v.copy()))
    containers.correct_baseline_many(datas, deg=2, margin=3.0)
    for d, (u, v, V, I, V0, u0, v0), roll in zip(datas, held, rolls):
        assert bs.same_bits(V, V0) and bs.same_bits(u, u0) and bs.same_bits(v, v0)
        assert not np.shares_memory(d.u, u) and not np.shares_memory(d.v, v) and not np.shares_memory(d.V, V)
        bV, bI = d.baseline
        exclude = baseline.widened([tuple(p.bounds) for p in d.peaks], 3.0)
        case = bs.Case("roll", d.w, V0, 2, exclude, True)
        truth, _ = bs.exact_fit(case)
        m = case.mask()
        err = np.abs(bV.baseline[m] - truth[m]).max() / (bs.EPS * np.abs(V0[m]).max())
        print("correct_baseline_many: N %d, %d points outside the peaks, error %.3g e" % (len(d.w), bV.n, err))
        assert bV.status == 0 and err <= BOUND_E
        assert bs.same_bits(d.V, V0 - bV.baseline)
        # the quadratic that was added, to what the peaks' tails and the noise outside +-3 bounds leave
        assert np.abs(bV.baseline[m] - roll[m]).max() < 0.05 * np.abs(roll).max() + 5 * bV.sigma


def test_fit_many_attaches_the_residual_baseline():
    def jobs():
        out = []
        for k, N in enumerate((320, 400, 320)):
            sp = synth.make_spectrum(N, 2, seed=60 + k)
            out.append(dict(data=synth.SynthData(sp["w"], sp["u"], sp["v"], sp["peaks"]), lower=list(sp["lower"]),
                            upper=list(sp["upper"]), options=dict(swarmsize=16, maxiter=8, seed=5 + k)))
        return out
    batched = nmrfit_amd.fit_many(jobs(), residual_baseline=1)
    plain = nmrfit_amd.fit_many(jobs())
    lone = nmrfit_amd.fit_many(jobs(), batch=False, residual_baseline=dict(deg=1, return_baseline=True))
    for fb, fp, fl in zip(batched, plain, lone):
        assert np.array_equal(fb.params, fp.params) and fb.error == fp.error and "residual_baseline" not in vars(fp)
        assert np.array_equal(fb.params, fl.params)
        rb = fb.residual_baseline
        assert isinstance(rb, baseline.BaselineFit) and rb.status == 0 and rb.deg == 1 and rb.baseline is None
        assert bs.same_row(rb.row, fl.residual_baseline.row) and fl.residual_baseline.baseline is not None
        assert bs.same_bits(rb(fb.data.w), fl.residual_baseline.baseline)


def test_fit_replicas_many_takes_its_sigmas_from_one_device_call(monkeypatch):
    from nmrfit_amd import noise

    def jobs():
        out = []
        for k in range(2):
            sp = synth.make_spectrum(320, 2, seed=70 + k)
            out.append(dict(data=synth.SynthData(sp["w"], sp["u"], sp["v"], sp["peaks"]), lower=list(sp["lower"]),
                            upper=list(sp["upper"]), noise_region=(3.4, 3.6)))
        return out
    kw = dict(replicas=2, seed=3, options=dict(swarmsize=16, maxiter=6))
    host = nmrfit_amd.fit_replicas_many(jobs(), **kw)
    calls = []
    real = baseline.sample_noise_many
    monkeypatch.setattr(baseline, "sample_noise_many", lambda *a, **k: calls.append(len(a[0])) or real(*a, **k))
    dev = nmrfit_amd.fit_replicas_many(jobs(), device_sigma=True, **kw)
    assert calls == [2]                                                       # one call for all jobs
    again = nmrfit_amd.fit_replicas_many(jobs(), **kw)
    for h, d, a, job in zip(host, dev, again, jobs()):
        assert np.array_equal(h.sigma, a.sigma) and np.array_equal(h.params, a.params)      # the default: the host path, bit for bit
        assert np.array_equal(h.sigma[1], noise._job_sigma(job, job["data"]))
        assert np.all(np.abs(d.sigma - h.sigma) <= 1e-9 * h.sigma) and np.all(d.sigma[1] > 0)
        assert np.array_equal(d.params[0], h.params[0])                       # fit 0 is the data as it is


def test_results_do_not_depend_on_fresh_device_memory(tmp_path):
    files = {}
    for tag, poison in (("unset", None), ("255", "255"), ("63", "63")):
        out = str(tmp_path / ("baseline_%s.npz" % tag))
        env = dict(os.environ)
        env.pop("NMRFIT_POISON_ALLOC", None)
        if poison is not None:
            env["NMRFIT_POISON_ALLOC"] = poison
        try:
            run = subprocess.run([sys.executable, "-m", "tests.baseline_support", "poison", out], cwd=bs.ROOT, env=env,
                                 capture_output=True, text=True, timeout=60)
        except subprocess.TimeoutExpired as e:      # (no further child)
            pytest.fail("pattern %s: no exit within 60 s\n%s" % (tag, (e.stderr or b"")[-3000:]))
        # (a signal shows as a negative code: the same stop, and no further child)
        assert run.returncode == 0, "pattern %s: exit %d\n%s\n%s" % (tag, run.returncode, run.stdout[-1500:], run.stderr[-3000:])
        with np.load(out, allow_pickle=False) as z:
            files[tag] = {k: z[k] for k in z.files}
    base = files["unset"]
    assert len(base) >= 9
    for tag, poison in (("255", "255"), ("63", "63")):
        got = files[tag]
        assert str(got["__poison__"]) == poison and str(base["__poison__"]) == ""      # (the child did see the knob)
        assert set(got) == set(base)
        differ = [k for k in base if not k.startswith("__")
                  and (base[k].dtype != got[k].dtype or base[k].shape != got[k].shape or base[k].tobytes() != got[k].tobytes())]
        assert not differ, "pattern %s: arrays differ from the unpoisoned run's: %s" % (tag, differ)

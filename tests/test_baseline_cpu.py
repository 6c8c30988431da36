"""
CPU tier of the polynomial baselines (nmrfit_amd/baseline.py, csrc/baseline.hip, include/nmrfit_amd_baseline.h): the
numpy mirror of the device's arithmetic against the exact least-squares polynomial (tests/baseline_support.py), the
ctypes table against the header, the library's argument checks (made before any device work), the kernels' resources,
and the host-side pieces (subtract_rotated, correct_baseline_many, the fit_many keyword).

Measured over the case list (635 jobs, 535 with a truth), in units of e = 2^-52 max|y| over the mask: the mirror's worst
baseline error is 5.06 e (descending/N1000/interval/d8); np.polyfit on raw w, the method of peaks.sample_noise, reaches
1.7e15 e.  The mirror's sigma uses at most 0.029 of its bound n 2^-52 sigma.
"""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from nmrfit_amd import _cabi, baseline
from tests import baseline_support as bs

ROOT = bs.ROOT
BOUND_E = bs.BOUND_E


@pytest.fixture(scope="module")
def judged():
    """Per case with a truth: (case, the mirror's fit, the exact values, the exact sigma) -- computed once."""
    out = []
    for c in bs.cases():
        f = baseline.fit_host(c.w, c.y, c.deg, c.intervals, c.complement)
        if f.status == 0 and c.has_truth():
            out.append((c, f) + bs.exact_fit(c))
    return out


def test_the_mirror_against_the_exact_polynomial(judged):
    """The mirror's baseline, over the masked points and all points with |t| <= 1, stays within BOUND_E units of
    2^-52 max|y|; and wherever np.polyfit is off by more than 4 units the mirror is no worse than it."""
    assert len(judged) >= 500
    worst, worst_polyfit, at = 0.0, 0.0, None
    for c, f, truth, _ in judged:
        err = bs.baseline_error(c, f.baseline, truth)
        ref = bs.baseline_error(c, bs.polyfit_baseline(c), truth)
        if err > worst:
            worst, at = err, c.name
        worst_polyfit = max(worst_polyfit, ref)
        if ref > 4.0:
            assert err <= ref, (c.name, err, ref)
    print("mirror against the exact polynomial: worst error %.3g e (%s); np.polyfit's worst %.3g e" % (worst, at, worst_polyfit))
    assert worst <= BOUND_E, (worst, at)
    assert worst_polyfit > 100.0      # (what the issue found: the raw-ppm fit is off by far more than the conditioned one)


def test_the_mirror_sigma_against_the_exact_sigma(judged):
    """|sigma - sigma_truth| <= n 2^-52 sigma_truth, the first-order bound of a sum of n rounded terms.  Where the
    polynomial interpolates (n = d + 1) the exact residual is zero and what is left is the baseline's own error."""
    used, at = 0.0, None
    for c, f, _, sigma in judged:
        if f.n == c.deg + 1:
            assert sigma == 0.0 and f.sigma <= BOUND_E * bs.EPS * np.abs(c.y[c.mask()]).max(), (c.name, f.sigma)
            continue
        assert sigma > 0.0, c.name
        frac = abs(f.sigma - sigma) / (f.n * bs.EPS * sigma)
        if frac > used:
            used, at = frac, c.name
    print("mirror sigma against the exact sigma: used fraction of the bound %.3g (%s)" % (used, at))
    assert used <= 1.0, (used, at)


def test_statuses_and_nan_rules_of_the_mirror():
    by_name = {c.name: c for c in bs.cases()}

    def fit(name):
        c = by_name[name]
        return c, baseline.fit_host(c.w, c.y, c.deg, c.intervals, c.complement)
    for d in bs.DEGS:
        c, f = fit("empty/d%d" % d)
        assert f.status == 1 and f.n == 0 and np.isnan(f.row[2:7]).all() and np.isnan(f.baseline).all()
        assert np.isnan(f.row[8:9 + d]).all() and not f.row[9 + d:].any() and np.isnan(f.sigma)
        assert fit("empty_complement/d%d" % d)[1].status == 1
        c, f = fit("one_short/d%d" % d)
        assert f.status == (2 if d else 1) and f.n == d and np.isnan(f.coef).all()
        c, f = fit("interpolates/d%d" % d)
        assert f.status == 0 and f.n == d + 1
        c, f = fit("all_equal/d%d" % d)      # 67 equal points: a constant fits, nothing higher does
        assert f.n == 67 and f.domain == (3.25, 3.25) and f.status == (0 if d == 0 else 2)
        c, f = fit("r_limit/d%d" % d)
        assert f.status == 0 and len(c.intervals) == baseline.MAX_INTERVALS and f.n == int(((c.w >= 3.4) & (c.w <= 3.8)).sum())
        c, f = fit("inf_edges/all/d%d" % d)
        assert f.n == len(c.w) and f.status == 0
        c, f = fit("y_nan_inside/N257/whole/d%d" % d)
        assert f.status == 0 and np.isnan(f.coef).all() and np.isnan(f.baseline).all() and np.isnan(f.sigma) and f.rcond > 0
        c, f = fit("y_nan_outside/N257/interval/d%d" % d)
        assert f.status == 0 and np.isfinite(f.row).all() and np.isfinite(f.baseline).all()
        c, f = fit("nan_w/N257/whole/d%d" % d)
        # (b_j = c_0 + c_i T_i(t_j): at a NaN w_j it is NaN as soon as there is a term in t)
        assert f.n == 256 and np.isnan(f.baseline[128]) == (d > 0) and np.isfinite(np.delete(f.baseline, 128)).all()
    # N = 1: a constant through the point; any higher degree is short of points
    assert [fit("ascending/N1/whole/d%d" % d)[1].status for d in bs.DEGS] == [0, 2, 2, 2, 2]
    # the object evaluates its own polynomial by the device's recurrence
    c, f = fit("shuffled/N320/outside2/d4")
    assert bs.same_bits(f(c.w), f.baseline)


def _declared(header):
    text = open(os.path.join(ROOT, "include", header)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return set(re.findall(r"\b(nmrfit_[a-z0-9_]+)\s*\(", text))


def test_table_and_header():
    """BASELINE_SIGNATURES is what include/nmrfit_amd_baseline.h declares, the library exports it, no name is shared
    with another header or table, the product header and the ABI number are as they were."""
    names = _declared("nmrfit_amd_baseline.h")
    assert names == set(_cabi.BASELINE_SIGNATURES) == {"nmrfit_baseline_fit", "nmrfit_batch_residual_baseline"}
    for header in sorted(os.listdir(os.path.join(ROOT, "include"))):
        if header.endswith(".h") and header != "nmrfit_amd_baseline.h":
            assert not (names & _declared(header)), header
    for table in (_cabi.ALL_SIGNATURES, _cabi.PREP_SIGNATURES, _cabi.LSQ_SIGNATURES, _cabi.LSQ_IM_SIGNATURES,
                  _cabi.NOISE_SIGNATURES, _cabi.QUALITY_SIGNATURES):
        assert not (names & set(table))
    assert len(_declared("nmrfit_amd.h")) == 46
    L = _cabi.lib()
    for n in names:
        assert hasattr(L, n), n
    assert L.nmrfit_abi_version() == _cabi.ABI_VERSION == 6
    text = open(os.path.join(ROOT, "include", "nmrfit_amd_baseline.h")).read()
    assert "#define NMRFIT_BASELINE_MAX_INTERVALS %d" % baseline.MAX_INTERVALS in text
    assert "#define NMRFIT_BASELINE_ROW %d" % baseline.ROW in text and "#define NMRFIT_BASELINE_MAX_DEG %d" % baseline.MAX_DEG in text
    import nmrfit_amd
    assert nmrfit_amd.baseline is baseline and nmrfit_amd.BaselineFit is baseline.BaselineFit


def test_argument_validation_needs_no_gpu():
    """nmrfit_baseline_fit reports every argument error of the header as NMRFIT_E_INVALID and the per-call limits as
    NMRFIT_E_UNSUPPORTED before anything touches a device; an impossible device index is answered by the shared check,
    as for nmrfit_weights_build; the batch call refuses a null handle."""
    L = _cabi.lib()
    p = _cabi.ptr
    i32, i64 = (lambda a: np.array(a, dtype=np.int32)), (lambda a: np.array(a, dtype=np.int64))
    N, w, y = i64([4, 3]), np.arange(7.0), np.zeros(14)
    deg, R, comp = i32([1, 0]), i32([1, 2]), i32([0, 1])
    edges = np.array([0.0, 1.0, -np.inf, np.inf, 2.0, 1.0])
    rows, base = np.zeros(2 * 2 * baseline.ROW), np.zeros(14)

    def call(device=0, K=2, N=N, w=w, C=2, y=y, deg=deg, R=R, edges=edges, comp=comp, rows=rows, base=base):
        return L.nmrfit_baseline_fit(device, K, p(N), p(w), C, p(y), p(deg), p(R), p(edges), p(comp), p(rows), p(base))
    for name in ("N", "w", "y", "deg", "R", "comp", "rows"):
        assert call(**{name: None}) == _cabi.E_INVALID, name
    assert call(edges=None) == _cabi.E_INVALID and b"edges" in L.nmrfit_last_error()
    assert call(K=0) == _cabi.E_INVALID and call(K=-1) == _cabi.E_INVALID
    assert call(N=i64([4, 0])) == _cabi.E_INVALID and call(N=i64([-4, 3])) == _cabi.E_INVALID
    assert call(R=i32([1, -1])) == _cabi.E_INVALID
    assert call(deg=i32([1, -1])) == _cabi.E_INVALID and call(deg=i32([9, 0])) == _cabi.E_INVALID
    assert call(C=0) == _cabi.E_INVALID and call(C=3) == _cabi.E_INVALID
    bad = edges.copy()
    bad[5] = np.nan
    assert call(edges=bad) == _cabi.E_INVALID and b"NaN" in L.nmrfit_last_error()
    assert call(N=i64([_cabi.WEIGHTS_MAX_POINTS, 1])) == _cabi.E_UNSUPPORTED
    many = 65536
    assert L.nmrfit_baseline_fit(0, many, p(np.ones(many, dtype=np.int64)), p(w), 1, p(y), p(np.zeros(many, dtype=np.int32)),
                                 p(np.zeros(many, dtype=np.int32)), None, p(np.zeros(many, dtype=np.int32)), p(rows),
                                 None) == _cabi.E_UNSUPPORTED
    big = i32([baseline.MAX_INTERVALS + 1, 0])
    assert call(R=big, edges=np.zeros(2 * int(big.sum()))) == _cabi.E_UNSUPPORTED
    # valid calls: infinite edges, no baseline output, no interval anywhere -- what is reported then is the missing
    # device (or, with a GPU, nothing)
    assert call() in (_cabi.OK, _cabi.E_NO_DEVICE)
    assert call(base=None) in (_cabi.OK, _cabi.E_NO_DEVICE)
    assert call(R=i32([0, 0]), edges=None) in (_cabi.OK, _cabi.E_NO_DEVICE)
    # an impossible device index: the shared check's answer, the one nmrfit_weights_build gives
    assert call(device=1 << 20) == _cabi.E_NO_DEVICE
    mine = L.nmrfit_last_error()
    out = np.zeros(7)
    assert L.nmrfit_weights_build(1 << 20, 2, p(N), p(w), p(i32([0, 0])), None, None, p(out), None) == _cabi.E_NO_DEVICE
    assert mine == L.nmrfit_last_error() and mine
    assert L.nmrfit_batch_residual_baseline(None, None, p(deg), p(R), p(edges), p(comp), p(rows), None) == _cabi.E_INVALID
    assert b"null batch handle" in L.nmrfit_last_error()


def test_python_argument_errors_come_before_the_library(monkeypatch):
    monkeypatch.setattr(_cabi, "lib", lambda: pytest.fail("the library was reached"))
    w, y = np.linspace(3, 4, 10), np.zeros(10)
    with pytest.raises(ValueError):
        baseline.fit_many([w], [y, y])
    with pytest.raises(ValueError):
        baseline.fit_many([w], [np.zeros(9)])
    with pytest.raises(ValueError):
        baseline.fit_many([w], [np.zeros((3, 10))])
    with pytest.raises(ValueError):
        baseline.fit_many([w], [y], deg=9)
    with pytest.raises(ValueError):
        baseline.fit_many([w, w], [y, y], intervals=[[(3.0, 3.5)]])
    with pytest.raises(ValueError):
        baseline.sample_noise_many([w, w], [y, y], [(3.0, 3.5)] * 3)
    with pytest.raises(ValueError):
        baseline.option(dict(degree=2))
    assert baseline.option(None) is None and baseline.option(2)["deg"] == 2 and baseline.option(True)["deg"] == 1
    assert baseline.widened([(3.0, 3.2), (3.6, 3.5)], 2.0) == [(3.1 - 0.2, 3.1 + 0.2), (3.55 - 0.1, 3.55 + 0.1)]


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="hipcc not available")
def test_kernel_resources():
    """tools/kernel_resources.py --check --unit baseline.hip: every instantiation of the job kernel and the gather
    kernel without scratch memory and without spills."""
    run = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"), "--check", "--unit", "baseline.hip"],
                         capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, run.stdout[-3000:] + run.stderr[-3000:]
    lines = [ln.split() for ln in run.stdout.splitlines() if ln.startswith("baseline_")]
    names = [ln[0] for ln in lines]
    assert sorted(names) == ["baseline_jobs_kernel<2>", "baseline_jobs_kernel<4>", "baseline_jobs_kernel<8>",
                             "baseline_residual_kernel"], run.stdout
    for ln in lines:      # kernel VGPR AGPR scratch waves LDS s-spill
        assert int(ln[3]) == 0 and int(ln[6]) == 0 and int(ln[1]) <= 128, ln
    print(run.stdout)


def test_subtract_rotated_inverts_adding_a_rotated_baseline():
    from nmrfit_amd.proc_autophase import ps2
    rng = np.random.default_rng(5)
    N, p0, p1 = 777, 0.3, -1.1
    u, v, b = rng.standard_normal(N), rng.standard_normal(N), 0.1 * np.linspace(-1, 2, N) ** 2
    du, dv = ps2(b, np.zeros(N), p0, p1, inv=True)
    u2, v2 = baseline.subtract_rotated(u + du, v + dv, b, p0, p1)
    assert np.abs(u2 - u).max() <= 8 * bs.EPS * 4 and np.abs(v2 - v).max() <= 8 * bs.EPS * 4
    assert not np.shares_memory(u2, u) and not np.shares_memory(v2, v)
    # in the phased frame: V drops by b, I stays
    V, I = ps2(u, v, p0, p1)
    V2, I2 = ps2(*baseline.subtract_rotated(u, v, b, p0, p1), p0, p1)
    assert np.abs(V2 - (V - b)).max() <= 16 * bs.EPS * 4 and np.abs(I2 - I).max() <= 16 * bs.EPS * 4


def _host_fit_many(ws, ys, deg=2, intervals=None, complement=False, device=0, return_baseline=True):
    """baseline.fit_many by the mirror."""
    K = len(ws)
    d, c = baseline.per_spectrum(deg, K, "deg"), baseline.per_spectrum(complement, K, "complement")
    iv = [None] * K if intervals is None else intervals
    out = []
    for k in range(K):
        y = np.asarray(ys[k])
        fits = [baseline.fit_host(ws[k], row, d[k], iv[k], c[k]) for row in np.atleast_2d(y)]
        out.append(fits[0] if y.ndim == 1 else tuple(fits))
    return out


def _phased_data(N, seed, roll):
    from nmrfit_amd import containers, synth
    sp = synth.make_spectrum(N, 2, seed=seed, physical=True)
    d = containers.Data(sp["w"], sp["u"].copy(), sp["v"].copy())
    d.shift_phase(method="manual", p0=0.2, p1=-0.1)
    d.V = d.V + roll(sp["w"])
    d.peaks = sp["peaks"]
    return d


def test_correct_baseline_many_writes_all_or_nothing(monkeypatch):
    from nmrfit_amd import containers
    from nmrfit_amd.proc_autophase import ps2
    monkeypatch.setattr(baseline, "fit_many", _host_fit_many)
    roll = lambda w: 0.05 + 0.02 * (w - 3.5)      # noqa: E731
    datas = [_phased_data(300, 1, roll), _phased_data(500, 2, roll)]
    held = [(d.u, d.v, d.V, d.I, d.V.copy(), d.I.copy(), d.u.copy(), d.v.copy()) for d in datas]
    # spectrum 1 cannot be fitted (everything excluded): nothing is written anywhere
    with pytest.raises(ValueError, match="spectrum 1"):
        containers.correct_baseline_many(datas, deg=1, exclude=[[(3.4, 3.6)], [(0.0, 10.0)]])
    for d, (u, v, V, I, V0, I0, u0, v0) in zip(datas, held):
        assert d.u is u and d.v is v and d.V is V and d.I is I and not hasattr(d, "baseline")
        assert bs.same_bits(V, V0) and bs.same_bits(I, I0) and bs.same_bits(u, u0) and bs.same_bits(v, v0)
    # a Data cropped and not re-phased
    short = _phased_data(300, 3, roll)
    short.w = short.w[:200]
    with pytest.raises(ValueError, match="len"):
        containers.correct_baseline_many([datas[0], short])
    assert datas[0].V is held[0][2]
    # the default: outside the peaks' bounds; new arrays everywhere, the caller's untouched
    out = containers.correct_baseline_many(datas, deg=1, margin=2.0)
    assert out == datas
    for d, (u, v, V, I, V0, I0, u0, v0) in zip(datas, held):
        assert bs.same_bits(V, V0) and bs.same_bits(I, I0) and bs.same_bits(u, u0) and bs.same_bits(v, v0)
        for new, old in ((d.V, V), (d.I, I), (d.u, u), (d.v, v)):
            assert not np.shares_memory(new, old)
        bV, bI = d.baseline
        assert bV.status == 0 and bI.status == 0 and bV.deg == 1
        want = baseline.fit_host(d.w, V0, 1, baseline.widened([tuple(p.bounds) for p in d.peaks], 2.0), True)
        assert bs.same_row(bV.row, want.row) and bs.same_bits(d.V, V0 - want.baseline)
        uu, vv = ps2(d.V, d.I, d.p0, d.p1, inv=True)
        assert bs.same_bits(d.u, uu) and bs.same_bits(d.v, vv)


def test_fit_many_reads_the_residual_baseline_while_the_batch_is_resident(monkeypatch):
    """The keyword travels in _Call like ``quality``: the fits that store would polish one by one are polished first,
    the resident call is made at the final parameters outside the peaks' widened bounds before the batch closes, and
    store hands each fit its row.  Without the keyword nothing of this happens."""
    from nmrfit_amd import core, synth, utils

    class Resident:
        def __init__(self, fits):
            self.fits, self.calls = fits, []

        def status(self):
            return [dict(iteration=3, stop=0, fg=1.0) for _ in self.fits]

        def best(self):
            return [(np.full(len(f.lower), float(k)), 10.0 + k) for k, f in enumerate(self.fits)]

        def residual_baseline(self, X, **kw):
            self.calls.append(("baseline", [np.array(x) for x in X], kw))
            return ["row %d" % k for k in range(len(X))]

        def close(self):
            self.calls.append(("close",))
    monkeypatch.setattr(utils.FitUtility, "_polish", lambda self, xopt, fopt, plan: (xopt - 0.5, 0.5))
    assert core._Call(1, True, {}, False, False, False).residual_baseline is None
    for asked in (dict(deg=2, margin=3.0), None):
        fits = []
        for k, opts in enumerate(({"polish": True}, {})):
            sp = synth.make_spectrum(256, 2, seed=90 + k)
            fits.append(utils.FitUtility(synth.SynthData(sp["w"], sp["u"], sp["v"], sp["peaks"]), list(sp["lower"]),
                                         list(sp["upper"]), summary=False, options=opts))
        plans = [f._plan() for f in fits]
        fb = Resident(fits)
        b = core._Batch(fb, fits, plans, fits[0]._batch_key(plans[0]), [0, 1])
        call = core._Call(1, True, {}, False, False, False, False, baseline.option(asked))
        b.store(call, *b.read(call))
        D = len(fits[0].lower)
        assert np.array_equal(fits[0].params, np.full(D, -0.5)) and np.array_equal(fits[1].params, np.full(D, 1.0))
        if asked:
            (_, X, kw), closed = fb.calls
            assert closed == ("close",)
            assert np.array_equal(X[0], fits[0].params) and np.array_equal(X[1], fits[1].params)
            assert kw["deg"] == 2 and kw["complement"] == [True, True] and kw["return_baseline"] is False
            assert kw["intervals"] == [baseline.widened([tuple(p.bounds) for p in f.data.peaks], 3.0) for f in fits]
            assert [f.residual_baseline for f in fits] == ["row 0", "row 1"]
        else:
            assert fb.calls == [("close",)] and not any("residual_baseline" in vars(f) for f in fits)


def test_device_sigmas_of_a_replica_study_come_from_one_call(monkeypatch):
    """fit_replicas_many(device_sigma=True): every job that gives a noise_region (its own or the shared one) and no
    sigma goes into ONE sample_noise_many call on both channels; a job's own sigma keeps it out."""
    from nmrfit_amd import noise, synth
    calls = []

    def stand_in(ws, ys, regions, device=0):
        calls.append((len(ws), [tuple(r) for r in regions], device))
        return [tuple(baseline.fit_host(w, row, 2, [tuple(r)], False).sigma for row in y) for w, y, r in zip(ws, ys, regions)]
    monkeypatch.setattr(baseline, "sample_noise_many", stand_in)
    datas = []
    for k in range(3):
        sp = synth.make_spectrum(300, 2, seed=30 + k)
        datas.append(synth.SynthData(sp["w"], sp["u"], sp["v"], sp["peaks"]))
    jobs = [dict(data=datas[0]), dict(data=datas[1], sigma=0.5), dict(data=datas[2], noise_region=(3.5, 3.7))]
    got = noise._device_sigmas(jobs, dict(noise_region=(3.4, 3.6)), 2)
    assert calls == [(2, [(3.4, 3.6), (3.5, 3.7)], 2)] and sorted(got) == [0, 2]
    for m, region in ((0, (3.4, 3.6)), (2, (3.5, 3.7))):
        host = noise._job_sigma(dict(noise_region=region), datas[m])
        assert all(abs(a - b) <= 1e-9 * b for a, b in zip(got[m], host))
    assert noise._device_sigmas([dict(data=datas[0], sigma=1.0)], {}, 0) == {} and len(calls) == 1

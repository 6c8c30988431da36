"""
CPU tier of the residual statistics (nmrfit_amd/quality.py, csrc/quality.hip, include/nmrfit_amd_quality.h): the ctypes
table against the header, the library's argument checks (made before any device work), the numpy mirror of the device's
summation order against exactly summed terms, and the derived numbers of ``FitQuality`` on residuals with closed answers.
"""
import math
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

from nmrfit_amd import _cabi, quality

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 2.0 ** -52


def _declared(header):
    text = open(os.path.join(ROOT, "include", header)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return set(re.findall(r"\b(nmrfit_[a-z0-9_]+)\s*\(", text))


def test_table_and_header():
    """QUALITY_SIGNATURES is what include/nmrfit_amd_quality.h declares, the library exports it, no name is shared with
    another header or table, the product header and the ABI number are as they were."""
    names = _declared("nmrfit_amd_quality.h")
    assert names == set(_cabi.QUALITY_SIGNATURES) == {"nmrfit_quality_stats", "nmrfit_batch_quality_stats"}
    for header in sorted(os.listdir(os.path.join(ROOT, "include"))):
        if header.endswith(".h") and header != "nmrfit_amd_quality.h":
            assert not (names & _declared(header)), header
    for table in (_cabi.ALL_SIGNATURES, _cabi.PREP_SIGNATURES, _cabi.LSQ_SIGNATURES, _cabi.LSQ_IM_SIGNATURES,
                  _cabi.NOISE_SIGNATURES):
        assert not (names & set(table))
    assert len(_declared("nmrfit_amd.h")) == 46
    L = _cabi.lib()
    for n in names:
        assert hasattr(L, n), n
    assert L.nmrfit_abi_version() == _cabi.ABI_VERSION == 6
    text = open(os.path.join(ROOT, "include", "nmrfit_amd_quality.h")).read()
    assert "#define NMRFIT_QUALITY_MAX_REGIONS %d" % quality.MAX_REGIONS in text and quality.MAX_REGIONS >= 64
    assert "#define NMRFIT_QUALITY_ROW %d" % quality.ROW in text


def test_argument_validation_needs_no_gpu():
    """nmrfit_quality_stats reports every argument error of the header as NMRFIT_E_INVALID and the per-call limits as
    NMRFIT_E_UNSUPPORTED before anything touches a device; the batch call refuses a null handle."""
    L = _cabi.lib()
    p = _cabi.ptr
    K = 2
    N = np.array([4, 3], dtype=np.int64)
    w, u, v = np.arange(7.0), np.zeros(7), np.zeros(7)
    P = np.array([1, 0], dtype=np.int32)
    x = np.ones(7 + 4)
    R = np.array([1, 2], dtype=np.int32)
    edges = np.array([0.0, 1.0, -np.inf, np.inf, 2.0, 1.0])
    out = np.zeros((3 + 4) * 8)

    def call(K=K, N=N, w=w, u=u, v=v, P=P, x=x, R=R, edges=edges, out=out):
        return L.nmrfit_quality_stats(0, K, p(N), p(w), p(u), p(v), p(P), p(x), p(R), p(edges), p(out))
    for name in ("N", "w", "u", "v", "P", "x", "R", "out"):
        assert call(**{name: None}) == _cabi.E_INVALID, name
    assert call(edges=None) == _cabi.E_INVALID                                   # edges null where sum R > 0
    assert b"edges" in L.nmrfit_last_error()
    assert call(K=0) == _cabi.E_INVALID and call(K=-1) == _cabi.E_INVALID
    assert call(N=np.array([4, 0], dtype=np.int64)) == _cabi.E_INVALID
    assert call(N=np.array([-4, 3], dtype=np.int64)) == _cabi.E_INVALID
    assert call(R=np.array([1, -1], dtype=np.int32)) == _cabi.E_INVALID
    assert call(P=np.array([1, -1], dtype=np.int32)) == _cabi.E_INVALID
    bad = edges.copy()
    bad[5] = np.nan
    assert call(edges=bad) == _cabi.E_INVALID
    assert b"NaN" in L.nmrfit_last_error()
    # the limits of nmrfit_weights_build: 2^26 grid points and 65535 fits per call; the regions' cap per fit
    assert call(N=np.array([_cabi.WEIGHTS_MAX_POINTS, 1], dtype=np.int64)) == _cabi.E_UNSUPPORTED
    many = 65536
    assert L.nmrfit_quality_stats(0, many, p(np.ones(many, dtype=np.int64)), p(w), p(u), p(v), p(np.zeros(many, dtype=np.int32)),
                                  p(x), p(np.zeros(many, dtype=np.int32)), None, p(out)) == _cabi.E_UNSUPPORTED
    big = np.array([quality.MAX_REGIONS + 1, 0], dtype=np.int32)
    assert call(R=big, edges=np.zeros(2 * int(big.sum()))) == _cabi.E_UNSUPPORTED
    # an infinite edge and R = 0 everywhere with edges null are valid: what is reported then is the missing device
    # (or, on a GPU box, nothing)
    assert call() in (_cabi.OK, _cabi.E_NO_DEVICE)
    assert call(R=np.zeros(2, dtype=np.int32), edges=None) in (_cabi.OK, _cabi.E_NO_DEVICE)
    assert L.nmrfit_batch_quality_stats(None, None, p(R), p(edges), p(out)) == _cabi.E_INVALID
    assert b"null batch handle" in L.nmrfit_last_error()


# N = 700: a single point, the pairs across a wave's and a tile's start, an overlap, the whole grid, reversed edges, edges
# beyond both ends
N_MIRROR = 700
REGIONS = [(100.0, 100.2), (63.0, 64.0), (255.0, 256.0), (250.0, 300.4), (0.0, 699.0), (420.0, 380.0), (-50.0, 10.0),
           (690.0, 1.0e9)]
PAIRS = [(100, 100), (63, 64), (255, 256), (250, 300), (0, 699), (380, 420), (0, 10), (690, 699)]


def _exact_rows(e, d, fl):
    """Per row the terms of the five sums (as lists of floats), n, the maximum and its index -- no summation done."""
    j = np.arange(len(e))
    held = np.zeros(len(e), dtype=bool)
    masks = []
    for first, last in fl:
        m = (j >= first) & (j <= last)
        held |= m
        masks.append(m)
    masks += [np.ones(len(e), dtype=bool), ~held]
    rows = []
    for m in masks:
        idx = np.flatnonzero(m)
        pair = [i for i in idx if i > 0 and m[i - 1]]
        step = [float(e[i] - e[i - 1]) for i in pair]
        terms = [[float(e[i]) for i in idx], [float(e[i] * e[i]) for i in idx], [s * s for s in step],
                 [float(d[i]) for i in idx], [float(d[i] * d[i]) for i in idx]]
        a = np.abs(e[idx])
        rows.append((len(idx), terms, (float(a.max()), int(idx[a.argmax()])) if len(idx) else (0.0, -1)))
    return rows


def test_the_mirror_against_exact_arithmetic():
    """residual_stats_host gives n, the maximum and the argmax exactly and every sum within n 2^-52 sum|term| of
    math.fsum of the same (rounded) terms -- a bound that holds for any summation order."""
    rng = np.random.default_rng(11)
    w = np.arange(float(N_MIRROR))
    V = rng.standard_normal(N_MIRROR) * np.exp(rng.uniform(-8, 8, N_MIRROR))
    d = rng.standard_normal(N_MIRROR)
    fl = quality.region_indices(w, REGIONS)
    assert [tuple(r) for r in fl] == PAIRS
    rows = quality.residual_stats_host(V, d, w, REGIONS)
    assert rows.shape == (len(REGIONS) + 2, 8)
    e = V - d
    worst = 0.0
    for row, (n, terms, (top, at)) in zip(rows, _exact_rows(e, d, fl)):
        assert row[0] == n and row[6] == top and row[7] == at
        for got, t in zip(row[1:6], terms):
            bound = n * EPS * math.fsum(abs(q) for q in t)
            err = abs(got - math.fsum(t))
            assert err <= bound, (got, math.fsum(t), bound)
            worst = max(worst, err / bound if bound else 0.0)
    print("mirror against fsum: worst error / bound %.3g" % worst)
    assert rows[-1][0] == 0 and rows[-2][0] == N_MIRROR                       # (region 4 is the whole grid: nothing is left)
    # a descending grid: the regions of the reversed problem, mapped by the same argmin rule
    back = quality.region_indices(w[::-1].copy(), REGIONS)
    assert [tuple(r) for r in back] == [(N_MIRROR - 1 - b, N_MIRROR - 1 - a) for a, b in PAIRS]
    # a tie between two grid points goes to the lower index; an infinite edge: every distance is infinite, index 0
    assert [tuple(r) for r in quality.region_indices(w, [(0.5, 2.5), (np.inf, 3.0), (-np.inf, np.inf)])] == [(0, 2), (0, 3), (0, 0)]


def test_nan_and_order_of_the_mirror():
    """A NaN makes the sums of the rows that hold it NaN and never wins the maximum; -0.0 terms and an all-NaN row."""
    w = np.arange(300.0)
    V = np.zeros(300)
    d = np.linspace(-1, 1, 300)
    d[70] = np.nan
    rows = quality.residual_stats_host(V, d, w, [(60, 80), (100, 120), (70, 70)])
    assert np.isnan(rows[0][1:6]).all() and rows[0][0] == 21
    j = np.r_[60:70, 71:81]
    assert rows[0][6] == np.abs(d[j]).max() and rows[0][7] == j[np.abs(d[j]).argmax()]
    assert not np.isnan(rows[1]).any()
    assert rows[2][0] == 1 and rows[2][6] == 0.0 and rows[2][7] == -1 and np.isnan(rows[2][1]) and rows[2][3] == 0.0
    assert np.isnan(rows[3][1]) and not np.isnan(rows[4]).any()                # whole grid; the complement misses point 70


def _quality_of(e, d=None, regions=(), nparams=None):
    e = np.asarray(e, dtype=float)
    d = np.zeros_like(e) if d is None else d
    return quality.FitQuality(quality.residual_stats_host(e + d, d, np.arange(float(len(e))), list(regions)), nparams=nparams)


def test_closed_cases_of_fit_quality():
    n, c = 500, 0.375
    q = _quality_of(np.full(n, c), regions=[(10, 19)])
    assert q.rows.shape == (3, 8) and list(q.n) == [10, n, n - 10]
    assert np.all(q.bias == c) and np.all(q.rms == abs(c)) and np.all(q.durbin_watson == 0.0)
    assert list(q.max_abs) == [c] * 3 and list(q.argmax) == [10, 0, 0]
    assert len(q.regions.rows) == 1 and q.whole.n[0] == n and q.outside.n[0] == n - 10 and q.sigma_outside == abs(c)
    # e_j = c (-1)^j: every step is 2c, so DW = 4 c^2 (n - 1) / (c^2 n), exactly in fp64 for this c
    q = _quality_of(c * (-1.0) ** np.arange(n))
    assert q.whole.durbin_watson[0] == 4.0 * (n - 1) / n and q.whole.bias[0] == 0.0 and q.whole.rms[0] == c
    # an empty complement
    q = _quality_of(np.full(64, c), regions=[(0, 63)])
    assert q.outside.n[0] == 0 and q.outside.max_abs[0] == 0.0 and q.outside.argmax[0] == -1
    assert np.isnan(q.outside.rms[0]) and np.isnan(q.outside.bias[0]) and np.isnan(q.sigma_outside)
    assert np.isnan(q.chi2_reduced())
    # chi2_reduced with sigma given: sum e^2 / (sigma^2 (n - nparams)); by default sigma is the complement's rms
    q = _quality_of(np.full(n, c), regions=[(0, 9)], nparams=10)
    assert q.chi2_reduced(sigma=0.5) == n * c * c / (0.25 * (n - 10))
    assert q.chi2_reduced(sigma=0.5, nparams=0) == n * c * c / (0.25 * n)
    assert q.chi2_reduced() == n * c * c / (c * c * (n - 10))
    # r2 = 1 - sum e^2 / (sum d^2 - (sum d)^2 / n)
    d = np.arange(8.0)
    q = _quality_of(np.full(8, 0.5), d=d)
    assert q.whole.r2[0] == 1.0 - 8 * 0.25 / (np.sum(d * d) - np.sum(d) ** 2 / 8)
    assert np.isnan(_quality_of(np.ones(8)).whole.r2[0])                       # (constant data: no spread)


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="hipcc not available")
def test_kernel_resources():
    """What the compiler made of the two kernels (its own resource remarks; hipcc cross-compiles without a GPU): no
    scratch memory, no spills, at most 128 VGPRs."""
    csrc = os.path.join(ROOT, "nmrfit_amd", "csrc")
    with tempfile.TemporaryDirectory() as tmp:
        err = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=on",
                              "-fno-fast-math", "-I" + os.path.join(ROOT, "include"), "-I" + csrc, "--cuda-device-only", "-c",
                              os.path.join(csrc, "quality.hip"), "-o", os.path.join(tmp, "x.o"),
                              "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, timeout=600).stderr
    kernels, cur = {}, None
    for line in err.splitlines():
        m = re.search(r"remark: (.+?) \[-Rpass-analysis", line)
        if m:
            k, _, v = m.group(1).partition(": ")
            if k == "Function Name":
                cur = kernels.setdefault(v, {})
            elif cur is not None:
                cur[k.strip()] = v.strip()
    found = {name: r for name, r in kernels.items() if "quality_" in name}
    assert len(found) == 2 and any("quality_tiles_kernel" in n for n in found) and any("quality_fold_kernel" in n for n in found), err[-2000:]
    for name, r in found.items():
        assert int(r["ScratchSize [bytes/lane]"]) == 0 and int(r["VGPRs Spill"]) == 0 and int(r["SGPRs Spill"]) == 0, (name, r)
        assert int(r["VGPRs"]) <= 128, (name, r)


def test_fit_many_takes_the_rows_at_the_final_parameters(monkeypatch):
    """The read-back of a device batch under quality=True (no device: a stand-in holds what is resident): the fits
    that store would polish one by one after the batch has closed are polished first, the statistics are asked for at
    those final parameters with the peaks' bounds as regions, before the batch closes, and store hands each fit its
    rows.  Without the keyword nothing of this happens."""
    from nmrfit_amd import core, synth, utils

    class Resident:
        def __init__(self, fits):
            self.fits, self.calls = fits, []

        def status(self):
            return [dict(iteration=3, stop=0, fg=1.0) for _ in self.fits]

        def best(self):
            return [(np.full(len(f.lower), float(k)), 10.0 + k) for k, f in enumerate(self.fits)]

        def residual_stats(self, X, regions):
            self.calls.append(("stats", [np.array(x) for x in X], regions))
            return ["rows %d" % k for k in range(len(X))]

        def close(self):
            self.calls.append(("close",))
    monkeypatch.setattr(utils.FitUtility, "_polish", lambda self, xopt, fopt, plan: (xopt - 0.5, 0.5))
    for asked in (True, False):
        fits = []
        for k, opts in enumerate(({"polish": True}, {})):
            sp = synth.make_spectrum(256, 2, seed=90 + k)
            fits.append(utils.FitUtility(synth.SynthData(sp["w"], sp["u"], sp["v"], sp["peaks"]), list(sp["lower"]),
                                         list(sp["upper"]), summary=False, options=opts))
        plans = [f._plan() for f in fits]
        fb = Resident(fits)
        b = core._Batch(fb, fits, plans, fits[0]._batch_key(plans[0]), [0, 1])
        call = core._Call(1, True, {}, False, False, False, asked)
        assert core._Call(1, True, {}, False, False, False).quality is False
        refined, status, best, results = b.read(call)
        b.store(call, refined, status, best, results)
        D = len(fits[0].lower)
        assert np.array_equal(fits[0].params, np.full(D, -0.5)) and np.array_equal(fits[1].params, np.full(D, 1.0))
        if asked:
            (_, X, regions), closed = fb.calls
            assert closed == ("close",) and refined == {0}
            assert np.array_equal(X[0], fits[0].params) and np.array_equal(X[1], fits[1].params)
            assert regions == [[tuple(p.bounds) for p in f.data.peaks] for f in fits]
            assert [f.quality for f in fits] == ["rows 0", "rows 1"]
        else:
            assert fb.calls == [("close",)] and refined == set() and not any("quality" in vars(f) for f in fits)

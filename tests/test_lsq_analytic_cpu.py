"""
CPU tier of the analytic Jacobian (include/nmrfit_amd_lsq_analytic.h, csrc/lsq_analytic.hip): the closed forms of
tests/jac_truth.py against mpmath's own derivative of hp_truth's residual, the numpy statement lsq.jacobian_host inside
their bounds, the ABI table, the refusals that need no device, the ValueErrors of the Python layer, the compiler's
resource remarks for the new unit, and the lock-step polish over analytic normal equations against the same loop over
forward differences.
"""
import inspect
import os
import re
import subprocess
import sys

import mpmath
import numpy as np
import pytest

from nmrfit_amd import _cabi, core, lsq
from tests import hp_truth as hp
from tests import jac_truth as jt
from tests import lsq_analytic_support as A
from tests import lsq_support as S
from tests import rows_support as RS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
mp = mpmath.mp
# mpmath.diff with a step far below the narrowest scale a particle has (a width of 1e-18 just above the floor), at a
# working precision that leaves the differences 70 digits: the differentiator's own error stays below 1e-30 relative
DIFF = dict(h=mpmath.mpf(10) ** -50)
DIFF_DPS = 120
HEADER = "nmrfit_amd_lsq_analytic.h"
NAMES = {"nmrfit_jacobian_analytic", "nmrfit_batch_normal_equations_analytic"}


def small_case():
    """N = 65 (a ragged second tile), hostile weights, the hostile particles of P = 2 around two probes."""
    w, u, v = RS.make_grid("uniform", 65, seed=3)
    js = [17, 64]
    wt, _ = RS.hostile_weights(65, js, seed=4)
    return w, u, v, wt, js


def test_closed_forms_are_the_derivative_of_the_residual():
    """Every entry of jac_truth.point equals mpmath.diff of hp_truth's residual (residual_mp: hp.point's dV q) with
    respect to its parameter, to 1e-25 relative, at every hostile particle of P = 2 (and P = 0)."""
    w, u, v, wt, js = small_case()
    worst = 0.0
    with mp.workdps(DIFF_DPS):
        for j in js:
            for P in (0, 2):
                for n, x in enumerate(A.particles(w, j, P)):
                    t = jt.point(x, w, u, v, wt, j)
                    xm = [mp.mpf(float(c)) for c in x]
                    for i in range(x.size):
                        d = mp.diff(lambda z: jt.residual_mp(xm[:i] + [z] + xm[i + 1:], w, u, v, wt, j), xm[i], **DIFF)
                        ref = max(abs(d), abs(t["J"][i]))
                        gap = abs(d - t["J"][i]) / ref if ref > 0 else mp.mpf(0)
                        worst = max(worst, float(gap))
                        assert gap <= mp.mpf(10) ** -25, (j, P, n, jt.column_name(i), d, t["J"][i])
    print("closed forms against mpmath.diff: worst relative gap %.3g" % worst)


def test_slopes_are_the_derivatives_of_the_pieces():
    """Every |d piece / dt| a bound uses equals |mpmath.diff| of that piece, to 1e-25 relative, at the probed values of t
    and hostile (r, a, width)."""
    worst = 0.0
    with mp.workdps(DIFF_DPS):
        for tv in A.T_PROBES + (0.37, -2.5):
            for r, a, width in ((0.4, 1.1, 0.013), (-0.2, -0.8, -0.02), (1.3, 0.5, 1e-5), (0.0, 1.0, 0.3), (1.0, 1.0, 0.3)):
                t, ihw, rm, am = mp.mpf(tv), 2 / mp.mpf(width), mp.mpf(r), mp.mpf(a)
                sl = jt.peak_slopes(t, ihw, rm, am)
                for name in jt.PIECES:
                    d = abs(mp.diff(lambda z: jt.peak_pieces(z, ihw, rm, am)[name], t, **DIFF))
                    ref = max(d, sl[name])
                    gap = abs(d - sl[name]) / ref if ref > 0 else mp.mpf(0)
                    worst = max(worst, float(gap))
                    assert gap <= mp.mpf(10) ** -25, (tv, r, a, width, name, d, sl[name])
    print("slopes against mpmath.diff: worst relative gap %.3g" % worst)


def test_jacobian_host_is_within_the_bounds():
    w, u, v, wt, js = small_case()
    worst = {"J": hp.Worst("jacobian_host/J"), "r": hp.Worst("jacobian_host/r")}
    for j in js:
        for P in (0, 1, 2):
            for n, x in enumerate(A.particles(w, j, P)):
                J, r = lsq.jacobian_host(x, w, u, v, wt)
                assert J.shape == (w.size, x.size) and r.shape == (w.size,)
                assert np.isfinite(J).all() and np.isfinite(r).all()
                A.check_entries(worst, J[j], r[j], jt.point(x, w, u, v, wt, j), (j, P, n))
    fails = worst["J"].report() + worst["r"].report()
    assert not fails, fails[:5]


def _declared(header):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
    return set(re.findall(r"\b(nmrfit_\w+)\s*\(", text))


def test_table_and_header():
    """LSQ_ANALYTIC_SIGNATURES is what the header declares, the library exports it, no name is shared with another header
    or table, the product header and the ABI number are as they were."""
    assert _declared(HEADER) == set(_cabi.LSQ_ANALYTIC_SIGNATURES) == NAMES
    for header in sorted(os.listdir(os.path.join(ROOT, "include"))):
        if header.endswith(".h") and header != HEADER:
            assert not (NAMES & _declared(header)), header
    tables = [v for k, v in vars(_cabi).items() if k.endswith("_SIGNATURES") and k != "LSQ_ANALYTIC_SIGNATURES"]
    assert len(tables) >= 12
    for table in tables:
        assert not (NAMES & set(table))
    assert len(_declared("nmrfit_amd.h")) == 46
    L = _cabi.lib()
    for n in NAMES:
        assert hasattr(L, n), n
    assert L.nmrfit_abi_version() == _cabi.ABI_VERSION == 6
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", HEADER)).read(), flags=re.S)
    for n in NAMES:
        params = re.search(r"\b%s\s*\(([^)]*)\)" % n, text).group(1)
        assert len(params.split(",")) == len(_cabi.LSQ_ANALYTIC_SIGNATURES[n]), n


def test_argument_validation_needs_no_gpu():
    """Null handles are refused before anything touches a device."""
    L = _cabi.lib()
    x = np.ones(7)
    assert L.nmrfit_jacobian_analytic(None, 1, _cabi.ptr(x), None, None, None, None, None) == _cabi.E_INVALID
    assert L.nmrfit_batch_normal_equations_analytic(None, _cabi.ptr(x), None, None, None) == _cabi.E_INVALID


class _NoDevice:
    N = 64


def test_value_errors():
    with pytest.raises(ValueError):
        lsq.ResidualModel(_NoDevice(), jac="3-point")
    for mode in (True, "sum"):
        with pytest.raises(ValueError):
            lsq.ResidualModel(_NoDevice(), fit_im=mode, jac="analytic")
    m = lsq.ResidualModel(_NoDevice(), jac="analytic")
    assert m.jac_form == "analytic" and lsq.ResidualModel(_NoDevice()).jac_form == "2-point"
    with pytest.raises(ValueError):
        m.sandwich(np.zeros(7), 1.0, 1.0)
    with pytest.raises(ValueError):
        m.sandwich_im(np.zeros(7), 1.0, 1.0)
    with pytest.raises(ValueError):
        lsq.polish(_NoDevice(), np.zeros(7), np.zeros(7), np.ones(7), fit_im=True, channels="both", jac="analytic")
    with pytest.raises(ValueError):
        lsq.polish(_NoDevice(), np.zeros(7), np.zeros(7), np.ones(7), jac="exact")
    with pytest.raises(ValueError):
        core.fit_many([], batch_polish="both", polish_jac="analytic")
    with pytest.raises(ValueError):
        core.fit_many([], batch_polish=True, polish_jac="analytic", uncertainty=dict(sigma=1.0, channels="both"))
    with pytest.raises(ValueError):
        core.fit_many([], polish_jac="central")
    # every default is what it was
    from nmrfit_amd.batch import FitBatch
    for fn, name in ((lsq.least_squares, "jac"), (lsq.polish, "jac"), (FitBatch.normal_equations, "jac"), (FitBatch.polish, "jac"),
                     (core.fit_many, "polish_jac"), (lsq.ResidualModel.__init__, "jac")):
        assert inspect.signature(fn).parameters[name].default == "2-point", fn
    assert core._Call(1, True, {}, False, False, False).polish_jac == "2-point"


def test_fit_many_carries_polish_jac(monkeypatch):
    got = []
    monkeypatch.setattr(core, "_fit_many_local", lambda jobs, call: got.append(call.polish_jac) or [])
    core.fit_many([], batch_polish=True, polish_jac="analytic")
    core.fit_many([], batch_polish=True)
    assert got == ["analytic", "2-point"]


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="hipcc not available")
def test_new_kernels_use_no_scratch():
    """The compiler's own resource remarks for lsq_analytic.hip: both kernels without scratch memory and without scalar
    registers spilled."""
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"), "--unit", "lsq_analytic.hip"],
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-2000:]
    rows = {}
    for line in out.stdout.splitlines():
        m = re.match(r"(lsq_analytic\w*)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)", line)
        if m:
            rows[m.group(1)] = dict(vgpr=int(m.group(2)), scratch=int(m.group(4)), waves=int(m.group(5)), sgpr_spill=int(m.group(7)))
    print(out.stdout)
    assert set(rows) == {"lsq_analytic_kernel", "lsq_analytic_reduce_kernel"}, out.stdout[-2000:]
    for name, row in rows.items():
        assert row["scratch"] == 0 and row["sgpr_spill"] == 0, (name, row)
    assert rows["lsq_analytic_kernel"]["waves"] >= 2, rows


def test_polish_over_analytic_equations_ends_where_forward_differences_end():
    for P, case in zip((1, 2, 3), S.polish_cases()):
        gap, fa, fr, f0 = A.polish_gap(case)
        print("P = %d: start %.6g, analytic %.12g, forward differences %.12g, relative gap %.3g" % (P, f0, fa, fr, gap))
        assert fa < f0 and fr < f0
        assert gap <= A.FINAL_F_BAR, (P, gap, A.FINAL_F_BAR)

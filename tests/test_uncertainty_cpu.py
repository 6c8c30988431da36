"""
CPU tier of the sandwich covariance (nmrfit_amd/uncertainty.py, csrc/lsq_cov.hip, include/nmrfit_amd_cov.h): the numpy
mirror against the linear-response truth of tests/calibration_support.py, the faults the bars must catch, the D x D
algebra at its edges, the interface tables and the new kernels' resources.  No GPU.
"""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from nmrfit_amd import _cabi, lsq, uncertainty

from . import calibration_support as cs
from . import uncertainty_support as us

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_mirror_against_the_truth():
    """sandwich_host + covariance on the forward-difference Jacobian at Truth.x0 against Truth.sigma_x, Truth.af_sigma
    and Truth.cov.  The constants of uncertainty_support.MEASURED are the largest deviations printed here, per class of
    case; the bar is twice that, rounded up.  Nothing is fixed, nothing singular, and x0 is the minimiser: the Newton
    step is 1e-13 standard errors on the exact cases and 6e-6 on the noisy one."""
    worst = {}
    for name in us.EXACT_CASES + us.NOISY_CASES:
        fu = us.mirror(name)
        dev = us.deviations(name, fu)
        print("%-18s std %.3e  af %.3e  cov %.3e  distance %.2e" % (name, dev["std"], dev["af"], dev["cov"], fu.distance))
        assert fu.status == "ok" and not fu.fixed.any()
        for k, v in dev.items():
            assert v <= us.bars(name)[k], (name, k, v, us.bars(name)[k])
            worst[us.klass(name), k] = max(worst.get((us.klass(name), k), 0.0), v)
        assert fu.distance < 1e-4, (name, fu.distance)
        t = cs.truth(name)
        assert fu.area_fraction == cs.area_fraction(t.x0)
        assert np.array_equal(fu.cov, fu.cov.T) and np.allclose(np.diag(fu.correlation()), 1.0)
    print("measured:", {k: "%.3e" % v for k, v in sorted(worst.items())})
    # the constants are the measured values, rounded up in the third digit at most
    for (klass, k), v in worst.items():
        assert v <= us.MEASURED[klass][k] <= 1.02 * v, (klass, k, v, us.MEASURED[klass][k])


@pytest.mark.parametrize("fault", sorted(us.FAULTS))
def test_bar_catches_fault(fault):
    """Each fault, injected into the mirror's meat, exceeds the bar of the standard errors on its named case."""
    name, measured = us.FAULTS[fault]
    dev = us.deviations(name, us.mirror(name, fault))
    print("%-10s on %-12s std %.3e  af %.3e  cov %.3e" % (fault, name, dev["std"], dev["af"], dev["cov"]))
    assert dev["std"] > us.bars(name)["std"], (fault, dev)
    assert 0.9 * measured <= dev["std"] <= 1.1 * measured, (fault, dev["std"], measured)


def test_textbook_formula_is_not_the_covariance():
    """sigma^2 (J^T J)^-1 / N against the truth: 0.56 ... 0.66 of the true standard errors with the spectra's own weights,
    0.79 ... 1.00 with the dynamic ones -- why the meat is needed."""
    for name, lo, hi in (("n512_p2", 0.5, 0.7), ("n1024_p3_v2", 0.5, 0.7), ("user_n512_p2", 0.75, 1.01)):
        t = cs.truth(name)
        J, _ = us.jacobian_at_truth(name)
        naive = np.sqrt(np.diag(np.linalg.inv(J.T @ J)) * t.case.sigma_u ** 2 / t.case.N)
        ratio = naive / t.sigma_x
        print(name, "naive / true: %.3f ... %.3f" % (ratio.min(), ratio.max()))
        assert lo <= ratio.min() and ratio.max() <= hi


def test_parameter_on_a_bound_is_fixed():
    """A parameter placed on its bound leaves A and M: its error is 0, it is flagged, and the others' errors are those of
    the reduced problem (inverted here in raw variables by numpy)."""
    name = "n1024_p3_v2"
    t = cs.truth(name)
    c = t.case
    J, r = us.jacobian_at_truth(name)
    A, g = J.T @ J, J.T @ r
    M = uncertainty.sandwich_host(J, c.weights, t.x0, c.sigma_u, c.sigma_v)
    for i, side in ((3, "lower"), (7, "upper")):
        lower, upper = np.array(c.lower, float), np.array(c.upper, float)
        (lower if side == "lower" else upper)[i] = t.x0[i]
        fu = uncertainty.covariance(A, M, g, t.x0, lower, upper)
        keep = np.arange(c.D) != i
        assert fu.status == "ok" and fu.fixed[i] and fu.fixed.sum() == 1
        assert fu.params_std[i] == 0.0 and fu.newton_step[i] == 0.0
        assert not fu.cov[i].any() and not fu.cov[:, i].any()
        Ai = np.linalg.inv(A[np.ix_(keep, keep)])
        reduced = Ai @ M[np.ix_(keep, keep)] @ Ai
        assert np.allclose(fu.params_std[keep], np.sqrt(np.diag(reduced)), rtol=1e-7, atol=0.0)
        assert np.allclose(fu.cov[np.ix_(keep, keep)], reduced, rtol=1e-6, atol=1e-9 * np.abs(reduced).max())
        # fixing a parameter can only shrink the others' Gauss-Newton errors
        full = uncertainty.covariance(A, M, g, t.x0, c.lower, c.upper)
        assert fu.correlation()[i, i] == 1.0 and np.all(np.isfinite(fu.correlation()))
        assert full.status == "ok" and not full.fixed.any()


def test_singular_gives_nan_and_a_status():
    """A singular A (an all-zero column of J; a NaN) gives status "singular" and NaN standard errors,
    never an exception; with every parameter on a bound nothing is free."""
    name = "n512_p2"
    t = cs.truth(name)
    c = t.case
    J, r = us.jacobian_at_truth(name)
    for kind in ("zero", "nan"):
        Jb = np.array(J)
        if kind == "zero":
            Jb[:, 2] = 0.0      # (a zero pivot)
        else:
            Jb[7, 1] = np.nan
        M = uncertainty.sandwich_host(Jb, c.weights, t.x0, c.sigma_u, c.sigma_v)
        fu = uncertainty.covariance(Jb.T @ Jb, M, Jb.T @ r, t.x0, c.lower, c.upper)
        assert fu.status == "singular", kind
        assert np.isnan(fu.params_std).all() and np.isnan(fu.area_fraction_std) and np.isnan(fu.distance)
        assert np.isnan(fu.newton_step).all() and np.isfinite(fu.area_fraction)
    fu = uncertainty.covariance(J.T @ J, J.T @ J, J.T @ r, np.array(c.lower, float), c.lower, c.upper)
    assert fu.status == "singular" and fu.fixed.all() and not fu.params_std.any()


def test_area_fraction_gradient_matches_a_central_difference():
    for name in ("n512_p2", "n1024_p3_v2", "end_to_end"):
        x = cs.truth(name).x0
        grad = uncertainty.area_fraction_gradient(x)
        assert np.array_equal(grad, cs.area_fraction_gradient(x)) and uncertainty.area_fraction(x) == cs.area_fraction(x)
        num = np.zeros_like(x)
        for i in range(x.size):
            h = 1e-4 * abs(x[i]) if x[i] != 0.0 else 1e-4
            e = np.zeros_like(x)
            e[i] = h
            num[i] = (uncertainty.area_fraction(x + e) - uncertainty.area_fraction(x - e)) / (2.0 * h)
        # the area fraction is a ratio of sums of areas, T their total: a central difference with h = 1e-4 a_i <= 1e-4 T
        # has a truncation of (h / T)^2 <= 1e-8 of the gradient's size ~ 1 / T and a rounding of 2^-53 / 1e-4 ~ 1e-12 of it
        assert np.allclose(grad, num, rtol=0.0, atol=1e-7 * np.abs(grad).max()), (name, grad - num)
        assert not grad[:6].any() and not grad[7::3].any() and not grad[8::3].any()


def test_sigma_and_option_parsing():
    assert uncertainty.sigma_pair(0.5) == (0.5, 0.5) and uncertainty.sigma_pair((1.0, 2.0)) == (1.0, 2.0)
    assert uncertainty.sigma_pair(1.0, 3.0) == (1.0, 3.0)
    for bad in (-1.0, float("nan"), (1.0, 2.0, 3.0), (1.0, float("inf"))):
        with pytest.raises(ValueError):
            uncertainty.sigma_pair(bad)
    assert uncertainty.option(None) is None
    assert uncertainty.option(dict(sigma=(1.0, 2.0))) == dict(sigma=(1.0, 2.0), noise_region=None, device_sigma=False)
    for bad in (1.0, dict(sigmas=1.0)):
        with pytest.raises(ValueError):
            uncertainty.option(bad)
    # a job's own noise wins over the call's; a job with none takes the call's; none anywhere is an error
    c = cs.case("n512_p2")
    jobs = [dict(data=c.data(), sigma=(1.0, 2.0)), dict(data=c.data())]
    assert uncertainty.job_sigmas(jobs, uncertainty.option(dict(sigma=3.0))) == [(1.0, 2.0), (3.0, 3.0)]
    with pytest.raises(ValueError):
        uncertainty.job_sigmas(jobs, uncertainty.option({}))


def test_fit_many_refuses_what_the_covariance_does_not_cover():
    """fit_im jobs, more than 24 peaks and a malformed option raise ValueError before anything touches a device."""
    import nmrfit_amd
    c = cs.case("n512_p2")
    job = (c.data(), c.lower, c.upper)
    with pytest.raises(ValueError, match="real channel"):
        nmrfit_amd.fit_many([job, job], fit_im=True, uncertainty=dict(sigma=1.0))
    with pytest.raises(ValueError, match="real channel"):
        nmrfit_amd.fit_many([job, dict(data=c.data(), lower=c.lower, upper=c.upper, fit_im="sum")], uncertainty=dict(sigma=1.0))
    with pytest.raises(ValueError, match="24 peaks"):
        nmrfit_amd.fit_many([(c.data(), np.zeros(4 + 3 * 25), np.ones(4 + 3 * 25))], uncertainty=dict(sigma=1.0))
    with pytest.raises(ValueError):
        nmrfit_amd.fit_many([job], uncertainty=1.0)
    from nmrfit_amd import core
    assert core._Call._fields[-1] == "uncertainty" and core._Call._field_defaults["uncertainty"] is None


def _declared(header):
    text = open(os.path.join(ROOT, "include", header)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return set(re.findall(r"\b(nmrfit_[a-z0-9_]+)\s*\(", text))


def test_table_and_header():
    """COV_SIGNATURES is what include/nmrfit_amd_cov.h declares, the library exports it, no name is shared with another
    header or table, the product header and the ABI number are as they were."""
    names = _declared("nmrfit_amd_cov.h")
    assert names == set(_cabi.COV_SIGNATURES) == {"nmrfit_sandwich", "nmrfit_batch_sandwich"}
    for header in sorted(os.listdir(os.path.join(ROOT, "include"))):
        if header.endswith(".h") and header != "nmrfit_amd_cov.h":
            assert not (names & _declared(header)), header
    for table in (_cabi.ALL_SIGNATURES, _cabi.PREP_SIGNATURES, _cabi.LSQ_SIGNATURES, _cabi.LSQ_IM_SIGNATURES,
                  _cabi.NOISE_SIGNATURES, _cabi.QUALITY_SIGNATURES, _cabi.BASELINE_SIGNATURES):
        assert not (names & set(table))
    assert len(_declared("nmrfit_amd.h")) == 46
    L = _cabi.lib()
    for n in names:
        assert hasattr(L, n), n
    assert L.nmrfit_abi_version() == _cabi.ABI_VERSION == 6
    # the argument lists: the header's parameter count is the table's
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "nmrfit_amd_cov.h")).read(), flags=re.S)
    for n in names:
        params = re.search(r"\b%s\s*\(([^)]*)\)" % n, text).group(1)
        assert len(params.split(",")) == len(_cabi.COV_SIGNATURES[n]), n
    import nmrfit_amd
    assert nmrfit_amd.uncertainty is uncertainty and nmrfit_amd.FitUncertainty is uncertainty.FitUncertainty


def test_argument_validation_needs_no_gpu():
    """Null handles are refused before anything touches a device."""
    L = _cabi.lib()
    x = np.zeros(8)
    assert L.nmrfit_sandwich(None, 1, _cabi.ptr(x), _cabi.ptr(x), 1.0, 1.0, 1.0, None, None, None, None) == _cabi.E_INVALID
    assert L.nmrfit_batch_sandwich(None, _cabi.ptr(x), _cabi.ptr(x), _cabi.ptr(x), _cabi.ptr(x), _cabi.ptr(x), None, None,
                                   None, None) == _cabi.E_INVALID


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="hipcc not available")
def test_new_kernels_use_no_scratch():
    """The compiler's own resource remarks for lsq_cov.hip: both kernels without scratch memory or spills, the meat
    kernel at no more than the 136 VGPRs of the normal-equations kernel whose plan it follows (three waves per SIMD)."""
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"), "--unit", "lsq_cov.hip"],
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-2000:]
    rows = {}
    for line in out.stdout.splitlines():
        m = re.match(r"(lsq_meat\w*)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)", line)
        if m:
            rows[m.group(1)] = dict(vgpr=int(m.group(2)), scratch=int(m.group(4)), waves=int(m.group(5)), sgpr_spill=int(m.group(7)))
    print(out.stdout)
    assert set(rows) == {"lsq_meat_kernel", "lsq_meat_reduce_kernel"}, out.stdout[-2000:]
    for name, row in rows.items():
        assert row["scratch"] == 0 and row["sgpr_spill"] == 0, (name, row)
    assert rows["lsq_meat_kernel"]["vgpr"] <= 136 and rows["lsq_meat_kernel"]["waves"] >= 3, rows

"""
The two-channel sandwich of a ``fit_im`` fit on the CPU (nmrfit_amd/uncertainty.py ``sandwich_host_im`` /
``covariance_im``; include/nmrfit_amd_cov_im.h): the numpy mirror against an independent statement of the score's
covariance, against the linear response of lm_polish refits on both channels, against a replica study; the D x D algebra at
its edges; the options; the header, the table and the kernel's resources.  No GPU.
"""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from nmrfit_amd import _cabi, lsq, uncertainty

from . import calibration_support as cs
from . import uncertainty_im_support as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [(mode, ratio) for mode in U.MODES for ratio in U.RATIOS]


@pytest.mark.parametrize("mode,ratio", CASES)
def test_meat_is_the_covariance_of_the_score(mode, ratio):
    """M of ``covariance_im`` -- made of the three blocks and the q_ab -- equals G diag(sigma_u^2, sigma_v^2) G^T with G
    the D x 2N map from (du, dv) to d(grad f) stated from the rotation alone, to the rounding bound of
    ``meat_of_score``; for sigma_u == sigma_v the block ri is exactly zero; with the cross block left out
    (fault="no_cross", sigma_v = 2 sigma_u) the same bound is missed."""
    p = U.problem(mode, ratio)
    fu, _ = U.mirror(p.sp, p.x0, mode, p.sigma_u, p.sigma_v)
    want, bound = U.meat_of_score(U.host_pieces(p.sp, p.x0, mode), p.sp["weights"], p.x0, p.sigma_u, p.sigma_v)
    frac = float(np.max(np.abs(fu.M - want) / bound))
    print("mode %d, sigma_v / sigma_u = %g: worst |M - G S G^T| / bound %.3g" % (mode, ratio, frac))
    assert fu.status == "ok" and fu.channels == "both" and not fu.fixed.any()
    assert frac <= 1.0
    assert np.array_equal(fu.M, fu.M.T)
    if ratio == 1.0:
        assert not np.any(fu.meat[2])
    else:
        faulty, _ = U.mirror(p.sp, p.x0, mode, p.sigma_u, p.sigma_v, fault="no_cross")
        off = float(np.max(np.abs(faulty.M - want) / bound))
        shift = float(np.max(np.abs(faulty.params_std / fu.params_std - 1.0)))
        print("  no_cross: %.3g of the bound, standard errors moved by up to %.3g" % (off, shift))
        assert off > 1.0


@pytest.mark.parametrize("mode,ratio", CASES)
def test_linear_response(mode, ratio):
    """-H^-1 d(grad f) of the mirror against the central difference of lm_polish refits at data +- 0.05 n for four fixed
    noise vectors n: every parameter within twice its measured remainder (uncertainty_im_support.RESPONSE_MEASURED);
    with the derivative of 1 / rho_ch left out (fault="no_rank_one") some parameter leaves its bar."""
    got = U.response_deviation(mode, ratio)
    bar = U.response_bar(mode, ratio)
    print("mode %d, sigma_v / sigma_u = %g: |prediction - truth| / sigma_x per parameter\n  measured %s\n  recorded %s\n  bar      %s"
          % (mode, ratio, " ".join("%.3g" % v for v in got), " ".join("%.3g" % v for v in U.RESPONSE_MEASURED[(mode, ratio)]),
             " ".join("%.3g" % v for v in bar)))
    assert np.all(got <= bar)
    faulty = U.response_deviation(mode, ratio, fault="no_rank_one")
    print("  no_rank_one %s" % " ".join("%.3g" % v for v in faulty))
    assert np.any(faulty > bar)


@pytest.mark.parametrize("mode", U.MODES)
def test_replica_study(mode):
    """63 noisy copies of the base (sigma_v = 2 sigma_u, seeds REPLICA_SEED0 + k) refitted on both channels: the variance
    of every parameter over the mirror's params_std^2, and the area fraction's, inside the two-sided 1e-6 quantiles of
    chi^2_62 / 62."""
    p = U.problem(mode, 2.0)
    fu, _ = U.mirror(p.sp, p.x0, mode, p.sigma_u, p.sigma_v)
    X = U.replica_minimisers(mode)
    assert X.shape == (63, p.D) and not np.any((X <= p.lower) | (X >= p.upper))
    ratio = np.var(X, axis=0, ddof=1) / fu.params_std ** 2
    af = np.var([uncertainty.area_fraction(x) for x in X], ddof=1) / fu.area_fraction_std ** 2
    lo, hi = cs.chi2_quantiles(U.REPLICAS - 1)
    print("mode %d: var(replicas) / params_std^2 in %.3f .. %.3f, area fraction %.3f; quantiles (%.3f, %.3f)"
          % (mode, ratio.min(), ratio.max(), af, lo, hi))
    assert np.all((ratio > lo) & (ratio < hi)) and lo < af < hi


def _parts_and_meat(p):
    pieces = U.host_pieces(p.sp, p.x0, p.mode)
    (J_re, r_re, A_re, g_re, rho_re), (J_im, r_im, A_im, g_im, rho_im) = pieces
    meat = uncertainty.sandwich_host_im(J_re, r_re, J_im, r_im, p.sp["weights"], p.x0, p.sigma_u, p.sigma_v)
    return [(A_re, g_re, rho_re), (A_im, g_im, rho_im)], meat


def test_algebra_at_its_edges():
    """Fixed parameters, a channel with rho = 0 and an H that is not positive definite give the documented records
    without an exception."""
    p = U.problem(2, 2.0)
    parts, meat = _parts_and_meat(p)
    full = uncertainty.covariance_im(parts, meat, p.x0, p.lower, p.upper, sigma=(p.sigma_u, p.sigma_v))
    assert full.status == "ok" and full.rho == (parts[0][2], parts[1][2]) and full.sigma == (p.sigma_u, p.sigma_v)
    assert full.parts is not None and len(full.meat) == 3 and np.all(full.params_std > 0.0) and np.isfinite(full.distance)
    # a dict and a sequence are the same arguments
    named = uncertainty.covariance_im(dict(re=parts[0], im=parts[1]), dict(rr=meat[0], ii=meat[1], ri=meat[2]), p.x0, p.lower, p.upper)
    assert np.array_equal(named.cov, full.cov) and named.sigma is None
    # a parameter on a bound leaves H and M before the inversion
    lower = p.lower.copy()
    lower[3] = p.x0[3]
    fx = uncertainty.covariance_im(parts, meat, p.x0, lower, p.upper)
    assert fx.status == "ok" and fx.fixed[3] and fx.fixed.sum() == 1 and fx.params_std[3] == 0.0 and fx.newton_step[3] == 0.0
    assert not fx.cov[3].any() and not fx.cov[:, 3].any() and np.all(fx.params_std[~fx.fixed] > 0.0)
    free = np.ix_(~fx.fixed, ~fx.fixed)
    d = np.maximum(p.upper - lower, 1e-12)[~fx.fixed]
    Hs, Ms = fx.A[free] * np.outer(d, d), fx.M[free] * np.outer(d, d)
    direct = np.linalg.inv(Hs) @ Ms @ np.linalg.inv(Hs) * np.outer(d, d)
    sd = fx.params_std[~fx.fixed]
    # (two routes to H_ff^-1 M_ff H_ff^-1 in the scaled variables: each solve is good to ~ D cond eps of its result)
    assert np.max(np.abs(fx.cov[free] - direct) / np.outer(sd, sd)) <= 8.0 * p.D * np.linalg.cond(Hs) * U.EPS
    # a channel with rho = 0 (or a lost one) contributes nothing: the record of the other channel alone
    alone = uncertainty.covariance_im([parts[0], None], [meat[0], None, None], p.x0, p.lower, p.upper)
    for rho in (0.0, float("nan"), float("inf")):
        got = uncertainty.covariance_im([parts[0], (parts[1][0], parts[1][1], rho)], meat, p.x0, p.lower, p.upper)
        assert got.status == "ok" and np.array_equal(got.cov, alone.cov) and np.array_equal(got.newton_step, alone.newton_step)
        assert got.rho[0] == parts[0][2] and (got.rho[1] == rho or np.isnan(rho))
    assert np.isnan(alone.rho[1])
    # nothing left, or an H that is not positive definite: NaN and "singular"
    for bad in ([(parts[0][0], parts[0][1], 0.0), (parts[1][0], parts[1][1], 0.0)],
                [(-parts[0][0], parts[0][1], parts[0][2]), (-parts[1][0], parts[1][1], parts[1][2])],
                [(parts[0][0], 1e3 * np.sqrt(np.diag(parts[0][0])), parts[0][2]), None]):      # (g g^T / rho^3 outweighs A / rho)
        got = uncertainty.covariance_im(bad, meat, p.x0, p.lower, p.upper)
        assert got.status == "singular" and np.all(np.isnan(got.params_std)) and np.isnan(got.distance)
        assert np.isnan(got.area_fraction_std) and got.area_fraction == uncertainty.area_fraction(p.x0)
    with pytest.raises(ValueError, match="lacks the block"):
        uncertainty.covariance_im(parts, [meat[0], meat[1], None], p.x0, p.lower, p.upper)


def test_one_channel_is_the_real_channel_s_covariance():
    """``covariance`` on a single channel and ``covariance_im`` with the other channel absent agree at g = 0 -- to
    rounding, not to the bit: H = A / (2 rho) and M = M_JJ / (4 rho^2) carry scalars that A and M do not.  A scalar
    moves every entry of the scaled matrix by one rounding, which a Cholesky solve returns as at most ~ D cond eps of the
    solution (Higham, Accuracy and Stability, thm 10.4, constant of order D); the sandwich solves four times."""
    p = U.problem(2, 2.0)
    J, r, A, _, rho = U.host_pieces(p.sp, p.x0, 2)[0]
    zero = np.zeros(p.D)
    M = uncertainty.sandwich_host(J, p.sp["weights"], p.x0, p.sigma_u, p.sigma_v)
    meat = uncertainty.sandwich_host_im(J, r, J, r, p.sp["weights"], p.x0, p.sigma_u, p.sigma_v)
    assert np.array_equal(meat[0][:-1, :-1], M)      # (the JJ corner of Mt_rr IS the real channel's meat)
    one = uncertainty.covariance(A, M, zero, p.x0, p.lower, p.upper)
    two = uncertainty.covariance_im(dict(re=(A, zero, rho)), dict(rr=meat[0]), p.x0, p.lower, p.upper)
    d = np.maximum(p.upper - p.lower, 1e-12)
    tol = 4.0 * p.D * np.linalg.cond(A * np.outer(d, d)) * U.EPS
    dev = float(np.max(np.abs(two.cov - one.cov) / np.outer(one.params_std, one.params_std)))
    print("one channel: |cov_im - cov| / (sigma sigma) %.3g, tolerance %.3g" % (dev, tol))
    assert one.status == two.status == "ok" and dev <= tol and 0.0 < dev
    assert two.channels == "both" and not hasattr(one, "channels")


def test_options():
    """``uncertainty.option`` takes ``channels`` ("real" or "both" only) and leaves the record of every call without it
    as it was; a ``fit_im`` job without channels="both" is refused up front as ever, with it only the peak count is."""
    import nmrfit_amd
    plain = dict(sigma=(1.0, 2.0), noise_region=None, device_sigma=False)
    assert uncertainty.option(dict(sigma=(1.0, 2.0))) == plain == uncertainty.option(dict(sigma=(1.0, 2.0), channels="real"))
    assert uncertainty.option(dict(sigma=(1.0, 2.0), channels="both")) == dict(plain, channels="both")
    for bad in ("imag", "Both", None, True, 2):
        with pytest.raises(ValueError, match="channels"):
            uncertainty.option(dict(sigma=1.0, channels=bad))
    p = U.problem(2, 2.0)
    from nmrfit_amd import synth
    data = synth.SynthData(p.sp["w"], p.sp["u"], p.sp["v"], p.sp["peaks"])
    job = (data, p.lower, p.upper)
    for kw in (dict(sigma=1.0), dict(sigma=1.0, channels="real")):
        with pytest.raises(ValueError, match="real channel"):
            nmrfit_amd.fit_many([job, job], fit_im=True, uncertainty=kw)
        with pytest.raises(ValueError, match="real channel"):
            nmrfit_amd.fit_many([job, dict(data=data, lower=p.lower, upper=p.upper, fit_im="sum")], uncertainty=kw)
    with pytest.raises(ValueError, match="24 peaks"):
        nmrfit_amd.fit_many([dict(data=data, lower=np.zeros(4 + 3 * 25), upper=np.ones(4 + 3 * 25), fit_im="sum")],
                            uncertainty=dict(sigma=1.0, channels="both"))
    with pytest.raises(ValueError, match="channels"):
        nmrfit_amd.fit_many([job], fit_im=True, uncertainty=dict(sigma=1.0, channels="imag"))


def test_models_refuse_the_other_entrance():
    """A model made without a mode has no ``sandwich_im`` (and one with a mode still no ``sandwich``); FitBatch and
    FitUtility take no other ``channels``.  Nothing here touches a device."""
    class NoDevice:
        N = 16
    with pytest.raises(ValueError, match="without a fit_im mode"):
        lsq.ResidualModel(NoDevice(), fit_im=0).sandwich_im(np.zeros(7), 1.0, 1.0)
    with pytest.raises(ValueError, match="real channel"):
        lsq.ResidualModel(NoDevice(), fit_im="sum").sandwich(np.zeros(7), 1.0, 1.0)
    from nmrfit_amd.batch import FitBatch
    with pytest.raises(ValueError, match="channels"):
        FitBatch.uncertainty(object(), sigma_u=1.0, channels="imag")


def _declared(header):
    text = open(os.path.join(ROOT, "include", header)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return set(re.findall(r"\b(nmrfit_[a-z0-9_]+)\s*\(", text))


def test_table_and_header():
    """COV_IM_SIGNATURES is what include/nmrfit_amd_cov_im.h declares, the library exports it, no name is shared with
    another header or table, the product header and the ABI number are as they were."""
    names = _declared("nmrfit_amd_cov_im.h")
    assert names == set(_cabi.COV_IM_SIGNATURES) == {"nmrfit_sandwich_im", "nmrfit_batch_sandwich_im"}
    for header in sorted(os.listdir(os.path.join(ROOT, "include"))):
        if header.endswith(".h") and header != "nmrfit_amd_cov_im.h":
            assert not (names & _declared(header)), header
    for table in (_cabi.ALL_SIGNATURES, _cabi.PREP_SIGNATURES, _cabi.LSQ_SIGNATURES, _cabi.LSQ_IM_SIGNATURES,
                  _cabi.NOISE_SIGNATURES, _cabi.QUALITY_SIGNATURES, _cabi.BASELINE_SIGNATURES, _cabi.COV_SIGNATURES):
        assert not (names & set(table))
    assert len(_declared("nmrfit_amd.h")) == 46
    L = _cabi.lib()
    for n in names:
        assert hasattr(L, n), n
    assert L.nmrfit_abi_version() == _cabi.ABI_VERSION == 6
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "nmrfit_amd_cov_im.h")).read(), flags=re.S)
    for n in names:
        params = re.search(r"\b%s\s*\(([^)]*)\)" % n, text).group(1)
        assert len(params.split(",")) == len(_cabi.COV_IM_SIGNATURES[n]), n


def test_argument_validation_needs_no_gpu():
    """Null handles are refused before anything touches a device."""
    L = _cabi.lib()
    x = np.zeros(8)
    assert L.nmrfit_sandwich_im(None, 1, 2, _cabi.ptr(x), _cabi.ptr(x), 1.0, 1.0, 1.0, None, None, None, None) == _cabi.E_INVALID
    assert L.nmrfit_batch_sandwich_im(None, _cabi.ptr(x), _cabi.ptr(x), _cabi.ptr(x), _cabi.ptr(x), _cabi.ptr(x), None, None,
                                      None, None) == _cabi.E_INVALID


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="hipcc not available")
def test_new_kernels_use_no_scratch():
    """The compiler's own resource remarks for lsq_cov_im.hip: both kernels without scratch memory or spills, the meat
    kernel at three waves per SIMD like the kernels whose plan it follows."""
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"), "--unit", "lsq_cov_im.hip"],
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-2000:]
    rows = {}
    for line in out.stdout.splitlines():
        m = re.match(r"(lsq_meat_im\w*)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)", line)
        if m:
            rows[m.group(1)] = dict(vgpr=int(m.group(2)), scratch=int(m.group(4)), waves=int(m.group(5)), sgpr_spill=int(m.group(7)))
    print(out.stdout)
    assert set(rows) == {"lsq_meat_im_kernel", "lsq_meat_im_reduce_kernel"}, out.stdout[-2000:]
    for name, row in rows.items():
        assert row["scratch"] == 0 and row["sgpr_spill"] == 0, (name, row)
    assert rows["lsq_meat_im_kernel"]["waves"] >= 3, rows

"""
First-order standard errors of a fit from one Jacobian: the sandwich covariance (include/nmrfit_amd_cov.h,
csrc/lsq_cov.hip).

The fit minimises the weighted residual r_j = weights_j s (V_data,j - V_fit,j), s = 1/sqrt(N), and its weights are not
1/sigma: sigma^2 (J^T J)^-1 / N is NOT the covariance of its parameters.  With independent noise of standard deviation
sigma_u on u and sigma_v on v, V_data,j = u_j cos phi_j - v_j sin phi_j and phi_j = p0 + p1 (j / N),

    omega_j = cos^2 phi_j sigma_u^2 + sin^2 phi_j sigma_v^2        variance of V_data,j
    q_j     = (weights_j s)^2 omega_j                              variance of r_j
    M       = J^T diag(q) J                                        "the meat"
    cov     = A_ff^-1 M_ff A_ff^-1,   A = J^T J                    over the free parameters f

The device makes A, M and g = J^T r from the D + 1 residual rows of a forward-difference Jacobian
(``Evaluator.sandwich``, ``lsq.ResidualModel.sandwich``, ``FitBatch.sandwich``); ``sandwich_host`` states M in numpy, and
``covariance`` does the D x D algebra on the host -- plain numpy, against any provider of (A, M, g).

Validity.  First order in the noise, Gauss-Newton: on a spectrum the model does not fit exactly the neglected term
sum_j r_j grad^2 r_j of the Hessian is of relative size ~ noise x curvature (2e-3 of the standard errors on the noisy
calibration case, tests/uncertainty_support.py).  The standard errors describe the noise alone: ``distance`` says how
many of them the reported parameters lie from the local minimiser -- an unpolished swarm stops 0.06 ... 76 of them away
(DESIGN.md 4.11).  Real channel only: a ``fit_im`` fit minimises a mean of two norms and is refused.
"""
import numpy as np


def sigma_pair(sigma_u, sigma_v=None):
    """(sigma_u, sigma_v) as two floats, finite and >= 0; ``sigma_v`` None: ``sigma_u`` is a float for both or a pair."""
    if sigma_v is None:
        pair = (float(sigma_u),) * 2 if np.ndim(sigma_u) == 0 else tuple(float(s) for s in sigma_u)
    else:
        pair = (float(sigma_u), float(sigma_v))
    if len(pair) != 2 or not all(np.isfinite(s) and s >= 0.0 for s in pair):
        raise ValueError("uncertainty: sigma is a float or a pair (sigma_u, sigma_v), finite and >= 0, got %r" % (pair,))
    return pair


def residual_variance(weights, x, sigma_u, sigma_v):
    """q_j, the variance of the weighted residual at every grid point: (weights_j / sqrt(N))^2 omega_j with the phase of
    ``x`` (p0 = x[0], p1 = x[1])."""
    weights = np.asarray(weights, dtype=np.float64)
    N = weights.shape[0]
    phi = float(x[0]) + float(x[1]) * (np.arange(N, dtype=np.float64) / N)
    ws = weights * (1.0 / np.sqrt(N))
    return (ws * ws) * (np.cos(phi) ** 2 * (sigma_u * sigma_u) + np.sin(phi) ** 2 * (sigma_v * sigma_v))


def sandwich_host(J, weights, x, sigma_u, sigma_v):
    """What csrc/lsq_cov.hip computes, in numpy: M = J^T diag(q) J [D x D] from the Jacobian ``J`` [N x D] of the
    weighted residual, the ``weights`` [N], the parameters ``x`` (their phase) and the noise of the two channels.  The
    device's M differs in summation order and in the last bits of sincos."""
    J = np.asarray(J, dtype=np.float64)
    q = residual_variance(weights, x, sigma_u, sigma_v)
    return (q[:, None] * J).T @ J


def area_fraction(x):
    """``FitUtility.calculate_area_fraction`` from the parameter vector: the areas below their mean over all."""
    a = np.asarray(x, dtype=np.float64)[6::3]
    return float(a[a < a.mean()].sum() / a.sum())


def area_fraction_gradient(x):
    """Its gradient where the set of satellites does not change: (1[i a satellite] T - S) / T^2 on the area entries, S
    the sum of the areas below their mean and T the sum of all.  Undefined where an area EQUALS the mean: the set of
    satellites changes there and the area fraction jumps."""
    x = np.asarray(x, dtype=np.float64)
    a = x[6::3]
    sat = a < a.mean()
    S, T = a[sat].sum(), a.sum()
    grad = np.zeros_like(x)
    grad[6::3] = (sat * T - S) / (T * T)
    return grad


class FitUncertainty:
    """What ``covariance`` returns for one fit.

    cov [D, D] : A_ff^-1 M_ff A_ff^-1 on the free parameters, zero rows and columns for the fixed ones (NaN on the free
                 ones when ``status`` is "singular")
    params_std [D] : sqrt of its diagonal; 0 for a fixed parameter
    fixed [D] : bool, the parameters on a bound (x <= lower or x >= upper: what ``clip`` produces)
    correlation() : cov scaled by params_std (fixed parameters: 0, diagonal 1)
    area_fraction, area_fraction_std : the satellite area fraction at ``x`` and sqrt(grad^T cov grad); undefined where
                 an area equals the mean of the areas (``area_fraction_gradient``)
    newton_step [D] : delta = -A_ff^-1 g_f, the Gauss-Newton step to the local minimiser (0 for fixed parameters)
    distance : max_i |delta_i| / params_std_i over the free parameters -- how many standard errors ``x`` lies from the
                 local minimiser (NaN when singular; a step of exactly 0 counts as no distance, whatever the error)
    sigma : (sigma_u, sigma_v) the record was made with, or None
    status : "ok" or "singular" (the Cholesky factorisation of the scaled A_ff failed, or nothing is free)
    x, A, M, g : what it was made from
    """

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def correlation(self):
        sd = np.where(self.params_std > 0.0, self.params_std, 1.0)
        corr = self.cov / sd[:, None] / sd[None, :]
        corr[np.diag_indices_from(corr)] = 1.0
        return corr

    def __repr__(self):
        return "FitUncertainty(status=%r, area_fraction=%.6g +- %.3g, distance=%.3g)" % (
            self.status, self.area_fraction, self.area_fraction_std, self.distance)


def covariance(A, M, g, x, lower, upper, sigma=None):
    """The ``FitUncertainty`` of one fit from its D x D pieces: ``A`` = J^T J, ``M`` the meat, ``g`` = J^T r at the
    parameters ``x`` inside the box (``lower``, ``upper``).

    A parameter on a bound is fixed: its row and column leave A and M before the inversion, its standard error is 0.
    The inversion is done by Cholesky in variables scaled by max(upper - lower, 1e-12), as ``lsq.lm_polish`` scales them
    (A has a condition of ~1e6 in raw variables); a failed factorisation gives NaN and ``status == "singular"``, never an
    exception.  Plain numpy."""
    A, M = np.asarray(A, dtype=np.float64), np.asarray(M, dtype=np.float64)
    g, x = np.asarray(g, dtype=np.float64), np.asarray(x, dtype=np.float64)
    lower, upper = np.asarray(lower, dtype=np.float64), np.asarray(upper, dtype=np.float64)
    D = x.shape[0]
    fixed = (x <= lower) | (x >= upper)
    free = ~fixed
    cov = np.zeros((D, D))
    step = np.zeros(D)
    status = "ok"
    ix = np.ix_(free, free)
    d = np.maximum(upper - lower, 1e-12)[free]
    L = None
    if free.any() and np.all(np.isfinite(A[ix])) and np.all(np.isfinite(M[ix])) and np.all(np.isfinite(g[free])):
        try:
            L = np.linalg.cholesky(A[ix] * d[:, None] * d[None, :])
        except np.linalg.LinAlgError:
            L = None
    if L is None:
        status = "singular"
        cov[ix] = np.nan
        step[free] = np.nan
    else:
        def solve(B):      # (A_s)^-1 B through the factor
            return np.linalg.solve(L.T, np.linalg.solve(L, B))
        Ms = M[ix] * d[:, None] * d[None, :]
        Cs = solve(solve(Ms).T)                       # A_s^-1 M_s A_s^-1 (M_s symmetric)
        cov[ix] = 0.5 * (Cs + Cs.T) * np.outer(d, d)      # (symmetric to the bit)
        step[free] = -solve(g[free] * d) * d
    var = np.diag(cov).copy()
    std = np.sqrt(np.where(var > 0.0, var, 0.0))
    std[np.isnan(var)] = np.nan
    grad = area_fraction_gradient(x)
    with np.errstate(invalid="ignore", divide="ignore"):
        af_var = float(grad @ cov @ grad)
        ratio = np.abs(step[free]) / std[free]
    ratio = np.where(step[free] == 0.0, 0.0, ratio)      # (0 / 0: a step of zero is no distance)
    distance = float(np.max(ratio)) if ratio.size and status == "ok" else float("nan")
    return FitUncertainty(cov=cov, params_std=std, fixed=fixed, area_fraction=area_fraction(x),
                          area_fraction_std=float(np.sqrt(af_var)) if af_var >= 0.0 else float("nan"),
                          newton_step=step, distance=distance, sigma=None if sigma is None else tuple(sigma),
                          status=status, x=x, A=A, M=M, g=g)


def option(uncertainty):
    """``fit_many``'s ``uncertainty=`` as its record keeps it: None, or a dict with ``sigma`` (a float or a pair) or
    ``noise_region=(xstart, xstop)`` -- neither: every job must bring its own -- and ``device_sigma`` (bool)."""
    if uncertainty is None or uncertainty is False:
        return None
    if not isinstance(uncertainty, dict):
        raise ValueError("fit_many: uncertainty is a dict with sigma (a float or a pair) or noise_region=(xstart, xstop)")
    unknown = set(uncertainty) - {"sigma", "noise_region", "device_sigma"}
    if unknown:
        raise ValueError("fit_many: uncertainty has no option %s" % ", ".join(sorted(map(repr, unknown))))
    return dict(sigma=uncertainty.get("sigma"), noise_region=uncertainty.get("noise_region"),
                device_sigma=bool(uncertainty.get("device_sigma", False)))


def job_sigmas(jobs, opts, device=0):
    """(sigma_u, sigma_v) of every job of a ``fit_many(uncertainty=opts)`` call: a job's own ``sigma`` /
    ``noise_region`` wins over the call's, with exactly the meaning they have in ``fit_replicas_many``
    (``noise._job_sigma``; ``device_sigma``: ``noise._device_sigmas``)."""
    from . import noise
    shared = dict(sigma=opts["sigma"], noise_region=opts["noise_region"])
    found = noise._device_sigmas(jobs, shared, device) if opts["device_sigma"] else {}
    out = []
    for m, job in enumerate(jobs):
        own = job.get("sigma") is not None or job.get("noise_region") is not None
        out.append(found[m] if m in found else noise._job_sigma(job if own else shared, job["data"]))
    return out

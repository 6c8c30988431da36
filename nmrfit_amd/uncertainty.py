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
(DESIGN.md 4.11).  Real channel only: a ``fit_im`` fit minimises a mean of two norms and is refused here -- its entrance
is the two-channel sandwich below.

Both channels (include/nmrfit_amd_cov_im.h, csrc/lsq_cov_im.hip).  A ``fit_im`` fit minimises
f = (rho_re + rho_im)/2, rho_ch = ||r_ch||.  Its estimator solves grad f = sum_ch J_ch^T r_ch / (2 rho_ch) = 0, and with J
held fixed the score moves with the data by

    d(grad f) = 1/2 sum_ch (1/rho_ch) B_ch Jt_ch^T dr_ch,     Jt_ch = [J_ch | r_ch]  [N x (D + 1)],  B_ch = [I_D | -g_ch/rho_ch^2]
    H   = 1/2 sum_ch (A_ch/rho_ch - g_ch g_ch^T/rho_ch^3)      the Gauss-Newton Hessian of f (not combine_channels' dominating H)
    M   = 1/4 sum_a sum_b B_a Mt_ab B_b^T / (rho_a rho_b),     Mt_ab = Jt_a^T diag(q_ab) Jt_b
    cov = H_ff^-1 M_ff H_ff^-1

with q_rr = ws^2 (cos^2 phi sigma_u^2 + sin^2 phi sigma_v^2), q_ii = ws^2 (sin^2 phi sigma_u^2 + cos^2 phi sigma_v^2) and
q_ri = ws^2 cos phi sin phi (sigma_u^2 - sigma_v^2), ws_j = weights_j s: V and I are two rotations of the same (u, v).  The
device makes the three blocks Mt_rr, Mt_ii, Mt_ri next to A_ch, g_ch, rho_ch (``Evaluator.sandwich_im``,
``lsq.ResidualModel.sandwich_im``, ``FitBatch.sandwich_im``); ``sandwich_host_im`` states them in numpy and
``covariance_im`` does the algebra.  The errors belong to the minimiser of f: ``distance`` is measured with grad f, and
``batch_polish="both"`` / ``FitBatch.polish(channels="both")`` is the polish that reaches that minimiser.
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


def residual_covariances(weights, x, sigma_u, sigma_v):
    """``(q_rr, q_ii, q_ri)`` [N each]: per grid point the variances of the weighted residuals of the real and the
    imaginary channel and their covariance, with the phase of ``x``."""
    weights = np.asarray(weights, dtype=np.float64)
    N = weights.shape[0]
    phi = float(x[0]) + float(x[1]) * (np.arange(N, dtype=np.float64) / N)
    ws = weights * (1.0 / np.sqrt(N))
    cs, sn = np.cos(phi), np.sin(phi)
    var_u, var_v = sigma_u * sigma_u, sigma_v * sigma_v
    return ((ws * ws) * (cs * cs * var_u + sn * sn * var_v), (ws * ws) * (sn * sn * var_u + cs * cs * var_v),
            (ws * ws) * (cs * sn * (var_u - var_v)))


def sandwich_host_im(J_re, r_re, J_im, r_im, weights, x, sigma_u, sigma_v):
    """What csrc/lsq_cov_im.hip computes, in numpy: ``(Mt_rr, Mt_ii, Mt_ri)``, [(D + 1) x (D + 1)] each, with
    Mt_ab = Jt_a^T diag(q_ab) Jt_b and Jt_ch = [J_ch | r_ch] -- the Jacobian [N x D] and the residual [N] of either
    channel's weighted residual.  The device's blocks differ in summation order and in the last bits of sincos."""
    Jt = [np.column_stack((np.asarray(J, dtype=np.float64), np.asarray(r, dtype=np.float64))) for J, r in ((J_re, r_re), (J_im, r_im))]
    q_rr, q_ii, q_ri = residual_covariances(weights, x, sigma_u, sigma_v)
    return (q_rr[:, None] * Jt[0]).T @ Jt[0], (q_ii[:, None] * Jt[1]).T @ Jt[1], (q_ri[:, None] * Jt[0]).T @ Jt[1]


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

    A record made by ``covariance_im`` (a fit on both channels) has A = H, the Gauss-Newton Hessian of
    f = (rho_re + rho_im)/2, M the meat of its score and g = grad f, and carries four attributes more -- a real-channel
    record has none of them:
    channels : "both"
    rho : (rho_re, rho_im), NaN for an absent channel
    parts : the channels' (A_ch, g_ch, rho_ch) it was made from, (re, im), None for an absent channel
    meat : the blocks (Mt_rr, Mt_ii, Mt_ri) it was made from
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


def _channels(parts, meat):
    """``covariance_im``'s arguments as two lists: [(A, g, rho) or None] for (re, im) and the 2 x 2 table of blocks."""
    if isinstance(parts, dict):
        parts = [parts.get("re"), parts.get("im")]
    parts = list(parts)
    if isinstance(meat, dict):
        meat = [meat.get("rr"), meat.get("ii"), meat.get("ri")]
    rr, ii, ri = (None if m is None else np.asarray(m, dtype=np.float64) for m in meat)
    return parts, [[rr, ri], [None if ri is None else ri.T, ii]]


def covariance_im(parts, meat, x, lower, upper, sigma=None):
    """The ``FitUncertainty`` of one fit made on both channels, from its pieces: ``parts`` the channels' normal equations
    (a dict with "re" and / or "im", or the pair (re, im) with None for an absent channel, of ``(A_ch, g_ch, rho_ch)`` as
    ``lsq.combine_channels`` takes them) and ``meat`` the blocks ``(Mt_rr, Mt_ii, Mt_ri)`` (or a dict with "rr", "ii",
    "ri"; the blocks of an absent channel may be None) at the parameters ``x`` inside the box.

    H, M and the gradient of f = (rho_re + rho_im)/2 are formed as the module's docstring states them; a channel whose rho
    is 0 or not finite contributes nothing to any of them, as in ``combine_channels``.  Fixed parameters, the scaling,
    the Cholesky factorisation and the record are ``covariance``'s: H is not guaranteed positive definite, and a failed
    factorisation gives NaN and ``status == "singular"``, never an exception.  The record carries ``A`` = H, ``M`` = M,
    ``g`` = grad f, ``rho`` = (rho_re, rho_im) (NaN for an absent channel), ``channels`` = "both", and the pieces it
    was made from as ``parts`` and ``meat``.  ``newton_step`` is -H_ff^-1 grad f_f: the errors and ``distance`` belong to
    the minimiser of f.  Plain numpy."""
    x = np.asarray(x, dtype=np.float64)
    D = x.shape[0]
    parts, blocks = _channels(parts, meat)
    H, M, grad = np.zeros((D, D)), np.zeros((D, D)), np.zeros(D)
    rho, B = [float("nan")] * 2, [None] * 2
    for ch, part in enumerate(parts):
        if part is None:
            continue
        A, g, r = np.asarray(part[0], dtype=np.float64), np.asarray(part[1], dtype=np.float64), float(part[2])
        rho[ch] = r
        if not (np.isfinite(r) and r > 0.0):
            continue
        H += 0.5 * (A / r - np.outer(g, g) / (r * r * r))
        grad += g * (0.5 / r)
        B[ch] = np.column_stack((np.eye(D), -g / (r * r))) / r        # B_ch / rho_ch
    for a in (0, 1):
        for b in (0, 1):
            if B[a] is not None and B[b] is not None:
                if blocks[a][b] is None:
                    raise ValueError("covariance_im: the meat lacks the block of channels (%d, %d)" % (a, b))
                M += 0.25 * (B[a] @ blocks[a][b] @ B[b].T)
    M = 0.5 * (M + M.T)
    fu = covariance(H, M, grad, x, lower, upper, sigma=sigma)
    fu.rho, fu.channels, fu.parts, fu.meat = tuple(rho), "both", parts, meat
    return fu


def option(uncertainty):
    """``fit_many``'s ``uncertainty=`` as its record keeps it: None, or a dict with ``sigma`` (a float or a pair) or
    ``noise_region=(xstart, xstop)`` -- neither: every job must bring its own -- and ``device_sigma`` (bool).
    ``channels="both"`` (the default "real" leaves the dict as it always was): the ``fit_im`` jobs of the call get the
    two-channel record (``covariance_im``) instead of being refused."""
    if uncertainty is None or uncertainty is False:
        return None
    if not isinstance(uncertainty, dict):
        raise ValueError("fit_many: uncertainty is a dict with sigma (a float or a pair) or noise_region=(xstart, xstop)")
    unknown = set(uncertainty) - {"sigma", "noise_region", "device_sigma", "channels"}
    if unknown:
        raise ValueError("fit_many: uncertainty has no option %s" % ", ".join(sorted(map(repr, unknown))))
    channels = uncertainty.get("channels", "real")
    if not isinstance(channels, str) or channels not in ("real", "both"):
        raise ValueError('fit_many: uncertainty channels is "real" or "both", got %r' % (channels,))
    out = dict(sigma=uncertainty.get("sigma"), noise_region=uncertainty.get("noise_region"),
               device_sigma=bool(uncertainty.get("device_sigma", False)))
    if channels == "both":
        out["channels"] = "both"
    return out


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

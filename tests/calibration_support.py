"""
Shared by tests/test_calibration_cpu.py and tests/test_gpu_calibration.py (and the end-to-end tests of
tests/test_gpu_noise.py): the linear response of a least-squares fit to the noise of its own replica.

A base spectrum that the model fits exactly (``synth.make_spectrum(..., noise=0.0, physical=True)``) has the weighted
residual r(x; u, v) = weights (V_data - V_fit)/sqrt(N) equal to 0 at its minimiser x0.  The minimiser of the replica
(u_k, v_k) = (u + sigma_u z_u, v + sigma_v z_v) then is

    x_k - x0 = D_lin,k + O(sigma^2),      D_lin,k = -(J^T J)^-1 J^T dr_k,      dr_k = r(x0; u_k, v_k) - r(x0; u, v)

with J the derivative of r at x0 (Gauss-Newton: the term sum r_j grad^2 r_j of the full Hessian is itself of the order
of sigma, because r(x0) = 0).  The deviates of every replica are known (``noise.normals`` is the numpy statement of the
device's), so this is a prediction per replica and per parameter, not a statistic; spreads, area fractions and residual
sums follow from it.

The host truth here uses ``oracle.nmrfit_oracle.residual``, numpy and scipy, and of the package only ``synth`` and
``noise.replicas_host`` / ``noise.normals``.
"""
import functools

import numpy as np

from nmrfit_amd import noise, synth
from oracle import nmrfit_oracle as O

# -- the bar ---------------------------------------------------------------------------------------------------------
# The worst |D_k - D_lin,k| / sigma_x of scipy TRF refits (tolerances 1e-15, central-difference Jacobian) over every
# replica and parameter of cases() on the CPU, per noise level (tests/test_calibration_cpu.py::test_reference_within_bar
# prints them): the second-order remainder of the prediction.  It scales with sigma.
# Keys: (sigma_u / max|u|, sigma_v / sigma_u, "exact" or "noisy" base).
REMAINDER_MEASURED = {(1e-3, 1.0, "exact"): 0.04895, (1e-3, 2.0, "exact"): 0.3026, (1e-4, 1.0, "exact"): 0.002841,
                      (1e-3, 1.0, "noisy"): 0.01168}
# The same for the residual sums of the unit-weight twins: the worst |RSS(TRF refit) - RSS_k| / RSS_k.
RSS_REMAINDER_MEASURED = 2.770e-4
# The polish stops on a relative decrease of f below FTOL.  Near the minimiser f^2 = f*^2 + |J d|^2 with d the distance
# left, and f*^2 is at most sigma^2 mean(weights^2) -- in the metric of sigma_x, whose covariance is (J^T J)^-1 sigma^2 /N
# for white noise, a relative decrease eps of f is |d|^2 / sigma_x^2 <= 2 N eps.
FTOL = 1e-12
N_MAX = 1024


def stopping_distance(N, ftol=FTOL):
    return float(np.sqrt(2.0 * N * ftol))


def twice_rounded_up(x):
    """2 x, rounded up to two digits."""
    digits = 10.0 ** (np.floor(np.log10(2.0 * x)) - 1)
    return float(np.ceil(2.0 * x / digits - 1e-9) * digits)


def bar(c):
    """What |D_k - D_lin,k| / sigma_x may be on case ``c``: twice the measured remainder of the reference at its noise,
    rounded up, and the stopping distance of the polish."""
    return twice_rounded_up(REMAINDER_MEASURED[c.key]) + stopping_distance(c.N)


def rss_bar():
    return twice_rounded_up(RSS_REMAINDER_MEASURED) + 2.0 * FTOL


USER_REPLICAS, USER_SEED = 12, (1 << 33) + 77


# -- the problems ----------------------------------------------------------------------------------------------------
class Case:
    """One problem: the noiseless spectrum, its weights, and M noisy copies.

    name, N, P, M : the spectrum is ``synth.make_spectrum(N, P, seed=spec_seed, noise=base_noise, physical=True)``
    weights : "own" (the spectrum's), "unit" (the twin with unit weights) or "dynamic" (what ``fit`` builds from the
              peaks: ``oracle.compute_weights(w, peaks, 0.5)``)
    base_noise : 0.0 -- the model fits the base exactly -- or the noise of the base spectrum itself; the prediction then
              takes the full Hessian (``Truth``)
    level, ratio : sigma_u = level max|u| (a noisy base: the base's own sigma, level max V), sigma_v = ratio sigma_u
    seed0 : the noise seed of copy k (1 .. M) is seed0 + k (seed0 itself is fit 0's, the unperturbed data)
    """

    def __init__(self, name, N, P, M, weights="own", level=1e-3, ratio=1.0, seed0=100, spec_seed=5, base_noise=0.0):
        self.name, self.N, self.P, self.M, self.level, self.ratio, self.seed0 = name, N, P, M, level, ratio, seed0
        self.unit, self.exact = weights == "unit", base_noise == 0.0
        self.key = (level, ratio, "exact" if self.exact else "noisy")
        sp = synth.make_spectrum(N, P, seed=spec_seed, noise=base_noise, physical=True)
        self.spec = sp
        self.w, self.u, self.v = sp["w"], sp["u"], sp["v"]
        self.weights = {"own": lambda: sp["weights"], "unit": lambda: np.ones(N),
                        "dynamic": lambda: O.compute_weights(sp["w"], sp["peaks"], 0.5)}[weights]()
        self.lower, self.upper, self.x_true = sp["lower"], sp["upper"], sp["x_true"]
        self.D = 4 + 3 * P
        # (a noisy base is test_end_to_end's: its replicas take the base's own sigma, as that test does)
        self.sigma_u = level * float(np.max(np.abs(self.u))) if self.exact else float(sp["sigma"])
        self.sigma_v = ratio * self.sigma_u
        self.seeds = [seed0 + k for k in range(M + 1)]

    def spectrum_tuple(self):
        return self.w, self.u, self.v, self.weights

    def data(self):
        return synth.SynthData(self.w, self.u, self.v, self.spec["peaks"])


@functools.lru_cache(maxsize=None)
def cases():
    """The case list (built once, read-only).  The two device problems of the issue, a twin of each with unit weights,
    sigma_v = 2 sigma_u on one, seeds beyond 2^32; a short study at a tenth of the noise for the faults whose size is
    1/(2M); the two jobs of the user-level test, with the weights ``fit`` builds and the seeds ``fit_replicas_many``
    documents (seed + m (replicas + 1) + k); and the spectrum and seeds of tests/test_gpu_noise.py::test_end_to_end,
    whose base is noisy."""
    return (Case("n512_p2", 512, 2, 199, seed0=100),
            Case("n512_p2_unit", 512, 2, 199, weights="unit", seed0=(1 << 32) + 7000),
            Case("n1024_p3_v2", 1024, 3, 63, ratio=2.0, seed0=3000),
            Case("n1024_p3_unit", 1024, 3, 63, weights="unit", seed0=5000),
            Case("n512_p2_fine", 512, 2, 8, level=1e-4, seed0=900),
            Case("user_n512_p2", 512, 2, USER_REPLICAS, weights="dynamic", seed0=USER_SEED),
            Case("user_n1024_p3_v2", 1024, 3, USER_REPLICAS, weights="dynamic", ratio=2.0, seed0=USER_SEED + USER_REPLICAS + 1),
            Case("end_to_end", 1024, 2, 8, weights="dynamic", seed0=11, spec_seed=1, base_noise=1e-3))


def case(name):
    return {c.name: c for c in cases()}[name]


# -- the replica maker, and its faults ---------------------------------------------------------------------------------
FAULTS = ("variance", "sqrt2", "tied", "one_seed", "swapped")


def make_replicas(c, fault=None):
    """The M noisy copies of case ``c`` as the library documents them -- ``noise.replicas_host`` with (sigma_u, sigma_v)
    and seed0 + k -- or with one fault injected: sigma applied as a variance, sigma off by sqrt(2), z_v = z_u, one seed
    for every copy, sigma_u and sigma_v swapped."""
    su, sv = c.sigma_u, c.sigma_v
    seeds = c.seeds[1:]
    if fault is None:
        return noise.replicas_host([c.u] * c.M, [c.v] * c.M, su, sv, seeds)
    if fault == "variance":
        return noise.replicas_host([c.u] * c.M, [c.v] * c.M, su * su, sv * sv, seeds)
    if fault == "sqrt2":
        return noise.replicas_host([c.u] * c.M, [c.v] * c.M, np.sqrt(2.0) * su, np.sqrt(2.0) * sv, seeds)
    if fault == "swapped":
        return noise.replicas_host([c.u] * c.M, [c.v] * c.M, sv, su, seeds)
    if fault == "one_seed":
        return noise.replicas_host([c.u] * c.M, [c.v] * c.M, su, sv, [seeds[0]] * c.M)
    if fault == "tied":
        out = []
        for s in seeds:
            zu, _ = noise.normals(s, c.N)
            out.append((c.u + su * zu, c.v + sv * zu))
        return out
    raise ValueError(fault)


# -- the host truth ----------------------------------------------------------------------------------------------------
def residual(c, x, u=None, v=None):
    """r(x; u, v) = weights (V_data - V_fit) / sqrt(N), as lsq.py scales it."""
    return O.residual(np.asarray(x, dtype=np.float64), c.w, c.u if u is None else u, c.v if v is None else v, c.weights) / np.sqrt(c.N)


def central_steps(c):
    """The steps of the central differences: 1e-4 of the box.  The truncation is (h / scale)^2 / 6 of a derivative's
    size, 2e-9, the rounding 2^-53 / 1e-4."""
    return 1e-4 * (np.asarray(c.upper) - np.asarray(c.lower))


def central_jacobian(c, x, u=None, v=None):
    h = central_steps(c)
    J = np.empty((c.N, c.D))
    for i in range(c.D):
        e = np.zeros(c.D)
        e[i] = h[i]
        J[:, i] = (residual(c, x + e, u, v) - residual(c, x - e, u, v)) / (2.0 * h[i])
    return J


def second_differences(c, x):
    """d^2 r / dx_i^2 at x by central second differences, [N x D]: what the forward step's truncation is made of."""
    h = 1e-3 * (np.asarray(c.upper) - np.asarray(c.lower))
    r0 = residual(c, x)
    S = np.empty((c.N, c.D))
    for i in range(c.D):
        e = np.zeros(c.D)
        e[i] = h[i]
        S[:, i] = (residual(c, x + e) - 2.0 * r0 + residual(c, x - e)) / (h[i] * h[i])
    return S


def trf(c, x0, u=None, v=None):
    """The least-squares minimiser of r(.; u, v) in the box by scipy's TRF at tolerances 1e-15 from ``x0``."""
    from scipy.optimize import least_squares
    lo, hi = np.asarray(c.lower, float), np.asarray(c.upper, float)
    res = least_squares(lambda x: residual(c, x, u, v), np.clip(x0, lo, hi), jac=lambda x: central_jacobian(c, x, u, v),
                        bounds=(lo, hi), method="trf", x_scale=np.maximum(hi - lo, 1e-12), ftol=1e-15, xtol=1e-15, gtol=1e-15)
    return res.x


def area_fraction(x):
    """What ``FitUtility.calculate_area_fraction`` computes from the parameters: the areas below their mean over all."""
    a = np.asarray(x, dtype=np.float64)[6::3]
    return float(a[a < a.mean()].sum() / a.sum())


def area_fraction_gradient(x):
    """Its gradient where the set of satellites does not change: d/da_i [S / T] = (1[i a satellite] T - S) / T^2."""
    x = np.asarray(x, dtype=np.float64)
    a = x[6::3]
    sat = a < a.mean()
    S, T = a[sat].sum(), a.sum()
    g = np.zeros_like(x)
    g[6::3] = (sat * T - S) / (T * T)
    return g


class Truth:
    """The host truth of one case.

    x0 : the base fit (TRF from x_true); J [N x D] at x0 by central differences; A = J^T J
    H : A where the model fits the base exactly; else the full Hessian of |r|^2 / 2 at x0, A + sum_j r_j grad^2 r_j, by
        central differences of the gradient J(x)^T r(x) -- the second term is of the order of the base's noise, as large
        as the replica's.  The prediction is then the Newton step D_lin,k = -H^-1 grad_k with grad_k = J_k^T r_k the
        gradient of the REPLICA's objective at x0 (its own central-difference Jacobian); for an exact base that is
        -(J^T J)^-1 J^T dr_k up to second order.
    var : the variance of every point of dr, weights^2 (cos^2 phi sigma_u^2 + sin^2 phi sigma_v^2) / N
          (V_data = u cos phi - v sin phi, phi_j = p0 + p1 j / N); weights^2 sigma^2 / N where sigma_u = sigma_v
    cov : the sandwich (J^T J)^-1 J^T diag(var) J (J^T J)^-1; sigma_x its diagonal's root
    af0, af_grad, af_sigma : the area fraction at x0, its gradient, sqrt(grad^T cov grad)
    """

    def __init__(self, c):
        self.case = c
        self.x0 = trf(c, c.x_true)
        self.J = central_jacobian(c, self.x0)
        self.A = self.J.T @ self.J
        self.r0 = residual(c, self.x0)
        self.H = self.A if c.exact else self._full_hessian()
        self.Ainv = np.linalg.inv(self.H)
        self.pinv = -self.Ainv @ self.J.T                                     # D_lin = pinv dr
        phi = self.x0[0] + self.x0[1] * np.arange(c.N) / c.N
        self.var = c.weights ** 2 * (np.cos(phi) ** 2 * c.sigma_u ** 2 + np.sin(phi) ** 2 * c.sigma_v ** 2) / c.N
        self.cov = self.pinv @ (self.var[:, None] * self.pinv.T)
        self.sigma_x = np.sqrt(np.diag(self.cov))
        self.af0 = area_fraction(self.x0)
        self.af_grad = area_fraction_gradient(self.x0)
        self.af_sigma = float(np.sqrt(self.af_grad @ self.cov @ self.af_grad))

    def _full_hessian(self):
        c, h = self.case, central_steps(self.case)
        H = np.empty((c.D, c.D))
        for i in range(c.D):
            e = np.zeros(c.D)
            e[i] = h[i]
            gp = central_jacobian(c, self.x0 + e).T @ residual(c, self.x0 + e)
            gm = central_jacobian(c, self.x0 - e).T @ residual(c, self.x0 - e)
            H[:, i] = (gp - gm) / (2.0 * h[i])
        return 0.5 * (H + H.T)

    def dr(self, uv):
        """dr_k of the replicas' actual arrays, [M x N]."""
        return np.array([residual(self.case, self.x0, u, v) - self.r0 for u, v in uv])

    def linear(self, uv):
        """D_lin,k of the replicas ``uv`` (a list of (u_k, v_k)), [M x D]."""
        if self.case.exact:
            return self.dr(uv) @ self.pinv.T
        c = self.case
        return np.array([-self.Ainv @ (central_jacobian(c, self.x0, u, v).T @ residual(c, self.x0, u, v)) for u, v in uv])

    def rss(self, uv):
        """The whole-grid sum of squares of V_fit - V_data at the replica's minimiser, to first order:
        N |dr_k + J D_lin,k|^2 (unit weights: r = (V_data - V_fit) / sqrt(N))."""
        dr = self.dr(uv)
        return self.case.N * np.sum((dr + (dr @ self.pinv.T) @ self.J.T) ** 2, axis=1)

    def refit(self, uv):
        """x_k - x0 by TRF on every replica, from x0: [M x D]."""
        return np.array([trf(self.case, self.x0, u, v) for u, v in uv]) - self.x0


@functools.lru_cache(maxsize=None)
def truth(name):
    """The Truth of case ``name`` with ``replicas`` (the documented copies) and ``lin`` (their D_lin), computed once."""
    t = Truth(case(name))
    t.replicas = make_replicas(t.case)
    t.lin = t.linear(t.replicas)
    t.lin.setflags(write=False)
    return t


# -- the checks ----------------------------------------------------------------------------------------------------
def pointwise(t, delta, lin=None):
    """|D_k - D_lin,k| / sigma_x, [M x D]."""
    return np.abs(np.asarray(delta) - (t.lin if lin is None else lin)) / t.sigma_x


def spread_tolerance(b, M):
    """What the sample standard deviation (ddof 1) of M values may differ by from that of their predictions, in units of
    sigma_x, when every value is within b sigma_x of its prediction: the centred vectors differ by at most sqrt(M) b in
    norm, and the standard deviation is that norm over sqrt(M - 1)."""
    return b * np.sqrt(M / (M - 1.0))


def chi2_quantiles(dof, q=1e-6):
    """The two-sided q quantiles of chi^2_dof / dof."""
    from scipy.stats import chi2
    return chi2.ppf(q, dof) / dof, chi2.isf(q, dof) / dof

"""
Least-squares backend on top of the batched residual kernel (BASELINE.json config 5, SURVEY.md
section 8 row f2).  The reference has no such backend -- its "least-squares fit" is the swarm
minimising the RMSE (README.md:3, nmrfit/utils.py:176) -- so this is a build-defined extension
that reuses the hot path: one ``nmrfit_residual_batch`` launch returns the residual vectors of
the D+1 parameter rows a forward-difference Jacobian needs.

    fun(x) = weights*(V_data - V_fit) / sqrt(N)        so that ||fun(x)||_2 == objective(x)
    jac(x) = [fun(x + h_i e_i) - fun(x)] / h_i         D+1 rows, one launch

``least_squares`` hands both to scipy.optimize.least_squares (trust-region reflective, box
bounds); ``polish`` refines a swarm result.  scipy runs on the host; every residual and
Jacobian column comes from the GPU.

The Jacobian is formed on the device (``nmrfit_jacobian``, csrc/lsq.hip): the D + 1 residual rows never
leave it, J arrives in the N x D layout scipy takes, bit for bit the expression above.  The same kernel
reduces the normal equations A = J^T J, g = J^T fun there (``ResidualModel.normal_equations``; for every fit
of a device batch in one go: ``FitBatch.normal_equations``), D^2 + D doubles per fit instead of N D.
``lm_polish`` is the small host loop over such D x D systems that refines K fits in lock step
(``FitBatch.polish``, ``fit_many(batch_polish=True)``); ``normal_equations_host`` states the same quantities
in numpy.

Both channels (``nmrfit_jacobian_im``, include/nmrfit_amd_lsq_im.h).  A fit made with ``fit_im`` minimises
f = (rho_re + rho_im)/2, the mean of the two channels' RMSEs (equations.py:205-209) -- a mean of two norms, not a sum of
squares.  The device returns, per channel, the residual rows, J, r, A = J^T J, g = J^T r and rho; ``combine_channels``
makes of them the gradient of f in the forward-difference model and a positive semi-definite matrix that dominates its
Gauss-Newton Hessian, the ``(H, grad f, f)`` that ``lm_polish`` takes as it is.  ``ResidualModel(..., fit_im=mode)``,
``polish(..., channels="both")``, ``FitBatch.polish(channels="both")`` and ``fit_many(batch_polish="both")`` are the ways in;
every default is the real channel alone, as before.

The analytic Jacobian (``nmrfit_jacobian_analytic``, csrc/lsq_analytic.hip; include/nmrfit_amd_lsq_analytic.h).  The
derivative of the pseudo-Voigt residual is elementary: ``jac="analytic"`` (``ResidualModel``, ``least_squares``,
``polish``, ``FitBatch.normal_equations`` / ``polish``, ``fit_many(polish_jac=...)``) forms J, r and the normal equations
in ONE pass over the resident spectrum -- no D + 1 residual rows, no steps, no flipped steps at the upper bound -- with
f = ||r|| the call's own sum; ``jacobian_host`` states the same quantities in numpy and ``analytic_provider`` feeds
``lm_polish`` from them.  Real channel only; every default stays "2-point".
"""
import numpy as np

from . import _cabi

_SQRT_EPS = float(np.sqrt(np.finfo(np.float64).eps))


def forward_rows(x, lower=None, upper=None, rel_step=_SQRT_EPS):
    """The D + 1 parameter rows of a forward-difference Jacobian at ``x`` and the steps actually taken after
    rounding: h_i = rel_step*max(1,|x_i|), flipped where x_i + h_i would leave the box (scipy's '2-point' rule)."""
    x = np.asarray(x, dtype=np.float64)
    h = rel_step * np.maximum(1.0, np.abs(x))
    if upper is not None:
        flip = x + h > upper
        if lower is not None:
            flip &= (x - h >= lower)
        h = np.where(flip, -h, h)
    rows = np.tile(x, (x.size + 1, 1))
    idx = np.arange(x.size)
    rows[idx + 1, idx] += h
    return rows, rows[idx + 1, idx] - x


def normal_equations_host(R, c, s):
    """What csrc/lsq.hip computes from the D + 1 residual rows ``R`` [(D + 1) x N], the factors ``c`` (s / h_i) and
    ``s`` = 1/sqrt(N), in numpy: ``(A, g, J, r)`` with r = R[0]*s, J[j, i] = (R[i + 1][j] - R[0][j])*c_i [N x D],
    A = J^T J, g = J^T r.  (J and r are the device's bit for bit; A and g differ in summation order.)"""
    R = np.asarray(R, dtype=np.float64)
    c = np.asarray(c, dtype=np.float64)
    r = R[0] * s
    J = np.ascontiguousarray(((R[1:] - R[0]) * c[:, None]).T)
    return J.T @ J, J.T @ r, J, r


def jacobian_host(x, w, u, v, weights):
    """What csrc/lsq_analytic.hip computes, in numpy: ``(J, r)`` at the parameter vector ``x`` -- r = s weights (V -
    model) [N], s = 1/sqrt(N), and J [N x D] its closed-form derivatives (include/nmrfit_amd_lsq_analytic.h states them),
    t formed from the centred grid as the kernels form it.  A width of zero or below the kernels' floor is the caller's
    to avoid (the device call refuses it)."""
    x, w, u, v = (np.asarray(q, dtype=np.float64) for q in (x, w, u, v))
    N, D = w.size, x.size
    P = (D - 4) // 3
    wt = np.ones(N) if weights is None else np.asarray(weights, dtype=np.float64)
    w0 = w[N // 2]
    wc = w - w0
    frac = np.arange(N, dtype=np.float64) / float(N)
    phi = x[0] + x[1] * frac
    sn, cs = np.sin(phi), np.cos(phi)
    V, I = cs * u - sn * v, sn * u + cs * v
    q = wt * (1.0 / np.sqrt(N))
    r, yoff = x[2], x[3]
    ln2 = float(np.log(2.0))
    J = np.empty((N, D))
    model = np.zeros(N)
    d_r = np.zeros(N)
    for k in range(P):
        width, loc, a = x[4 + 3 * k:7 + 3 * k]
        ihw = 2.0 / width
        t = (wc - (loc - w0)) * ihw
        t2 = t * t
        iS = 1.0 / (1.0 + t2)
        e = np.exp2(-t2)
        Lh, Gh = ihw / np.pi * iS, ihw * np.sqrt(ln2 / np.pi) * e
        L, G = a * r * Lh, a * (1.0 - r) * Gh
        model += L + G
        d_r += a * (Lh - Gh)
        J[:, 4 + 3 * k] = q * (0.5 * ihw) * (L * (1.0 - t2) * iS + G * (1.0 - 2.0 * ln2 * t2))
        J[:, 5 + 3 * k] = -q * (2.0 * ihw * t) * (L * iS + ln2 * G)
        J[:, 6 + 3 * k] = -q * (r * Lh + (1.0 - r) * Gh)
    J[:, 0] = -q * I
    J[:, 1] = -q * I * frac
    J[:, 2] = -q * d_r
    J[:, 3] = -q * float(P)
    return J, q * (V - (model + P * yoff))     # (the reference adds yoff once per peak)


def normal_equations_host_im(R_re, R_im, c, s):
    """``normal_equations_host`` per channel: ``{"re": (A, g, rho), "im": (A, g, rho)}`` from the D + 1 residual rows of
    either channel, rho = ||r|| the channel's RMSE at row 0 -- what ``nmrfit_jacobian_im`` returns, stated in numpy (A, g
    and rho differ from the device's in summation order).  ``combine_channels`` takes the dict as it is."""
    out = {}
    for ch, R in (("re", R_re), ("im", R_im)):
        A, g, _, r = normal_equations_host(R, c, s)
        out[ch] = (A, g, float(np.sqrt(r @ r)))
    return out


def combine_channels(parts):
    """``(H, grad, f)`` of the objective f = (rho_re + rho_im)/2 from its channels' normal equations.  ``parts``: a dict
    with "re" and / or "im", or a sequence, of ``(A_ch, g_ch, rho_ch)`` with A_ch = J_ch^T J_ch, g_ch = J_ch^T r_ch and
    rho_ch = ||r_ch||.  Since d rho/dx = J^T r / rho,
        grad = (g_re/rho_re + g_im/rho_im)/2
        H    = (A_re/rho_re + A_im/rho_im)/2
    H is positive semi-definite and dominates the Gauss-Newton Hessian of f: the terms left out, -g g^T/rho^3 per channel,
    are negative semi-definite.  ``lm_polish`` solves (H + lam diag H) d = -grad and accepts on f' < f: with this triple it
    minimises the fit_im objective.  A channel whose rho is 0 or not finite contributes nothing to H and grad (it is at
    its minimum, or lost); f is half the sum of the rhos as they are.  One channel alone gives today's (A, g, f) up to
    the factor 1/(2 rho) on A and g -- which the relative damping cancels -- and f = rho/2.  Plain numpy."""
    parts = list(parts.values()) if isinstance(parts, dict) else list(parts)
    D = np.asarray(parts[0][1]).shape[0]
    H = np.zeros((D, D))
    grad = np.zeros(D)
    f = 0.0
    for A, g, rho in parts:
        rho = float(rho)
        f += 0.5 * rho
        if np.isfinite(rho) and rho > 0.0:
            H += np.asarray(A, dtype=np.float64) * (0.5 / rho)
            grad += np.asarray(g, dtype=np.float64) * (0.5 / rho)
    return H, grad, f


def _jac_form(who, jac):
    if jac not in ("2-point", "analytic"):
        raise ValueError('%s: jac is "2-point" or "analytic"' % who)
    return jac


class ResidualModel:
    """fun / jac callables over an ``equations.Evaluator``.  ``fit_im`` 0 (default): the real channel, as ever.  With a
    mode (True / "sum"): ``fun`` is the stacked 2N vector [r_re; r_im], ``jac`` the stacked 2N x D matrix (J_re above
    J_im, one ``nmrfit_jacobian_im`` call) -- scipy's TRF then minimises rho_re^2 + rho_im^2 -- and ``normal_equations``
    the combined ``(H, grad f, f)`` of the objective itself (``combine_channels``).

    ``jac="analytic"`` (real channel only): ``jac`` and ``normal_equations`` are the closed-form derivatives of ONE
    ``nmrfit_jacobian_analytic`` call at x -- f is then that call's own ||r|| -- while ``fun`` stays the rows launch;
    ``sandwich`` / ``sandwich_im`` are the forward-difference model's alone."""

    def __init__(self, evaluator, lower=None, upper=None, rel_step=_SQRT_EPS, fit_im=0, jac="2-point"):
        from .equations import fit_im_mode
        self.fit_im = fit_im_mode(fit_im)
        self.jac_form = _jac_form("ResidualModel", jac)
        if self.jac_form == "analytic" and self.fit_im:
            raise ValueError('ResidualModel: jac="analytic" covers the real channel only (fit_im=False)')
        self.ev = evaluator
        self.N = evaluator.N
        self.lower = None if lower is None else _cabi.f64(lower)
        self.upper = None if upper is None else _cabi.f64(upper)
        self.rel_step = rel_step
        self.n_fun = 0
        self.n_jac = 0
        self._scale = 1.0 / np.sqrt(self.N)

    def fun(self, x):
        self.n_fun += 1
        if self.fit_im:
            R_re, R_im, _ = self.ev.residual_batch_im(np.asarray(x, dtype=np.float64), self.fit_im)
            return np.concatenate((R_re[0], R_im[0])) * self._scale
        return self.ev.residual_batch(np.asarray(x, dtype=np.float64))[0] * self._scale

    def steps(self, x):
        """Forward steps h_i = rel_step*max(1,|x_i|), flipped where x_i + h_i would leave the
        box (scipy's '2-point' rule)."""
        x = np.asarray(x, dtype=np.float64)
        h = self.rel_step * np.maximum(1.0, np.abs(x))
        if self.upper is not None:
            flip = x + h > self.upper
            if self.lower is not None:
                flip &= (x - h >= self.lower)
            h = np.where(flip, -h, h)
        return h

    def rows(self, x):
        return forward_rows(x, self.lower, self.upper, self.rel_step)

    def jac(self, x):
        """[fun(x + h_i e_i) - fun(x)] / h_i as N x D: one launch of the D + 1 residual rows, J formed on the
        device from them (csrc/lsq.hip) -- the bits of ``(R[1:] - R[0]) * (scale / h)`` transposed."""
        self.n_jac += 1
        if self.jac_form == "analytic":
            return self.ev.jacobian_analytic(x, J=True)["J"]
        rows, h = self.rows(x)
        if self.fit_im:   # [2, N, D] as it arrives is J_re above J_im
            return self.ev.jacobian_im(rows, self._scale / h, self._scale, self.fit_im, J=True)["J"].reshape(2 * self.N, -1)
        return self.ev.jacobian(rows, self._scale / h, self._scale, J=True)["J"]

    def normal_equations(self, x):
        """``(A, g, f)`` at x: A = J^T J [D x D], g = J^T fun(x) [D] reduced on the device in a fixed order, and f the
        objective value the same launch returns for x.  D <= 76."""
        self.n_jac += 1
        if self.jac_form == "analytic":
            out = self.ev.jacobian_analytic(x, normal=True)
            return out["A"], out["g"], out["f"]
        rows, h = self.rows(x)
        if self.fit_im:
            out = self.ev.jacobian_im(rows, self._scale / h, self._scale, self.fit_im, normal=True)
            return combine_channels([(out["A"][ch], out["g"][ch], out["f2"][ch]) for ch in (0, 1)])
        out = self.ev.jacobian(rows, self._scale / h, self._scale, normal=True)
        return out["A"], out["g"], out["f"]

    def sandwich(self, x, sigma_u, sigma_v):
        """``(A, M, g, f)`` at x: ``normal_equations``'s A, g and f (the same launches, the same bits) and the meat
        M = J^T diag(q) J of the sandwich covariance under noise (sigma_u, sigma_v) on the two channels
        (``Evaluator.sandwich``; ``uncertainty.covariance`` takes them).  Real channel only, D <= 76: a model made with a
        ``fit_im`` mode has ``sandwich_im``."""
        if self.fit_im:
            raise ValueError("ResidualModel.sandwich: the covariance covers the real channel only (fit_im=False)")
        if self.jac_form == "analytic":
            raise ValueError('ResidualModel.sandwich: the meat is made of the forward-difference rows (jac="2-point")')
        self.n_jac += 1
        rows, h = self.rows(x)
        out = self.ev.sandwich(rows, self._scale / h, self._scale, sigma_u, sigma_v)
        return out["A"], out["M"], out["g"], out["f"]

    def sandwich_im(self, x, sigma_u, sigma_v):
        """``(parts, meat)`` at x for a model made with a ``fit_im`` mode: ``parts`` the channels' ``(A_ch, g_ch, rho_ch)``
        as ``combine_channels`` takes them -- the bits ``normal_equations`` combines -- and ``meat`` [3, D + 1, D + 1]
        the blocks (rr, ii, ri) of the two-channel sandwich (``Evaluator.sandwich_im``); ``uncertainty.covariance_im``
        takes both.  D <= 76."""
        if not self.fit_im:
            raise ValueError("ResidualModel.sandwich_im: the model was made without a fit_im mode: sandwich is its call")
        if self.jac_form == "analytic":
            raise ValueError('ResidualModel.sandwich_im: the meat is made of the forward-difference rows (jac="2-point")')
        self.n_jac += 1
        rows, h = self.rows(x)
        out = self.ev.sandwich_im(rows, self._scale / h, self._scale, self.fit_im, sigma_u, sigma_v)
        return [(out["A"][ch], out["g"][ch], float(out["f2"][ch])) for ch in (0, 1)], out["M"]

    def objective(self, x):
        return float(np.linalg.norm(self.fun(x)))


def least_squares(evaluator, x0, lower, upper, fit_im=0, jac="2-point", **kwargs):
    """scipy.optimize.least_squares with GPU residuals / Jacobian.  Returns the scipy result;
    ``result.cost`` is 0.5*objective**2 and ``result.objective`` the RMSE the swarm minimises.  ``fit_im`` (a mode):
    the stacked residual of both channels -- ``result.objective`` is then sqrt(rho_re^2 + rho_im^2).  ``jac``: "2-point"
    (the forward-difference Jacobian from D + 1 residual rows) or "analytic" (the closed forms, real channel only)."""
    from scipy.optimize import least_squares as _ls
    lower, upper = _cabi.f64(lower), _cabi.f64(upper)
    model = ResidualModel(evaluator, lower, upper, fit_im=fit_im, jac=jac)
    x0 = np.clip(np.asarray(x0, dtype=np.float64), lower, upper)
    kwargs.setdefault("method", "trf")
    kwargs.setdefault("x_scale", np.maximum(upper - lower, 1e-12))
    res = _ls(model.fun, x0, jac=model.jac, bounds=(lower, upper), **kwargs)
    res.objective = float(np.sqrt(2.0 * res.cost))
    res.n_residual_launches = model.n_fun + model.n_jac
    return res


def polish(evaluator, x_swarm, lower, upper, fit_im=False, channels="real", jac="2-point", **kwargs):
    """Refine a swarm result; keeps it if the least-squares step does not improve on it.

    The residual rows are the REAL-part residual only.  ``fit_im`` is the mode the swarm
    minimised: acceptance and the returned value use that same objective
    (``objective_batch(x, fit_im=...)``), so a step that lowers the real-part RMSE but raises the
    imaginary term is rejected and the meaning of the returned error never changes.

    ``channels="both"`` (with a ``fit_im`` mode): TRF on the stacked residual of both channels, [r_re; r_im] with
    J_re above J_im -- it minimises rho_re^2 + rho_im^2 where the swarm minimised (rho_re + rho_im)/2, close relatives
    with the same zero; acceptance is on the swarm's objective as above.

    ``jac="analytic"`` (``channels="real"``): TRF with the closed-form Jacobian; acceptance is unchanged."""
    x_swarm = np.asarray(x_swarm, dtype=np.float64)
    if channels not in ("real", "both"):
        raise ValueError('polish: channels is "real" or "both"')
    if _jac_form("polish", jac) == "analytic":
        if channels == "both":
            raise ValueError('polish: jac="analytic" covers the real channel only (channels="real")')
        kwargs["jac"] = jac
    if channels == "both":
        from .equations import fit_im_mode
        if not fit_im_mode(fit_im):
            raise ValueError('polish: channels="both" refines a fit_im objective: pass the fit\'s fit_im')
        kwargs["fit_im"] = fit_im
    res = least_squares(evaluator, x_swarm, lower, upper, **kwargs)
    f0, f1 = (float(f) for f in evaluator.objective_batch(np.stack([x_swarm, res.x]), fit_im=fit_im))
    if f1 <= f0:
        return res.x, f1, res
    return x_swarm, f0, res


def rows_provider(residuals, lowers, uppers, rel_step=_SQRT_EPS):
    """A ``provider`` for ``lm_polish`` from K callables ``residuals[k](rows) -> (R [(D + 1) x N], f [D + 1])`` (a
    host restatement of the residual, an ``Evaluator.residual_batch(..., return_f=True)``): rows and steps as ``ResidualModel`` makes them, the
    normal equations by ``normal_equations_host``."""
    def provider(X):
        out = []
        for k, x in enumerate(X):
            if x is None:
                out.append(None)
                continue
            rows, h = forward_rows(x, lowers[k], uppers[k], rel_step)
            R, f = residuals[k](rows)
            s = 1.0 / np.sqrt(R.shape[1])
            A, g, _, _ = normal_equations_host(R, s / h, s)
            out.append((A, g, float(f[0])))
        return out
    return provider


def analytic_provider(jacobians):
    """A ``provider`` for ``lm_polish`` from K callables ``jacobians[k](x) -> (J [N x D], r [N])`` (``jacobian_host`` on
    a spectrum, or an ``Evaluator.jacobian_analytic(x, J=True, r=True)`` unpacked): A = J^T J, g = J^T r, f = ||r||."""
    def provider(X):
        out = []
        for k, x in enumerate(X):
            if x is None:
                out.append(None)
                continue
            J, r = jacobians[k](x)
            out.append((J.T @ J, J.T @ r, float(np.sqrt(r @ r))))
        return out
    return provider


def rows_provider_im(residuals, lowers, uppers, rel_step=_SQRT_EPS):
    """``rows_provider`` on both channels: ``residuals[k](rows) -> (R_re, R_im)`` ([(D + 1) x N] each: a host
    restatement, or ``Evaluator.residual_batch_im(rows, mode)[:2]``); per fit the combined ``(H, grad f, f)`` of
    f = (rho_re + rho_im)/2 by ``normal_equations_host_im`` and ``combine_channels``."""
    def provider(X):
        out = []
        for k, x in enumerate(X):
            if x is None:
                out.append(None)
                continue
            rows, h = forward_rows(x, lowers[k], uppers[k], rel_step)
            R_re, R_im = residuals[k](rows)[:2]
            s = 1.0 / np.sqrt(R_re.shape[1])
            out.append(combine_channels(normal_equations_host_im(R_re, R_im, s / h, s)))
        return out
    return provider


def _lm_step(A, g, x, lower, upper, scale, lam):
    """One damped step of a box-bounded fit in scaled variables: variables on a bound whose descent direction points
    outward are frozen; (A' + lam diag(A')) d = -g' by Cholesky over the free ones.  None when the factorisation fails
    (the caller raises lam) or nothing is free."""
    free = ~(((x <= lower) & (g > 0.0)) | ((x >= upper) & (g < 0.0)))
    if not free.any():
        return None
    d = scale[free]
    As = A[np.ix_(free, free)] * d[:, None] * d[None, :]
    gs = g[free] * d
    diag = np.diag(As).copy()
    diag[~(diag > 0.0)] = 1.0
    try:
        L = np.linalg.cholesky(As + lam * np.diag(diag))
    except np.linalg.LinAlgError:
        return None
    step = np.linalg.solve(L.T, np.linalg.solve(L, -gs))
    if not np.all(np.isfinite(step)):
        return None
    delta = np.zeros_like(x)
    delta[free] = step * d
    return delta


def lm_polish(provider, X0, lowers, uppers, max_launches=30, lam0=1e-3, up=10.0, down=10.0, ftol=1e-12):
    """Levenberg-Marquardt on K independent box-bounded least-squares problems in lock step, from device-made (or any)
    normal equations.  ``provider(X)`` takes a list of K parameter vectors (None for a fit that has stopped) and
    returns, per entry that is not None, ``(A, g, f)`` at it: A = J^T J, g = J^T r, f = ||r||.  One call evaluates the
    trial points of every active fit -- and brings their A and g, so an accepted point needs no second call.

    Per fit: variables scaled by max(upper - lower, 1e-12) (``least_squares``'s x_scale); a variable on a bound with -g
    pointing outward is frozen for the step; the step solves (A + lam diag(A)) d = -g by Cholesky, a failed
    factorisation raises lam; the trial point is clip(x + d); f' < f accepts (lam /= down), else x stays (lam *= up).  A
    fit stops on a relative decrease below ``ftol``, on lam > 1e12, or with the budget of ``max_launches`` provider
    calls.  f never rises: the result is never worse than the start.

    Returns ``(X, f, info)``: K vectors, K values, and a dict with ``launches``, per fit ``accepted`` and ``stop``
    ("ftol", "lambda", "budget", "frozen") and ``history`` (per fit, f after every launch it took part in)."""
    K = len(X0)
    lowers = [np.asarray(lo, dtype=np.float64) for lo in lowers]
    uppers = [np.asarray(up_, dtype=np.float64) for up_ in uppers]
    scales = [np.maximum(hi - lo, 1e-12) for lo, hi in zip(lowers, uppers)]
    X = [np.clip(np.asarray(x, dtype=np.float64), lo, hi) for x, lo, hi in zip(X0, lowers, uppers)]
    got = provider(list(X))
    launches = 1
    A = [np.array(q[0]) for q in got]
    g = [np.array(q[1]) for q in got]
    f = [float(q[2]) for q in got]
    lam = [float(lam0)] * K
    stop = [None] * K
    accepted = [0] * K
    history = [[fk] for fk in f]
    active = list(range(K))
    while active:
        if launches >= max_launches:
            for k in active:
                stop[k] = "budget"
            break
        trial = [None] * K
        for k in list(active):
            delta = None
            while delta is None:
                delta = _lm_step(A[k], g[k], X[k], lowers[k], uppers[k], scales[k], lam[k])
                if delta is None:
                    free = ~(((X[k] <= lowers[k]) & (g[k] > 0.0)) | ((X[k] >= uppers[k]) & (g[k] < 0.0)))
                    if not free.any():
                        stop[k] = "frozen"
                        break
                    lam[k] *= up
                    if lam[k] > 1e12:
                        stop[k] = "lambda"
                        break
            if delta is None:
                active.remove(k)
                continue
            trial[k] = np.clip(X[k] + delta, lowers[k], uppers[k])
        if not active:
            break
        got = provider(trial)
        launches += 1
        for k in list(active):
            A1, g1, f1 = got[k]
            f1 = float(f1)
            if f1 < f[k]:
                gain = (f[k] - f1) / max(f[k], 1e-300)
                X[k], A[k], g[k], f[k] = trial[k], np.array(A1), np.array(g1), f1
                accepted[k] += 1
                lam[k] /= down
                if gain < ftol:
                    stop[k] = "ftol"
            else:
                lam[k] *= up
                if lam[k] > 1e12:
                    stop[k] = "lambda"
            history[k].append(f[k])
            if stop[k] is not None:
                active.remove(k)
    return X, np.array(f), dict(launches=launches, accepted=accepted, stop=stop, history=history)

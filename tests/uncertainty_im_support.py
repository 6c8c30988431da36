"""
Shared by tests/test_uncertainty_im_cpu.py and tests/test_gpu_uncertainty_im.py: the two-channel sandwich of a fit made
with ``fit_im`` (nmrfit_amd/uncertainty.py ``sandwich_host_im`` / ``covariance_im``, csrc/lsq_cov_im.hip).

The truths use tests/lsq_im_support.residual_rows -- the two-channel residual in closed form, both modes -- and
``lsq.lm_polish`` over ``lsq_im_support.host_provider``, which minimises f = (rho_re + rho_im)/2 itself.  ``mirror`` is the
feature's own statement on the CPU: ``sandwich_host_im`` + ``covariance_im`` on the forward-difference rows the device
forms (``lsq.forward_rows``) with the closed form in the kernel's place.  ``score_map`` is an independent statement of the
same first-order quantity, built from the rotation of (u, v) into the two channels and not from any q_ab.
"""
import functools

import numpy as np

from nmrfit_amd import lsq, noise, synth, uncertainty

from . import calibration_support as cs
from . import lsq_im_support as LI
from . import lsq_support as S

MODES = LI.MODES
RATIOS = (1.0, 2.0)              # sigma_v / sigma_u
EPS = float(np.finfo(np.float64).eps)

# -- the bars ------------------------------------------------------------------------------------------------------------
# Linear response: per parameter the worst |prediction - truth| / sigma_x of the mirror over the DIRECTION_SEEDS, per
# (mode, sigma_v / sigma_u), measured on the CPU (tests/test_uncertainty_im_cpu.py::test_linear_response re-measures and
# prints them).  prediction = -H^-1 d(grad f) for the data moved by a noise vector n; truth = the central difference of
# lm_polish refits (ftol = 0) at data +- STEP n.  What is left is what the first order neglects: sum r grad^2 r of the
# Hessian and the data dependence of J's phase columns -- not the code under test.  That remainder is 0.02 ... 0.05 on the
# two phases and a tenth of it on the line shapes, so a bar on the worst parameter would hide a fault of the line shapes
# behind the phases: every parameter is held to calibration_support.twice_rounded_up of its OWN measured value.
RESPONSE_MEASURED = {
    (1, 1.0): (0.0472, 0.0383, 0.00236, 0.000522, 0.00122, 0.036, 0.00438, 0.00455, 0.0203, 0.00197),
    (1, 2.0): (0.0543, 0.0537, 0.00571, 0.00134, 0.00235, 0.0404, 0.00531, 0.00409, 0.0429, 0.00432),
    (2, 1.0): (0.0144, 0.0192, 0.00325, 0.000323, 0.00257, 0.00991, 0.00185, 0.00067, 0.015, 0.0019),
    (2, 2.0): (0.0168, 0.0225, 0.00341, 0.00117, 0.00232, 0.0122, 0.00343, 0.000912, 0.019, 0.00301),
}
# The same with fault="no_rank_one" (the derivative of 1 / rho_ch left out of the score and of H), for the record: the
# mixing fraction, the offset, the widths and the areas leave their bars by factors of up to 9.
RESPONSE_NO_RANK_ONE = {
    (1, 1.0): (0.0746, 0.0536, 0.0118, 0.00266, 0.00176, 0.0562, 0.0142, 0.00541, 0.019, 0.0101),
    (1, 2.0): (0.0772, 0.0682, 0.0118, 0.00295, 0.0032, 0.0567, 0.0139, 0.00504, 0.048, 0.011),
    (2, 1.0): (0.0174, 0.0154, 0.00942, 0.00325, 0.00927, 0.0288, 0.0169, 0.0134, 0.0236, 0.0345),
    (2, 2.0): (0.0177, 0.0213, 0.0101, 0.00525, 0.0106, 0.0341, 0.0179, 0.0136, 0.0225, 0.0375),
}
DIRECTION_SEEDS = (9101, 9102, 9103, 9104)
STEP = 0.05
# The replica study: base seed 5 as everywhere here, copy k of mode m takes noise seed REPLICA_SEED0 + k.
REPLICAS, REPLICA_SEED0 = 63, 7300
POLISH = dict(max_launches=400, ftol=0.0)


def response_bar(mode, ratio):
    """[D]: what |prediction - truth| / sigma_x may be, parameter by parameter."""
    return np.array([cs.twice_rounded_up(v) for v in RESPONSE_MEASURED[(mode, ratio)]])


# -- the problems --------------------------------------------------------------------------------------------------------
class Problem:
    """The base of the CPU tests: ``synth.make_spectrum(512, 2, seed=5, noise=1e-3, physical=True)`` -- a noisy base, so
    both rho > 0 and the minimiser of f is a smooth function of the data -- its minimiser ``x0`` in ``mode`` (lm_polish
    from x_true, ftol = 0), and noise of the base's own level on u, ``ratio`` times it on v."""

    def __init__(self, mode, ratio, N=512, P=2, spec_seed=5):
        self.mode, self.ratio = mode, ratio
        self.sp = synth.make_spectrum(N, P, seed=spec_seed, noise=1e-3, physical=True)
        self.N, self.D = N, 4 + 3 * P
        self.lower, self.upper = np.asarray(self.sp["lower"], float), np.asarray(self.sp["upper"], float)
        self.sigma_u = float(self.sp["sigma"])
        self.sigma_v = ratio * self.sigma_u
        self.x0 = refit(self.sp, mode, self.sp["x_true"])

    def moved(self, du, dv):
        """The spectrum with (du, dv) added to (u, v)."""
        return dict(self.sp, u=self.sp["u"] + du, v=self.sp["v"] + dv)

    def direction(self, seed):
        """A noise vector of the problem's level: (sigma_u z_u, sigma_v z_v) with ``noise.normals(seed, N)``."""
        zu, zv = noise.normals(seed, self.N)
        return self.sigma_u * zu, self.sigma_v * zv


@functools.lru_cache(maxsize=None)
def problem(mode, ratio):
    return Problem(mode, ratio)


def refit(sp, mode, x_start):
    """The minimiser of f = (rho_re + rho_im)/2 on ``sp`` in ``mode``: lm_polish over the closed-form rows from
    ``x_start``, run until it cannot lower f any more."""
    X, _, _ = lsq.lm_polish(LI.host_provider([sp], mode), [np.asarray(x_start, float)], [sp["lower"]], [sp["upper"]], **POLISH)
    return X[0]


# -- the mirror ----------------------------------------------------------------------------------------------------------
def host_pieces(sp, x, mode):
    """Per channel (J [N x D], r [N], A, g, rho) at x from the closed-form rows, as the device forms them."""
    rows, h = lsq.forward_rows(x, np.asarray(sp["lower"], float), np.asarray(sp["upper"], float))
    R_re, R_im, _ = LI.residual_rows(rows, *S.spectrum_tuple(sp), mode)
    s = 1.0 / np.sqrt(R_re.shape[1])
    out = []
    for R in (R_re, R_im):
        A, g, J, r = lsq.normal_equations_host(R, s / h, s)
        out.append((J, r, A, g, float(np.sqrt(r @ r))))
    return out


def score_map(pieces, weights, x, rank_one=True):
    """(G, |G|): the D x 2N map from (du, dv) to d(grad f) at fixed J, stated directly from the rotation
    dV = cos phi du - sin phi dv, dI = sin phi du + cos phi dv:
        G = 1/2 sum_ch (1 / rho_ch) B_ch Jt_ch^T diag(weights s) [rotation of ch]
    and the same with every factor's magnitude in its place (what a rounding bound is made of).  ``rank_one`` False:
    the column r_ch of Jt_ch -- the derivative of 1 / rho_ch -- left out."""
    N = weights.shape[0]
    D = pieces[0][0].shape[1]
    phi = float(x[0]) + float(x[1]) * (np.arange(N, dtype=np.float64) / N)
    cs_, sn = np.cos(phi), np.sin(phi)
    ws = weights / np.sqrt(N)
    rot = ((cs_, -sn), (sn, cs_))
    G, Gabs = np.zeros((D, 2 * N)), np.zeros((D, 2 * N))
    for ch, (J, r, _, g, rho) in enumerate(pieces):
        if not (np.isfinite(rho) and rho > 0.0):
            continue
        Jt = np.column_stack((J, r))
        B = np.column_stack((np.eye(D), -g / (rho * rho) if rank_one else np.zeros(D)))
        half = 0.5 / rho
        for side in (0, 1):
            G[:, side * N:(side + 1) * N] += half * (B @ (Jt * (ws * rot[ch][side])[:, None]).T)
            Gabs[:, side * N:(side + 1) * N] += half * (np.abs(B) @ (np.abs(Jt) * (ws * np.abs(rot[ch][side]))[:, None]).T)
    return G, Gabs


def mirror(sp, x, mode, sigma_u, sigma_v, fault=None):
    """``(FitUncertainty, G)`` at x from the CPU mirror -- ``sandwich_host_im`` and ``covariance_im`` -- with ``score_map``
    next to it; or with one fault injected: "no_rank_one" (the derivative of 1 / rho_ch left out: the last row and
    column of every block of the meat, the g g^T / rho^3 of H and the matching column of G) or "no_cross" (the block
    Mt_ri left out: real and imaginary residuals taken as independent)."""
    if fault not in (None, "no_rank_one", "no_cross"):
        raise ValueError(fault)
    pieces = host_pieces(sp, x, mode)
    (J_re, r_re, A_re, g_re, rho_re), (J_im, r_im, A_im, g_im, rho_im) = pieces
    meat = [m.copy() for m in uncertainty.sandwich_host_im(J_re, r_re, J_im, r_im, sp["weights"], x, sigma_u, sigma_v)]
    parts = [(A_re, g_re, rho_re), (A_im, g_im, rho_im)]
    if fault == "no_cross":
        meat[2][:] = 0.0
    if fault == "no_rank_one":
        for m in meat:
            m[-1, :] = 0.0
            m[:, -1] = 0.0
        parts = [(A, np.zeros_like(g), rho) for A, g, rho in parts]
    fu = uncertainty.covariance_im(parts, meat, x, sp["lower"], sp["upper"], sigma=(sigma_u, sigma_v))
    G, _ = score_map(pieces, np.asarray(sp["weights"], float), x, rank_one=fault != "no_rank_one")
    return fu, G


def meat_of_score(pieces, weights, x, sigma_u, sigma_v):
    """(M, bound): G diag(sigma_u^2 1_N, sigma_v^2 1_N) G^T, and what ``covariance_im``'s M may differ from it by, per
    entry.  Both sides are sums of the same 4 N (D + 1)^2 real products, grouped differently.  Every product carries at
    most 24 roundings on either side (the phase: quotient, product, sum; sin and cos at 1 ulp; ws and its square; the
    variances and their combination in q_ab; the scalings by 1 / rho_ch and g_ch / rho_ch^2; the product itself); each
    side adds 2 N (D + 1) terms per channel pair in some order, which costs at most that many eps of the sum of their
    magnitudes -- and the magnitudes are those of the UNCANCELLED factors (|B| |Jt|^T |rotation|: the two channels'
    scores cancel at the minimiser of f, their roundings do not).  Twice the sum for the two sides:
        bound = 2 eps (4 N (D + 1) + 24) (|G| diag(var) |G|^T)."""
    N = weights.shape[0]
    D = pieces[0][0].shape[1]
    G, Gabs = score_map(pieces, weights, x)
    var = np.concatenate((np.full(N, sigma_u * sigma_u), np.full(N, sigma_v * sigma_v)))
    return (G * var) @ G.T, 2.0 * EPS * (4.0 * N * (D + 1) + 24.0) * ((Gabs * var) @ Gabs.T)


def predicted_shift(fu, G, du, dv):
    """-H_ff^-1 d(grad f)_f for the data moved by (du, dv): the first-order shift of the minimiser."""
    free = ~fu.fixed
    out = np.zeros(fu.x.shape[0])
    out[free] = -np.linalg.solve(fu.A[np.ix_(free, free)], (G @ np.concatenate((du, dv)))[free])
    return out


@functools.lru_cache(maxsize=None)
def response_truth(mode, ratio):
    """Per DIRECTION_SEEDS the central difference [x(data + STEP n) - x(data - STEP n)] / (2 STEP) of the minimiser of f,
    [len(DIRECTION_SEEDS) x D], by lm_polish refits from the base's minimiser."""
    p = problem(mode, ratio)
    out = []
    for seed in DIRECTION_SEEDS:
        du, dv = p.direction(seed)
        xp = refit(p.moved(STEP * du, STEP * dv), mode, p.x0)
        xm = refit(p.moved(-STEP * du, -STEP * dv), mode, p.x0)
        out.append((xp - xm) / (2.0 * STEP))
    out = np.array(out)
    out.setflags(write=False)
    return out


def response_deviation(mode, ratio, fault=None):
    """[D]: per parameter the worst |prediction - truth| / sigma_x over the directions; sigma_x is the faultless mirror's."""
    p = problem(mode, ratio)
    sigma_x = mirror(p.sp, p.x0, mode, p.sigma_u, p.sigma_v)[0].params_std
    fu, G = mirror(p.sp, p.x0, mode, p.sigma_u, p.sigma_v, fault)
    truth = response_truth(mode, ratio)
    return np.max([np.abs(predicted_shift(fu, G, *p.direction(seed)) - want) / sigma_x
                   for seed, want in zip(DIRECTION_SEEDS, truth)], axis=0)


@functools.lru_cache(maxsize=None)
def replica_minimisers(mode, ratio=2.0):
    """[REPLICAS x D]: the minimiser of f on every noisy copy of the base -- ``noise.replicas_host`` with the problem's
    (sigma_u, sigma_v) and the seeds REPLICA_SEED0 + k -- by lm_polish from the base's minimiser."""
    p = problem(mode, ratio)
    seeds = [REPLICA_SEED0 + k for k in range(REPLICAS)]
    uv = noise.replicas_host([p.sp["u"]] * REPLICAS, [p.sp["v"]] * REPLICAS, p.sigma_u, p.sigma_v, seeds)
    out = np.array([refit(dict(p.sp, u=u, v=v), mode, p.x0) for u, v in uv])
    out.setflags(write=False)
    return out


# -- the device's blocks against numpy -------------------------------------------------------------------------------------
# What |Mt_dev - Mt_numpy| may be per entry, with numpy's blocks (q Jt_a)^T Jt_b made from the device's OWN rows (Jt is
# bit for bit the host expression) and numpy's q.  The reasoning is uncertainty_support.meat_bound's, term by term: about
# 16 eps of a term for its own roundings, phi's rounding through d q / d phi, and 2 N eps for the two orders of summation.
# For the symmetric kinds d q / d phi relative to q is at most 2 (|p0| + |p1|) max sigma^2 / min sigma^2, as there.  The
# cross kind's q = ws^2 cos phi sin phi (sigma_u^2 - sigma_v^2) has zeros where its derivative does not vanish, and the
# difference of the variances cancels: every magnitude is taken with ws^2 max(sigma_u^2, sigma_v^2) in |q|'s place, which
# bounds |q| (|cos sin| <= 1/2), the error of the difference (eps max sigma^2) and |d q / d phi| <= ws^2 max sigma^2.
def blocks_bound(Jt_a, Jt_b, q, kind, weights, x, sigma_u, sigma_v):
    """[C x C]: eps * sum_j |q|_j |Jt_a[j, x]| |Jt_b[j, y]| * factor, ``kind`` in ("rr", "ii", "ri")."""
    N = Jt_a.shape[0]
    s2 = (sigma_u * sigma_u, sigma_v * sigma_v)
    phase = abs(x[0]) + abs(x[1])
    if kind == "ri":
        ws = np.asarray(weights, float) / np.sqrt(N)
        mag = ws * ws * max(s2)
        factor = 2.0 * N + 16.0 + 2.0 + 2.0 * phase
    else:
        mag = np.abs(q)
        factor = 2.0 * N + 16.0 + 2.0 * phase * max(s2) / min(s2)
    return EPS * factor * ((mag[:, None] * np.abs(Jt_a)).T @ np.abs(Jt_b))


# -- the device shapes -----------------------------------------------------------------------------------------------------
# (N, P): less than one tile; a tile tail; the CPU base's shape; three peaks; D = 76 (the full accumulator set, the split of
# the cross job, the largest LDS)
DEVICE_SHAPES = ((40, 1), (130, 2), (512, 2), (1024, 3), (256, 24))
RAGGED = ((130, 2), (1024, 3), (40, 1))
# Three fits whose doubled residual rows, 2 (D + 1) N doubles, are 84000, 81200 and 94300: any two exceed the smallest
# workspace budget (NMRFIT_LSQ_WORKSPACE_MB=1: 131072 doubles), so under it every fit is a group of its own, while the
# default budget holds a whole part.  In GROUP_ORDER they make a batch of seven fits, which the library divides over two
# parts (fits 0-2 and 3-6): every fit's share of M_out lies behind another part's and, under the small budget, behind
# other groups'.  2100 = 32 tiles and a tail of 52 points, 1400 = 21 tiles and a tail of 56.
GROUP_SHAPES = ((2100, 5), (1400, 8), (2050, 6))
GROUP_ORDER = (0, 1, 2, 0, 1, 2, 1)


@functools.lru_cache(maxsize=None)
def device_problem(N, P):
    """(spectrum, a point near its optimum, (sigma_u, sigma_v) with sigma_v = 2 sigma_u)."""
    sp = synth.make_spectrum(N, P, seed=300 + P, noise=1e-3, physical=True)
    x = S.perturbed_start(sp, 310 + P, spread=0.01)
    return sp, x, (float(sp["sigma"]), 2.0 * float(sp["sigma"]))


def lone_sandwich_im(sp, x, mode, sig, real=False):
    """(parts, meat) of ``ResidualModel.sandwich_im`` on a lone context; ``real``: (A, M, g, f) of ``sandwich`` there."""
    from nmrfit_amd.equations import Evaluator
    with Evaluator(sp["w"], sp["u"], sp["v"], sp["weights"]) as ev:
        if real:
            return lsq.ResidualModel(ev, sp["lower"], sp["upper"]).sandwich(x, sig[0], sig[1])
        return lsq.ResidualModel(ev, sp["lower"], sp["upper"], fit_im=mode).sandwich_im(x, sig[0], sig[1])


def batch_of(sps, mode, **kw):
    from nmrfit_amd.batch import FitBatch
    return FitBatch([S.spectrum_tuple(sp) for sp in sps], [sp["lower"] for sp in sps], [sp["upper"] for sp in sps],
                    swarmsize=8, seeds=list(range(len(sps))), fit_im=mode, **kw)


def raw_normal_equations_im(fb, X):
    """nmrfit_batch_normal_equations_im itself: per fit dict(A [2, D, D], g [2, D], rho [2])."""
    from nmrfit_amd import _cabi
    rows, c = [], []
    s = 1.0 / np.sqrt(fb.Ns.astype(np.float64))
    for k, x in enumerate(X):
        r, h = lsq.forward_rows(_cabi.f64(x), fb.lowers[k], fb.uppers[k])
        rows.append(r.ravel())
        c.append(s[k] / h)
    rows, c = np.concatenate(rows), np.concatenate(c)
    D = np.asarray(fb.D, dtype=np.int64)
    aoff = np.concatenate(([0], np.cumsum(D * D)))
    A, g, f2 = np.empty(2 * int(aoff[-1])), np.empty(2 * int(fb.offsets[-1])), np.empty(2 * fb.K)
    _cabi.check(_cabi.lib().nmrfit_batch_normal_equations_im(fb._h, _cabi.ptr(rows), _cabi.ptr(c), _cabi.ptr(s), _cabi.ptr(A),
                                                             _cabi.ptr(g), _cabi.ptr(f2)))
    return [dict(A=A[2 * aoff[k]:2 * aoff[k + 1]].reshape(2, D[k], D[k]),
                 g=g[2 * fb.offsets[k]:2 * fb.offsets[k + 1]].reshape(2, D[k]), rho=f2[2 * k:2 * k + 2]) for k in range(fb.K)]


def flat(parts, meat):
    """One record of a fit's (parts, meat) for bit comparisons."""
    return dict(A=np.array([p[0] for p in parts]), g=np.array([p[1] for p in parts]), rho=np.array([p[2] for p in parts]),
                M=np.array(meat))


def same_bits(a, b):
    return all(np.array_equal(a[k], b[k]) for k in ("A", "g", "rho", "M"))


def device_record(mode=2):
    """What one process gets for the RAGGED problems: every fit on a lone context and in one batch, as one dict of arrays."""
    probs = [device_problem(N, P) for N, P in RAGGED]
    rec = {}
    with batch_of([p[0] for p in probs], mode) as fb:
        got = fb.sandwich_im([p[1] for p in probs], [p[2][0] for p in probs], [p[2][1] for p in probs])
    for k, (sp, x, sig) in enumerate(probs):
        for where, pm in (("lone", lone_sandwich_im(sp, x, mode, sig)), ("batch", got[k])):
            for name, a in flat(*pm).items():
                rec["%s.%d.%s" % (where, k, name)] = a
    return rec


def main(out):
    """``python -m tests.uncertainty_im_support OUT.npz``: device_record() of this process (a child of
    tests/test_gpu_uncertainty_im.py, started with its own NMRFIT_POISON_ALLOC)."""
    np.savez(out, **device_record())


if __name__ == "__main__":
    import sys
    main(sys.argv[1])

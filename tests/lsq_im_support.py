"""
Shared by tests/test_lsq_im_cpu.py and tests/test_gpu_lsq_im.py (least squares on both channels,
include/nmrfit_amd_lsq_im.h): the two-channel residual of the objective in closed form, in numpy -- float64, an
independent statement of what the device's rows are, good for derivatives and for driving the host loop, not a truth to
the last bit (that is tests/hp_truth.py) -- and the bar the device-driven polish is held to.
"""
import numpy as np
from scipy.special import dawsn

from nmrfit_amd import lsq
from tests import lsq_support as S

MODES = (1, 2)                 # 1: the reference's fit_im=True (last peak's dispersion line only); 2: "sum" (all peaks)
_LN2 = np.log(2.0)

# The final relative gap of f = (rho_re + rho_im)/2 between lsq.lm_polish over the combined host provider
# (lsq.rows_provider_im on residual_rows below) with the budget the GPU tests give it -- 100 D launches, default ftol --
# and a long run of the same loop (2000 D launches, ftol = 0), the largest over lsq_support.polish_cases() (P = 1, 2, 3,
# N = 1024, perturbed starts) and both modes.  Measured on the CPU by tests/test_lsq_im_cpu.py
# (test_lm_polish_on_both_channels prints every case); nothing of it comes from the device code.  The GPU tests hold the
# device-driven loop to ten times it, capped at 1e-6 (beyond the cap a difference is another minimum, not another
# stopping rule) -- as lsq_support.MEASURED_GAP / FINAL_F_BAR do for the real channel.
MEASURED_GAP_IM = 6.95e-14
FINAL_F_BAR_IM = min(10.0 * MEASURED_GAP_IM, 1e-6)


def model_terms(x, w):
    """Per peak [P x N]: the absorption line (without yoff) and its dispersion partner, equations.py:141-147 and the
    Hilbert transform of it (Lorentzian 1/(1+t^2) -> t/(1+t^2); Gaussian exp(-x^2) -> (2/sqrt(pi)) Dawson(x))."""
    x = np.asarray(x, dtype=np.float64)
    r = x[2]
    width, loc, a = x[4::3, None], x[5::3, None], x[6::3, None]
    t = (w[None, :] - loc) * (2.0 / width)
    AL = a * r * (2.0 / (np.pi * width))
    AG = a * (1.0 - r) * (2.0 / width) * np.sqrt(_LN2 / np.pi)
    real = AL / (1.0 + t * t) + AG * np.exp2(-t * t)
    imag = AL * t / (1.0 + t * t) + AG * (2.0 / np.sqrt(np.pi)) * dawsn(np.sqrt(_LN2) * t)
    return real, imag


def residual_rows(rows, w, u, v, weights, mode):
    """``(R_re, R_im, f2)`` of the parameter rows [B x D]: R_re = weights (Vd - Vf), R_im = weights (Id - If) with If of
    ``mode``, f2 [B x 2] the two RMSEs -- the quantities of include/nmrfit_amd_lsq_im.h in closed form."""
    rows = np.atleast_2d(np.asarray(rows, dtype=np.float64))
    N = w.size
    jn = np.arange(N) / N
    R_re, R_im = np.empty((rows.shape[0], N)), np.empty((rows.shape[0], N))
    for b, x in enumerate(rows):
        phi = x[0] + x[1] * jn
        cs, sn = np.cos(phi), np.sin(phi)
        real, imag = model_terms(x, w)
        P = real.shape[0]
        Vf = P * x[3] + real.sum(axis=0)
        If = (imag[-1] if P else np.zeros(N)) if mode == 1 else imag.sum(axis=0)
        R_re[b] = weights * ((cs * u - sn * v) - Vf)
        R_im[b] = weights * ((sn * u + cs * v) - If)
    f2 = np.stack((np.sqrt(np.mean(R_re * R_re, axis=1)), np.sqrt(np.mean(R_im * R_im, axis=1))), axis=1)
    return R_re, R_im, f2


def magnitudes(x, w, u, v, weights):
    """||m|| with m_j = weights_j (|u_j| + |v_j| + sum of the magnitudes of the model's terms) / sqrt(N): what a rounding
    of relative size eps anywhere in ``residual_rows`` moves one channel's scaled residual vector by, per unit of eps."""
    real, imag = model_terms(x, w)
    m = weights * (np.abs(u) + np.abs(v) + np.abs(real).sum(axis=0) + np.abs(imag).sum(axis=0) + real.shape[0] * abs(x[3]))
    return float(np.linalg.norm(m) / np.sqrt(w.size))


def objective(x, sp, mode):
    return float(residual_rows(x, *S.spectrum_tuple(sp), mode)[2].mean())


def host_residual(sp, mode):
    return lambda rows: residual_rows(rows, *S.spectrum_tuple(sp), mode)


def host_provider(specs, mode):
    return lsq.rows_provider_im([host_residual(sp, mode) for sp in specs], [sp["lower"] for sp in specs],
                                [sp["upper"] for sp in specs])

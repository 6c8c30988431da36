"""
Host mirror of the reference's phase module (nmrfit/proc_autophase.py): ``ps2`` (:9-36),
``ps`` (:39-68), ``autops`` (:71-104), ``approximate_phase`` (:107-139) and the two phase
scores (ACME :142-187, peak minima :190-219).  Host code, as in the reference: Data.shift_phase and
FitUtility.generate_result run these; inside the objective the rotation is fused into the GPU kernel.
For many spectra, phase_scores / approximate_phase_many / autops_many (end of this module) run the
scores and the whole optimisation on the GPU (opt-in).  ``manual_ps`` (:222-300, a matplotlib slider GUI) is out of scope.

Units follow the reference: ``ps2`` takes radians, ``ps`` and the scores take DEGREES, and
``approximate_phase`` converts the optimiser's degrees to the radians ``Data`` stores.
"""
import numpy as np
import scipy.optimize

from ._cabi import _MAX_SPECTRA_PER_CALL


def _ramp(size, p0, p1):
    """exp(i (p0 + p1 j / size)), j the array index: the order of operations of the reference."""
    return np.exp(1.0j * (p0 + (p1 * np.arange(size) / size)))


def ps2(u, v, p0=0.0, p1=0.0, inv=False):
    """(u + i v) * exp(+-i (p0 + p1*j/N)), radians, j the array index; returns (real, imag)."""
    data = np.asarray(u) + 1j * np.asarray(v)
    apod = _ramp(data.shape[-1], p0, p1).astype(data.dtype)
    if inv:
        apod = 1 / apod
    data = apod * data
    return data.real, data.imag


def ps(data, p0=0.0, p1=0.0, inv=False):
    """Linear phase correction of a complex spectrum, p0 and p1 in degrees (proc_autophase.py:39-68)."""
    data = np.asarray(data)
    apod = _ramp(data.shape[-1], p0 * np.pi / 180.0, p1 * np.pi / 180.0).astype(data.dtype)
    if inv:
        apod = 1 / apod
    return apod * data


def _ps_acme_score(ph, data):
    """ACME score (Chen Li et al., J. Magn. Reson. 158 (2002) 164-168) as the reference evaluates
    it (proc_autophase.py:142-187): entropy of the normalised absolute first difference of the
    real part, plus 1000 x the sum of squares of its negative excursions."""
    real = np.real(ps(data, p0=ph[0], p1=ph[1]))
    slope = np.abs((real[1:] - real[:-1]) / 2.0)
    prob = slope / np.sum(slope)
    prob[prob == 0] = 1                       # 0 log 0 := 0
    entropy = np.sum(-prob * np.log(prob))
    neg = real - np.abs(real)                 # 2 x the negative part
    penalty = np.sum((neg / 2) ** 2) if np.sum(neg) < 0 else 0.0
    return entropy + 1000 * penalty


def _ps_peak_minima_score(ph, data):
    """|min left - min right| within 100 points of the tallest point (proc_autophase.py:190-219)."""
    real = np.real(ps(data, p0=ph[0], p1=ph[1]))
    i = np.argmax(real)
    return np.abs(np.min(real[i - 100:i]) - np.min(real[i:i + 100]))


_SCORES = {"acme": _ps_acme_score, "peak_minima": _ps_peak_minima_score}


def _optimise(data, fn, p0, p1):
    if not callable(fn):
        fn = _SCORES[fn]
    return scipy.optimize.fmin(fn, x0=[p0, p1], args=(data,), disp=False)


def autops(data, fn, p0=0.0, p1=0.0):
    """Nelder-Mead over (p0, p1) in degrees on the chosen score; returns the phased spectrum
    (proc_autophase.py:71-104)."""
    opt = _optimise(data, fn, p0, p1)
    return ps(data, p0=opt[0], p1=opt[1])


def approximate_phase(data, fn, p0=0.0, p1=0.0):
    """The same optimisation, returning (p0, p1) in RADIANS (proc_autophase.py:107-139) -- what
    Data.shift_phase('auto') stores."""
    opt = _optimise(data, fn, p0, p1)
    return opt[0] * np.pi / 180, opt[1] * np.pi / 180


# ---- device-batched phase estimation (opt-in; libnmrfit_amd.so: nmrfit_phase_scores / _estimate / _brute_levels) ---
# The functions above stay the host path Data.shift_phase runs.  These evaluate the same scores and run the same
# scipy.optimize.fmin for a whole list of spectra of any lengths on the GPU: one workgroup per spectrum runs the whole
# Nelder-Mead, each score a workgroup reduction.  Inputs are converted to float64: a complex64
# spectrum is phased in fp64 here, where the host path builds a complex64 ramp.

_KINDS = {"acme": 0, "peak_minima": 1}


def _kind(fn):
    if fn not in _KINDS:
        raise ValueError("fn must be 'acme', 'peak_minima' or a callable, got %r" % (fn,))
    return _KINDS[fn]


def _pack(spectra):
    """(N, u, v) of a list of complex spectra, the spectra one after the other, float64."""
    zs = [np.asarray(z) for z in spectra]
    if not zs:
        raise ValueError("no spectra")
    N = np.array([z.shape[-1] for z in zs], dtype=np.int64)
    for k, z in enumerate(zs):
        if z.ndim != 1:
            raise ValueError("spectrum %d is not one-dimensional" % k)
    u = np.ascontiguousarray(np.concatenate([z.real for z in zs]), dtype=np.float64)
    v = np.ascontiguousarray(np.concatenate([z.imag if np.iscomplexobj(z) else np.zeros(z.shape) for z in zs]),
                             dtype=np.float64)
    return N, u, v


def _chunks(N):
    """(k0, k1, o0, o1): spectra [k0, k1) of at most _MAX_SPECTRA_PER_CALL, their points [o0, o1) of the packed u, v.
    Spectra are independent and a spectrum's values do not depend on its batch, so cutting changes no value."""
    off = np.concatenate([[0], np.cumsum(N)])
    for k0 in range(0, len(N), _MAX_SPECTRA_PER_CALL):
        k1 = min(k0 + _MAX_SPECTRA_PER_CALL, len(N))
        yield k0, k1, int(off[k0]), int(off[k1])


def _device_scores(kind, N, u, v, cand, device=0):
    """nmrfit_phase_scores: cand is (S, M, 2); returns (S, M) scores and S statuses."""
    from . import _cabi
    cand = np.ascontiguousarray(cand, dtype=np.float64)
    S, M = cand.shape[0], cand.shape[1]
    score = np.empty((S, M), dtype=np.float64)
    status = np.zeros(S, dtype=np.int32)
    for k0, k1, o0, o1 in _chunks(N):
        _cabi.check(_cabi.lib().nmrfit_phase_scores(
            int(device), int(kind), k1 - k0, _cabi.ptr(N[k0:k1]), _cabi.ptr(u[o0:o1]), _cabi.ptr(v[o0:o1]), M,
            _cabi.ptr(cand[k0:k1]), _cabi.ptr(score[k0:k1]), _cabi.ptr(status[k0:k1])))
    return score, status


def _empty_window(status):
    bad = np.flatnonzero(status)
    if bad.size:
        raise ValueError("peak minima: spectrum %d has its tallest point within its first 100 points, where the "
                         "reference's window real[i - 100:i] is empty (np.min raises)" % bad[0])


def phase_scores(spectra, phases, fn='acme', device=0):
    """The ACME or peak-minima score (``_ps_acme_score`` / ``_ps_peak_minima_score``) of every phase pair for every
    spectrum, on the GPU.  ``spectra``: complex arrays of any lengths; ``phases``: (p0, p1) in DEGREES, shape (M, 2)
    (the same pairs for every spectrum) or (S, M, 2).  Returns an (S, M) array.  Spectra are phased in float64
    (complex64 input too).  ValueError where a peak-minima window is empty (the reference raises there)."""
    N, u, v = _pack(spectra)
    S = len(N)
    ph = np.asarray(phases, dtype=np.float64)
    if ph.ndim == 2 and ph.shape[1] == 2:
        ph = np.broadcast_to(ph, (S,) + ph.shape)
    if ph.ndim != 3 or ph.shape[0] != S or ph.shape[2] != 2 or ph.shape[1] < 1:
        raise ValueError("phases must be (M, 2) or (S, M, 2) with S = %d, got %s" % (S, np.shape(phases)))
    kind = _kind(fn)
    score, status = _device_scores(kind, N, u, v, ph, device)
    if kind == _KINDS["peak_minima"]:
        _empty_window(status)
    return score


def estimate_many(spectra, fn='acme', p0=0.0, p1=0.0, device=0):
    """fmin over (p0, p1) for every spectrum on the GPU: (x in DEGREES (S, 2), f, nfev, nit), as
    ``scipy.optimize.fmin(score, [p0, p1], full_output=True)`` returns them per spectrum."""
    from . import _cabi
    N, u, v = _pack(spectra)
    S = len(N)
    x0 = np.empty((S, 2), dtype=np.float64)
    x0[:, 0] = np.broadcast_to(np.asarray(p0, dtype=np.float64), (S,))
    x0[:, 1] = np.broadcast_to(np.asarray(p1, dtype=np.float64), (S,))
    x = np.empty((S, 2), dtype=np.float64)
    f = np.empty(S, dtype=np.float64)
    nfev, nit, status = (np.zeros(S, dtype=np.int32) for _ in range(3))
    for k0, k1, o0, o1 in _chunks(N):
        _cabi.check(_cabi.lib().nmrfit_phase_estimate(
            int(device), _kind(fn), k1 - k0, _cabi.ptr(N[k0:k1]), _cabi.ptr(u[o0:o1]), _cabi.ptr(v[o0:o1]),
            _cabi.ptr(x0[k0:k1]), _cabi.ptr(x[k0:k1]), _cabi.ptr(f[k0:k1]), _cabi.ptr(nfev[k0:k1]), _cabi.ptr(nit[k0:k1]),
            _cabi.ptr(status[k0:k1])))
    _empty_window(status)
    return x, f, nfev, nit


def approximate_phase_many(spectra, fn='acme', p0=0.0, p1=0.0, device=0):
    """``[approximate_phase(z, fn, p0, p1) for z in spectra]`` as an (S, 2) array in RADIANS, every optimisation on
    the GPU in one launch.  ``p0``, ``p1``: starting points in degrees, scalars or one per spectrum.  A callable ``fn``
    runs that host loop.  Spectra are phased in float64: complex64 input is not phased with the reference's complex64
    ramp.  ValueError naming the spectrum where a peak-minima window is empty."""
    if callable(fn):
        S = len(spectra)
        p0s = np.broadcast_to(np.asarray(p0, dtype=np.float64), (S,))
        p1s = np.broadcast_to(np.asarray(p1, dtype=np.float64), (S,))
        return np.array([approximate_phase(z, fn, a, b) for z, a, b in zip(spectra, p0s, p1s)], dtype=np.float64).reshape(S, 2)
    x = estimate_many(spectra, fn, p0, p1, device)[0]
    return x * np.pi / 180


def autops_many(spectra, fn='acme', p0=0.0, p1=0.0, device=0):
    """``[autops(z, fn, p0, p1) for z in spectra]``: the phased spectra, the optimisation on the GPU (host ``ps``
    applies the phases; a callable ``fn`` runs the host loop)."""
    if callable(fn):
        S = len(spectra)
        p0s = np.broadcast_to(np.asarray(p0, dtype=np.float64), (S,))
        p1s = np.broadcast_to(np.asarray(p1, dtype=np.float64), (S,))
        return [autops(z, fn, a, b) for z, a, b in zip(spectra, p0s, p1s)]
    x = estimate_many(spectra, fn, p0, p1, device)[0]
    return [ps(z, p0=opt[0], p1=opt[1]) for z, opt in zip(spectra, x)]


def brute_levels(us, vs, angles, device=0, n=None):
    """The level test of Data._brute_phase for every angle and spectrum: (S, M) errors, NaN where the rotated
    spectrum is not upright (max(V) <= |min(V)|).  The rotation factors are exp(1j * angle), built here as ps2 builds
    them.  The device rounds V = real(exp(1j angle) (u + 1j v)) as fma(c, u, -(s v)), which is how numpy's complex
    multiply rounds it when it runs its FMA loop (x86-64 with AVX2 or AVX-512: the errors are then the host loop's bit
    for bit); a numpy without that loop rounds c u - s v and can differ in the last bit.

    ``n``: the length of the two means, a scalar or one per spectrum; None takes max(1, N // 5000) from each spectrum's
    length N.  The host loop takes n from len(self.V) before its scan, and select_bounds crops u, v but not V: on a
    cropped Data that n is not N's (shift_phase_many passes the host's).  Where n > N the slices V[:n], V[-n:] are the
    whole spectrum and the error is 0, as in python.  Mean lengths above 128 are refused (NmrfitError,
    NMRFIT_E_UNSUPPORTED; by default spectra of 645000 points or more): those means would take numpy's recursive
    pairwise order, which the device does not restate.  Any number of spectra (cut into calls of at most 65535)."""
    from . import _cabi
    fac = np.exp(1j * np.asarray(angles, dtype=np.float64))
    S = len(us)
    cand = np.empty((S, fac.size, 2), dtype=np.float64)
    cand[:, :, 0] = fac.real
    cand[:, :, 1] = fac.imag
    N = np.array([len(u) for u in us], dtype=np.int64)
    u = np.ascontiguousarray(np.concatenate([np.asarray(a, dtype=np.float64) for a in us]))
    v = np.ascontiguousarray(np.concatenate([np.asarray(a, dtype=np.float64) for a in vs]))
    if n is None:
        n_mean = np.maximum(1, N // 5000)
    else:
        n_mean = np.ascontiguousarray(np.broadcast_to(np.asarray(n, dtype=np.int64), (S,)))
    score = np.empty((S, fac.size), dtype=np.float64)
    for k0, k1, o0, o1 in _chunks(N):
        _cabi.check(_cabi.lib().nmrfit_phase_brute_levels(
            int(device), k1 - k0, _cabi.ptr(N[k0:k1]), _cabi.ptr(n_mean[k0:k1]), _cabi.ptr(u[o0:o1]),
            _cabi.ptr(v[o0:o1]), fac.size, _cabi.ptr(cand[k0:k1]), _cabi.ptr(score[k0:k1])))
    return score

"""
Raw FIDs to spectra on the device (include/nmrfit_amd_fid.h, csrc/fid.hip).

The reference makes a spectrum in ``core.load`` (nmrfit/core.py:51-60), between nmrglue's file reader and ``Data``:

    data = ng.proc_base.fft(data)            # fftshift(fft(data, axis=-1))
    data = data / np.max(data)               # complex max (lexicographic), complex division
    u = data.real.sum(axis=0);  v = data.imag.sum(axis=0)
    w = np.linspace(rangeppm - offsetppm, -offsetppm, u.size)
    result = containers.Data(w[::-1], u[::-1], v[::-1])

The file readers stay out of scope.  The arithmetic from "complex FID in memory" to (w, u, v) is here: a batched fp64
Fourier transform with zero filling on the GPU, whose last pass stores centred and reversed, then the normaliser, the
quotient (Smith's rule, numpy's complex division) and the sum over traces.

    transform_many(fids, zero_fill)          K FIDs (one or several traces each, any mix of lengths), one library call
    transform_host(fid, zero_fill)           the reference lines above restated with np.fft (no nmrglue needed)
    finish_host(Y)                           the finishing stage exactly as the header words it: (u, v, row) from Y
    ppm_axis(n, sw, sfrq, tof)               core.load's w (host numpy: a grid is not device work)
    spectra_from_fids(fids, sw, sfrq, tof)   a list of Data, ready for shift_phase_many and the rest

A complex64 FID is widened exactly to fp64 on the host and the output is fp64: the reference's Varian path rounds the
transform to complex64 (nmrglue's cast), which is not reproduced.

CONDITIONING (include/nmrfit_amd_fid_cond.h, csrc/fid_cond.hip).  The Bruker branch of ``core.load`` (nmrfit/core.py:34-43)
runs nmrglue's ``remove_digital_filter`` between the reader and the transform, and any real spectrum gets a window there.
``transform_many`` and ``spectra_from_fids`` take both -- ``grpdly=``, ``grpdly_mode=``, ``window=`` -- and do them on the
device in the same library call (nmrfit_fid_condition_transform).  nmrglue is not a dependency and no parity with it is
claimed: the definition is the header's, modelled on nmrglue's ``rm_dig_filter`` and normative on its own.  With
rho_n(i) = exp(+2 pi i g i / n):

    "fid"        per trace x of s points (s a power of two on the device):  X = fft(x);  B[k] = X[k] rho_s(k);
                 y[j] = fft(B)[(-j) mod s] / s  (the inverse transform);  skip = floor(g + 2),  add = max(skip - 6, 0);
                 y[j] += y[s - 1 - j] for j < add;  the conditioned trace is y[:s - skip]
    "spectrum"   the trace stays as it is; after the main transform Y[i] *= rho_n(i), i the centred index, before the
                 normaliser -- an exact shift of the signed frequency up to the constant factor exp(-i pi g), which p0
                 absorbs.  Any trace length.
    window       x'[j] = y[j] W[j], one product per part, after the "fid" form; W[0] = 0.5 is first-point scaling

    condition_host(fid, grpdly, mode, window, zero_fill)   the definition in numpy (fp64, or long double for a clongdouble FID)
    conditioned_length(n_in, grpdly, mode)                 n_in' = n_in - floor(g + 2) ("fid") or n_in
    ramp(g, n)                                             rho_n, its angle reduced mod 1 exactly in integers
    window_em / window_gauss / window_sine                 plain numpy windows, ``first_point=`` for W[0]

Only a group delay given as a number (GRPDLY) is taken; the DSPFVS / DECIM table of old firmware is out of scope.

ANY LENGTH (include/nmrfit_amd_fid_any.h, csrc/fid_any.hip).  ``core.load`` transforms a FID at the length it has; the
kernels take powers of two.  With ``any_length=True``, ``transform_many`` and ``spectra_from_fids`` transform a length that
is not a power of two (3 .. 2^21 - 1) at exactly that length, by a chirp-z (Bluestein) transform on the device
(nmrfit_fid_transform_any): three transforms of length M = 2^m >= 2 N - 1 by the same kernels and four element-wise stages.
``grpdly_mode="fid"`` then needs no ``zero_fill``: a Bruker FID of s = 2^m points comes out on the grid of s - floor(g + 2)
points, as ``core.load`` makes it.  ``grpdly_mode="spectrum"`` still needs a power of two.  Without ``any_length`` every
call, message and bit is as before.

    bluestein_host(x, N)                     the header's definition step by step in numpy, centred: fp64 (the mirror), or
                                             long double for a clongdouble input (the tests' truth)
    chirp(N)                                 c[k] = exp(-i pi k^2 / N), the angle reduced mod 2 N exactly in integers
"""
import functools

import numpy as np

from . import _cabi

ROW = 6                  # doubles per row (NMRFIT_FID_ROW): status, Re m, Im m, flat index of m, n, T
MAX_LOG2 = 22            # NMRFIT_FID_MAX_LOG2
LDS_LOG2 = 12            # NMRFIT_FID_LDS_LOG2: the longest transform that is one LDS-resident block
MAX_VALUES = 1 << 26     # T n summed over the spectra of one library call
ANY_MIN, ANY_MAX = 3, (1 << 21) - 1      # NMRFIT_FID_ANY_MIN / _MAX: the lengths the chirp path takes (no power of two)
OK, ZERO, NOT_FINITE = 0, 1, 2
FORM_NONE, FORM_FID, FORM_SPECTRUM = 0, 1, 2      # NMRFIT_FID_FORM_*
_MODES = {"fid": FORM_FID, "spectrum": FORM_SPECTRUM}


def ppm_axis(n, sw, sfrq, tof):
    """``core.load``'s grid as ``Data`` holds it: ``np.linspace(sw/sfrq - tof/sfrq, -tof/sfrq, n)[::-1]`` (sw: spectral
    width in Hz, sfrq: spectrometer frequency in MHz, tof: transmitter offset in Hz)."""
    rangeppm, offsetppm = sw / sfrq, tof / sfrq
    return np.linspace(rangeppm - offsetppm, -offsetppm, n)[::-1]


def _as_traces(fid, keep_long=False):
    """A FID as a contiguous (T, n_in) complex128 array (complex64 widens exactly); ``keep_long``: a clongdouble FID
    stays one (the numpy restatements' truth)."""
    a = np.asarray(fid)
    if keep_long and a.dtype == np.clongdouble and a.ndim in (1, 2) and a.size:
        return np.ascontiguousarray(a.reshape(-1, a.shape[-1]))
    if a.dtype not in (np.complex64, np.complex128):
        raise ValueError("fid: a FID is a complex64 or complex128 array (got %s)" % a.dtype)
    if a.ndim not in (1, 2) or a.shape[-1] == 0 or a.shape[0] == 0:
        raise ValueError("fid: a FID has shape (n,) or (T, n) with n, T > 0 (got %r)" % (a.shape,))
    return np.ascontiguousarray(a.reshape(-1, a.shape[-1]), dtype=np.complex128)


def _is_pow2(n):
    return n >= 1 and not n & (n - 1)


def transform_length(n_in, zero_fill=None, any_length=False):
    """The transform length of a trace of n_in points: n_in itself (None), the next power of two ("pow2"), or the int
    given.  ValueError, naming ``zero_fill``, for a length the device refuses: anything but a power of two, 2 .. 2^22 --
    or, with ``any_length``, any other length, 3 .. 2^21 - 1."""
    if zero_fill is None:
        n = int(n_in)
    elif isinstance(zero_fill, str):
        if zero_fill != "pow2":
            raise ValueError("fid: zero_fill is None, 'pow2' or an int (got %r)" % (zero_fill,))
        n = 2
        while n < n_in:
            n *= 2
    else:
        n = int(zero_fill)
        if n < n_in:
            raise ValueError("fid: zero_fill=%d is shorter than the trace (%d points)" % (n, n_in))
    if any_length and not _is_pow2(n):
        if n < ANY_MIN or n > ANY_MAX:
            raise ValueError("fid: a transform length is a power of two, 2 .. 2^%d, or with any_length any other length, "
                             "%d .. 2^21 - 1 (got %d): pass a zero_fill within these" % (MAX_LOG2, ANY_MIN, n))
        return n
    if n < 2 or n & (n - 1) or n > 1 << MAX_LOG2:
        raise ValueError("fid: a transform length is a power of two, 2 .. 2^%d (got %d): pass zero_fill='pow2', or "
                         "zero_fill=<a power of two>; other lengths are refused, not emulated" % (MAX_LOG2, n))
    return n


# -- the numpy restatements --------------------------------------------------------------------------------------

def transform_host(fid, zero_fill=None, return_transform=False):
    """The reference lines of ``core.load`` with ``np.fft``: (u, v) as ``Data`` holds them (reversed), plus
    Y = fftshift(fft(x)) of every trace when ``return_transform``.  Any transform length numpy takes."""
    x = _as_traces(fid)
    n = x.shape[-1] if zero_fill is None else (transform_length(x.shape[-1], "pow2") if isinstance(zero_fill, str) else int(zero_fill))
    if isinstance(zero_fill, str) and zero_fill != "pow2":
        raise ValueError("fid: zero_fill is None, 'pow2' or an int (got %r)" % (zero_fill,))
    if n < x.shape[-1]:
        raise ValueError("fid: zero_fill=%d is shorter than the trace (%d points)" % (n, x.shape[-1]))
    Y = np.fft.fftshift(np.fft.fft(x, n=n, axis=-1), axes=-1)
    with np.errstate(all="ignore"):
        data = Y / np.max(Y)
    u, v = data.real.sum(axis=0), data.imag.sum(axis=0)
    return (u[::-1], v[::-1], Y) if return_transform else (u[::-1], v[::-1])


def finish_host(Y):
    """The finishing stage as include/nmrfit_amd_fid.h words it, from Y of shape (T, n) or (n,) in its natural order:
    the lexicographic maximum m (ties: the first flat index), Y / m by Smith's rule with every operation rounded once,
    the running sum over the traces from +0.0, reversed.  Returns (u, v, row)."""
    Y = np.asarray(Y, dtype=np.complex128)
    Y = Y.reshape(-1, Y.shape[-1])
    T, n = Y.shape
    row = np.array([OK, np.nan, np.nan, np.nan, n, T], dtype=np.float64)
    a, b = Y.real, Y.imag
    nan = np.full(n, np.nan)
    if not (np.isfinite(a).all() and np.isfinite(b).all()):
        row[0] = NOT_FINITE
        return nan, nan.copy(), row
    fa, fb = a.ravel(), b.ravel()
    top = np.flatnonzero(fa == fa.max())
    at = int(top[np.argmax(fb[top])])           # (argmax: the first of equal values)
    mr, mi = np.float64(fa[at]), np.float64(fb[at])
    row[1:4] = mr, mi, at
    if mr == 0.0 and mi == 0.0:
        row[0] = ZERO
        return nan, nan.copy(), row
    with np.errstate(all="ignore"):
        if abs(mr) >= abs(mi):
            rat = mi / mr
            scl = 1.0 / (mr + mi * rat)
            qr, qi = (a + b * rat) * scl, (b - a * rat) * scl
        else:
            rat = mr / mi
            scl = 1.0 / (mi + mr * rat)
            qr, qi = (a * rat + b) * scl, (b * rat - a) * scl
        u, v = np.zeros(n), np.zeros(n)             # (np.sum's start: -0.0 alone comes out as +0.0)
        for t in range(T):
            u = u + qr[t]
            v = v + qi[t]
    return u[::-1], v[::-1], row


# -- conditioning: the numpy restatement ---------------------------------------------------------------------------

def grpdly_value(grpdly, truncate_grpdly=True):
    """The group delay as used: a float, rounded to one decimal unless ``truncate_grpdly`` is False (the parameter file's
    value, e.g. 67.98416137695312, is then taken as given).  ValueError unless it is finite and > 0."""
    g = float(grpdly)
    if not np.isfinite(g) or g <= 0.0:
        raise ValueError("fid: grpdly is a finite number > 0 (got %r)" % (grpdly,))
    if truncate_grpdly:
        g = float(np.round(g, 1))
        if g <= 0.0:
            raise ValueError("fid: grpdly rounds to 0 at one decimal (got %r): pass truncate_grpdly=False" % (grpdly,))
    return g


def _mode(grpdly_mode):
    if grpdly_mode not in _MODES:
        raise ValueError("fid: grpdly_mode is 'fid' or 'spectrum' (got %r)" % (grpdly_mode,))
    return _MODES[grpdly_mode]


def conditioned_length(n_in, grpdly=None, mode="fid"):
    """n_in': the points of a trace as it enters the main transform -- n_in - floor(g + 2) in the "fid" form, which needs
    n_in >= 2 floor(g + 2); n_in otherwise.  ``grpdly`` as used (see ``grpdly_value``)."""
    n_in = int(n_in)
    if grpdly is None or _mode(mode) != FORM_FID:
        return n_in
    skip = int(np.floor(float(grpdly) + 2.0))
    if n_in < 2 * skip:
        raise ValueError("fid: grpdly_mode='fid' needs a trace of at least 2 floor(grpdly + 2) = %d points (got %d)" % (2 * skip, n_in))
    return n_in - skip


@functools.lru_cache(maxsize=64)
def _ramp_cached(g, n, long):
    num, den = float(g).as_integer_ratio()                       # g exactly; den is a power of two
    k = (den * n).bit_length() - 1                               # g i / n = num i / 2^k   (n a power of two)
    if den * n != 1 << k:                                        # any other n: an exact rational, cut to 64 bits below
        k = 80
        top = [(((num * i) % (den * n)) << k) // (den * n) for i in range(n)]
    else:
        top = [(num * i) & ((1 << k) - 1) for i in range(n)]
    sh = max(0, k - 64)                                          # the fraction's first 64 bits (k - sh of them)
    hi = np.array([(t >> sh) >> 32 for t in top], dtype=np.float64).astype(np.longdouble)
    lo = np.array([(t >> sh) & 0xFFFFFFFF for t in top], dtype=np.float64).astype(np.longdouble)
    frac = (hi * np.longdouble(2.0 ** 32) + lo) / np.longdouble(2) ** (k - sh)
    two_pi = 2 * np.arctan2(np.longdouble(0), np.longdouble(-1))
    rho = (np.cos(two_pi * frac) + 1j * np.sin(two_pi * frac)).astype(np.clongdouble)
    rho = rho if long else rho.astype(np.complex128)
    rho.setflags(write=False)
    return rho


def ramp(g, n, dtype=np.complex128):
    """rho_n(i) = exp(+2 pi i g i / n), i = 0 .. n-1.  g i / n is reduced mod 1 exactly (Python integers on g's own bits)
    before cos and sin are taken in long double; fp64 is the rounding of that.  Read-only (cached)."""
    return _ramp_cached(float(g), int(n), np.dtype(dtype) == np.clongdouble)


def _times_window(y, W):
    """y[j] W[j]: one product per part (numpy's complex product with a real factor adds b * 0.0 and loses a -0.0)."""
    out = np.empty_like(y)
    out.real = y.real * W
    out.imag = y.imag * W
    return out


def condition_host(fid, grpdly=None, mode="fid", window=None, zero_fill=None):
    """The definition of include/nmrfit_amd_fid_cond.h in numpy: ``(xc, Y)`` -- the conditioned traces (T, n_in') as they
    enter the main transform, and Y (T, n) = fftshift(fft(xc, n)), times rho_n in the "spectrum" form; ``finish_host(Y)``
    gives (u, v, row).  ``grpdly`` as used (no rounding here; None: no removal), ``window``: None or n_in' reals.  A
    clongdouble FID is conditioned and transformed in long double (the tests' truth); any length numpy takes."""
    x = _as_traces(fid, keep_long=True)
    long = x.dtype == np.clongdouble
    real = np.longdouble if long else np.float64
    form = FORM_NONE if grpdly is None else _mode(mode)
    s = x.shape[-1]
    y = x
    if form == FORM_FID:
        n_out = conditioned_length(s, grpdly, mode)
        skip, add = s - n_out, max(s - n_out - 6, 0)
        B = np.fft.fft(x, axis=-1) * ramp(grpdly, s, x.dtype)
        y = np.fft.fft(B, axis=-1)[:, (-np.arange(s)) % s] / real(s)      # the inverse transform by the forward one
        j = np.arange(add)
        y[:, j] = y[:, j] + y[:, s - 1 - j]
        y = y[:, :s - skip]
    if window is not None:
        W = np.asarray(window, dtype=real)
        if W.shape != (y.shape[-1],):
            raise ValueError("fid: a window has as many values as the conditioned trace has points (%d, got shape %r)" % (y.shape[-1], W.shape))
        y = _times_window(y, W)
    xc = np.ascontiguousarray(y)
    n = xc.shape[-1] if zero_fill is None else (transform_length(xc.shape[-1], "pow2") if isinstance(zero_fill, str) else int(zero_fill))
    if n < xc.shape[-1]:
        raise ValueError("fid: zero_fill=%d is shorter than the conditioned trace (%d points)" % (n, xc.shape[-1]))
    Y = np.fft.fftshift(np.fft.fft(xc, n=n, axis=-1), axes=-1)
    if form == FORM_SPECTRUM:
        Y = Y * ramp(grpdly, n, x.dtype)
    return xc, Y


# -- any length: the numpy restatement ------------------------------------------------------------------------------

def conv_length(N):
    """M = 2^m, the smallest power of two >= 2 N - 1."""
    M = 1
    while M < 2 * int(N) - 1:
        M *= 2
    return M


@functools.lru_cache(maxsize=16)
def _chirp_cached(N, long):
    k = np.arange(N, dtype=np.int64)
    r = (k * k) % (2 * N)                                        # exact: k^2 < 2^42
    eighths = 4 * r                                              # 4 r / N = oct + rem / N
    octant = eighths // N
    rem = eighths - octant * N
    odd = (octant & 1).astype(bool)
    rr = np.where(odd, N - rem, rem).astype(np.longdouble)
    pi = np.arctan2(np.longdouble(0), np.longdouble(-1))
    th = rr / np.longdouble(N) * (pi / np.longdouble(4))
    cc, ss = np.cos(th), np.sin(th)
    half = np.sqrt(np.longdouble(0.5))
    exact = rem == 0                                             # a multiple of an eighth of a turn
    cc = np.where(exact, np.where(odd, half, np.longdouble(1)), cc)
    ss = np.where(exact, np.where(odd, half, np.longdouble(0)), ss)
    cc, ss = np.where(odd & ~exact, ss, cc), np.where(odd & ~exact, cc, ss)
    quarter = octant >> 1
    C = np.select([quarter == 0, quarter == 1, quarter == 2], [cc, -ss, -cc], ss)
    S = np.select([quarter == 0, quarter == 1, quarter == 2], [ss, cc, -ss], -cc)
    c = (C - 1j * S).astype(np.clongdouble)                      # the negative angle
    c = c if long else c.astype(np.complex128)
    c.setflags(write=False)
    return c


def chirp(N, dtype=np.complex128):
    """c[k] = exp(-i pi k^2 / N), k = 0 .. N-1, as csrc/fid_chirp.h makes it: k^2 reduced mod 2 N exactly, folded to an
    octant, cos and sin in long double; fp64 is the rounding of that.  Read-only (cached)."""
    return _chirp_cached(int(N), np.dtype(dtype) == np.clongdouble)


def _times(a, b):
    """The complex product by its parts, each rounded once: (a c - b d, a d + b c)."""
    out = np.empty(np.broadcast(a, b).shape, dtype=np.result_type(a, b))
    out.real = a.real * b.real - a.imag * b.imag
    out.imag = a.real * b.imag + a.imag * b.real
    return out


def bluestein_host(x, N):
    """include/nmrfit_amd_fid_any.h's definition step by step in numpy: Y (T, N) = fftshift(fft(x, N)) of every trace of x
    (n_in' <= N points) by the chirp-z transform -- a = x' c zero filled to M, b the wrapped conj(c), P = fft(a) fft(b),
    p = fft(P)[(-j) mod M] / M, X = p c, Y[i] = X[(i + N - N // 2) mod N].  fp64 for a complex128 input (the mirror of the
    device's steps; np.fft's transforms are not the device's bit for bit), long double for a clongdouble one (the truth)."""
    x = _as_traces(x, keep_long=True)
    long = x.dtype == np.clongdouble
    real = np.longdouble if long else np.float64
    N, n_in = int(N), x.shape[-1]
    if N < 1 or n_in > N:
        raise ValueError("fid: bluestein_host needs N >= the trace's length (%d, got N = %d)" % (n_in, N))
    c = chirp(N, x.dtype)
    M = conv_length(N)
    a = np.zeros((x.shape[0], M), dtype=x.dtype)
    a[:, :n_in] = _times(x, c[:n_in])
    b = np.zeros(M, dtype=x.dtype)
    b[:N] = np.conj(c)
    b[M - np.arange(1, N)] = np.conj(c[1:])
    P = _times(np.fft.fft(a, axis=-1), np.fft.fft(b))
    p = np.fft.fft(P, axis=-1)[:, (-np.arange(M)) % M] / real(M)          # the inverse transform by the forward one
    X = _times(p[:, :N], c)
    return X[:, (np.arange(N) + N - N // 2) % N]


@functools.lru_cache(maxsize=64)
def filter_peak(N):
    """beta = max_k |B[k]| of the definition, B = fft_M(b), in long double (a property of the definition, for the error
    bound of the header).  Cached: a transform of M points in long double per distinct N."""
    c = chirp(N, np.clongdouble)
    M = conv_length(N)
    b = np.zeros(M, dtype=np.clongdouble)
    b[:N] = np.conj(c)
    b[M - np.arange(1, N)] = np.conj(c[1:])
    return float(np.abs(np.fft.fft(b)).max())


def _first_point(W, first_point):
    W[0] = W[0] * first_point
    return W


def window_em(n, lb, sw, first_point=1.0):
    """Exponential multiplication: W[j] = exp(-pi lb j / sw), j = 0 .. n-1 (lb: line broadening in Hz, sw: spectral width
    in Hz, so j / sw is the time of point j).  W[0] is multiplied by ``first_point``."""
    return _first_point(np.exp(-np.pi * float(lb) * np.arange(int(n)) / float(sw)), first_point)


def window_gauss(n, gb, sw, first_point=1.0):
    """Gaussian: W[j] = exp(-(pi gb j / sw)^2 / (4 ln 2)): a line of gb Hz full width at half height in the spectrum."""
    return _first_point(np.exp(-(np.pi * float(gb) * np.arange(int(n)) / float(sw)) ** 2 / (4.0 * np.log(2.0))), first_point)


def window_sine(n, off=0.0, end=1.0, power=1.0, first_point=1.0):
    """Sine bell: W[j] = sin(pi off + pi (end - off) j / (n - 1)) ** power (off = 0.5, power = 2: the squared cosine)."""
    n = int(n)
    j = np.arange(n) / max(n - 1, 1)
    return _first_point(np.sin(np.pi * float(off) + np.pi * (float(end) - float(off)) * j) ** float(power), first_point)


# -- the device call -----------------------------------------------------------------------------------------------

def _calls(values, shared=None):
    """(first, last + 1) of consecutive spectra per library call: at most 65535 spectra and MAX_VALUES values.
    ``shared``: per spectrum None or (key, values) -- values counted once per distinct key of a call (the chirp path's
    filter planes, once per distinct N)."""
    out, i0, acc, keys = [], 0, 0, set()
    for i, val in enumerate(values):
        key, extra = shared[i] if shared is not None and shared[i] is not None else (None, 0)
        if i > i0 and (acc + val + (0 if key in keys else extra) > MAX_VALUES or i - i0 == _cabi._MAX_SPECTRA_PER_CALL):
            out.append((i0, i))
            i0, acc, keys = i, 0, set()
        if key is not None and key not in keys:
            keys.add(key)
            acc += extra
        acc += val
    if len(values):
        out.append((i0, len(values)))
    return out


def _per_fid(value, K, what, scalar):
    """``value`` as a list of K entries: None, one value (``scalar(value)`` says so) or one per FID."""
    if value is None:
        return [None] * K
    if scalar(value):
        return [value] * K
    value = list(value)
    if len(value) != K:
        raise ValueError("fid: %s is one value or one per FID (got %d for %d FIDs)" % (what, len(value), K))
    return value


def _is_one_window(window):
    """One window (a 1-D array, or a sequence of numbers) and not a sequence of windows."""
    if isinstance(window, np.ndarray):
        return window.ndim == 1 and window.dtype != object
    return len(window) > 0 and all(w is not None and np.ndim(w) == 0 for w in window)


def _conditioning(xs, grpdly, grpdly_mode, window, truncate_grpdly):
    """Per FID (form, g, n_in', index of its window or -1), and the distinct windows of the call (equal contents are one
    window).  Every argument error is raised here, before the library."""
    K = len(xs)
    modes = _per_fid(grpdly_mode, K, "grpdly_mode", lambda v: isinstance(v, str))
    gs = _per_fid(grpdly, K, "grpdly", lambda v: np.ndim(v) == 0)
    ws = _per_fid(window, K, "window", _is_one_window)
    jobs, windows, seen = [], [], {}
    for k, x in enumerate(xs):
        s, form = x.shape[1], _mode(modes[k])
        g = None if gs[k] is None else grpdly_value(gs[k], truncate_grpdly)
        if g is not None and form == FORM_FID and (s < 2 or s & (s - 1) or s > 1 << MAX_LOG2):
            raise ValueError("fid: grpdly_mode='fid' needs a trace length that is a power of two, 2 .. 2^%d (FID %d has %d "
                             "points): pass grpdly_mode='spectrum'" % (MAX_LOG2, k, s))
        n_out = conditioned_length(s, g, modes[k])
        at = -1
        if ws[k] is not None:
            W = np.ascontiguousarray(ws[k], dtype=np.float64)
            if W.shape != (n_out,):
                raise ValueError("fid: a window has as many values as the conditioned trace has points (FID %d: %d, got shape %r)"
                                 % (k, n_out, W.shape))
            if not np.isfinite(W).all():
                raise ValueError("fid: a window value is not finite (FID %d)" % k)
            key = W.tobytes()
            if key not in seen:
                seen[key] = len(windows)
                windows.append(W)
            at = seen[key]
        jobs.append((FORM_NONE if g is None else form, 0.0 if g is None else g, n_out, at))
    return jobs, windows


def transform_many(fids, zero_fill=None, device=0, return_transform=False, grpdly=None, grpdly_mode="fid", window=None,
                   truncate_grpdly=True, return_conditioned=False, any_length=False):
    """The spectra of K FIDs on the GPU (nmrfit_fid_transform).  Each FID is a complex64 or complex128 array of shape
    (n,) or (T, n): T traces that are summed after the normalisation, as ``core.load`` does.  ``zero_fill``: None (the
    transform length is the trace's), "pow2" (the next power of two) or an int; the zeros are made on the device.
    Returns per FID ``(u, v, row)`` -- fp64 arrays in ``Data``'s order and the library's row (status, Re m, Im m, the
    flat index of m in Y, n, T; status 0 transformed, 1 all-zero FID, 2 not finite: u and v are NaN then) -- plus
    ``Y`` of shape (T, n), the centred transform of every trace, when ``return_transform``.  A length the device
    refuses raises ValueError (see ``zero_fill``); there is no host fallback.  Lists of any length are cut into library
    calls of at most 65535 spectra and 2^26 transformed values.

    Conditioning on the device, in the same call (nmrfit_fid_condition_transform; the module docstring has the
    definition).  ``grpdly``: None, a Bruker group delay (the GRPDLY parameter; the DSPFVS / DECIM table of old firmware is
    not looked up) or one per FID (None entries: no removal), rounded to one decimal unless ``truncate_grpdly=False``.
    ``grpdly_mode``: "fid" (what ``core.load`` does; the trace length must be a power of two and the conditioned trace
    has floor(g + 2) points fewer, so it needs ``zero_fill``) or "spectrum" (any length; a ramp on the spectrum), or one
    of the two per FID.
    ``window``: None, n_in' reals (``window_em`` and the others; ``conditioned_length`` gives n_in'), or one per FID; equal
    windows are uploaded once.  ``return_conditioned``: the traces as they enter the main transform, (T, n_in'), last in
    the tuple.  With all of these left alone the call is the one made before they existed.

    ``any_length=True``: a transform length that is not a power of two (3 .. 2^21 - 1) is transformed at exactly that
    length on the device (nmrfit_fid_transform_any; the module docstring); ``grpdly_mode="fid"`` then needs no
    ``zero_fill``.  "spectrum" with such a length stays refused.  A call's values then count 2 T M per such FID and 2 M per
    distinct such length as well (M = ``conv_length(n)``).  Powers of two go the way they went, with the same bits."""
    xs = [_as_traces(f) for f in fids]
    plain = grpdly is None and window is None and not return_conditioned
    if plain:
        conds, windows = [(FORM_NONE, 0.0, x.shape[1], -1) for x in xs], []
    else:
        conds, windows = _conditioning(xs, grpdly, grpdly_mode, window, truncate_grpdly)
    ns = [transform_length(c[2], zero_fill, any_length) for c in conds]
    chirped = [not _is_pow2(n) for n in ns]                      # (any_length alone lets such a length through)
    for k, c in enumerate(conds):
        if chirped[k] and c[0] == FORM_SPECTRUM:
            raise ValueError("fid: grpdly_mode='spectrum' needs a transform length that is a power of two (FID %d: %d): pass "
                             "zero_fill, or grpdly_mode='fid'" % (k, ns[k]))
    values = [x.shape[0] * (n + (x.shape[1] if c[0] == FORM_FID else 0) + (2 * conv_length(n) if ch else 0))
              for x, n, c, ch in zip(xs, ns, conds, chirped)]
    shared = [(n, 2 * conv_length(n)) if ch else None for n, ch in zip(ns, chirped)]
    for k, val in enumerate(values):
        if shared[k] is not None:
            val += shared[k][1]
        if val > MAX_VALUES:
            raise ValueError("fid: T n = %d exceeds %d values per call (FID %d): a smaller zero_fill, or fewer traces"
                             % (val, MAX_VALUES, k))
    lib = _cabi.lib() if xs else None
    result = []
    for i0, i1 in _calls(values, shared):
        sel = range(i0, i1)
        by_chirp = any(chirped[k] for k in sel)
        K = len(sel)
        n_in = np.array([xs[k].shape[1] for k in sel], dtype=np.int64)
        n = np.array([ns[k] for k in sel], dtype=np.int64)
        T = np.array([xs[k].shape[0] for k in sel], dtype=np.int32)
        flat = np.concatenate([xs[k].ravel() for k in sel]).view(np.float64)
        u, v = np.empty(int(n.sum())), np.empty(int(n.sum()))
        rows = np.empty(K * ROW)
        Z = np.empty(2 * int((T * n).sum())) if return_transform else None
        if plain and not by_chirp:
            _cabi.check(lib.nmrfit_fid_transform(int(device), K, _cabi.ptr(n_in), _cabi.ptr(n), _cabi.ptr(T), _cabi.ptr(flat),
                                                 _cabi.ptr(u), _cabi.ptr(v), _cabi.ptr(rows), _cabi.ptr(Z)))
        else:
            call = lib.nmrfit_fid_transform_any if by_chirp else lib.nmrfit_fid_condition_transform
            form = np.array([conds[k][0] for k in sel], dtype=np.int32)
            g = np.array([conds[k][1] for k in sel], dtype=np.float64)
            n_out = np.array([conds[k][2] for k in sel], dtype=np.int64)
            used = sorted({conds[k][3] for k in sel} - {-1})              # the windows of THIS library call
            window_of = np.array([used.index(conds[k][3]) if conds[k][3] >= 0 else -1 for k in sel], dtype=np.int32)
            window_len = np.array([len(windows[m]) for m in used], dtype=np.int64)
            wflat = np.concatenate([windows[m] for m in used]) if used else None
            C = np.empty(2 * int((T * n_out).sum())) if return_conditioned else None
            _cabi.check(call(
                int(device), K, _cabi.ptr(n_in), _cabi.ptr(n), _cabi.ptr(T), _cabi.ptr(flat), _cabi.ptr(form), _cabi.ptr(g),
                _cabi.ptr(window_of), len(used), _cabi.ptr(window_len) if used else None, _cabi.ptr(wflat), _cabi.ptr(u),
                _cabi.ptr(v), _cabi.ptr(rows), _cabi.ptr(Z), _cabi.ptr(C)))
            coff = np.concatenate(([0], np.cumsum(T * n_out)))
        rows = rows.reshape(K, ROW)
        off = np.concatenate(([0], np.cumsum(n)))
        zoff = np.concatenate(([0], np.cumsum(T * n)))
        for i in range(K):
            one = (u[off[i]:off[i + 1]], v[off[i]:off[i + 1]], rows[i].copy())      # (u, v: views of the call's arrays)
            if return_transform:
                # (the library returns every trace in the output order: Y_t[i] is entry n - 1 - i)
                z = Z[2 * zoff[i]:2 * zoff[i + 1]].view(np.complex128).reshape(int(T[i]), int(n[i]))
                one += (z[:, ::-1].copy(),)
            if return_conditioned:
                one += (C[2 * coff[i]:2 * coff[i + 1]].view(np.complex128).reshape(int(T[i]), int(n_out[i])),)
            result.append(one)
    return result


def spectra_from_fids(fids, sw, sfrq, tof, zero_fill=None, device=0, grpdly=None, grpdly_mode="fid", window=None,
                      truncate_grpdly=True, any_length=False):
    """``core.load`` without the file reader, for many FIDs at once: a list of ``Data(w, u, v)`` with (u, v) from
    ``transform_many`` and ``w = ppm_axis(n, sw, sfrq, tof)``, ready for ``shift_phase_many`` / ``select_peaks_many`` /
    ``fit_many``.  ``sw``, ``sfrq``, ``tof`` (Hz, MHz, Hz): scalars or one value per FID.  ``grpdly``, ``grpdly_mode``,
    ``window``, ``truncate_grpdly``: the conditioning of ``transform_many`` (a Bruker FID: ``grpdly=<GRPDLY>``); ``any_length``:
    its exact-length transform (the grid ``core.load`` makes: no ``zero_fill`` needed).  A FID whose
    transform is not finite, or that is all zero, raises ValueError (nothing is returned)."""
    from .containers import Data

    def per_spectrum(value, K, what):
        if np.ndim(value) == 0:
            return [value] * K
        if len(value) != K:
            raise ValueError("spectra_from_fids: %s is one value or one per FID" % what)
        return list(value)
    fids = list(fids)
    K = len(fids)
    sws, sfrqs, tofs = (per_spectrum(x, K, name) for x, name in ((sw, "sw"), (sfrq, "sfrq"), (tof, "tof")))
    got = transform_many(fids, zero_fill=zero_fill, device=device, grpdly=grpdly, grpdly_mode=grpdly_mode, window=window,
                         truncate_grpdly=truncate_grpdly, any_length=any_length)
    for k, (_, _, row) in enumerate(got):
        if row[0] != OK:
            raise ValueError("spectra_from_fids: FID %d %s" % (k, "is all zero" if row[0] == ZERO else "has a transform that is not finite"))
    return [Data(ppm_axis(len(u), float(sws[k]), float(sfrqs[k]), float(tofs[k])), u, v) for k, (u, v, _) in enumerate(got)]

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

A caller who wants apodisation multiplies the FID first; Bruker's digital-filter removal is not done.  A complex64 FID
is widened exactly to fp64 on the host and the output is fp64: the reference's Varian path rounds the transform to
complex64 (nmrglue's cast), which is not reproduced.
"""
import numpy as np

from . import _cabi

ROW = 6                  # doubles per row (NMRFIT_FID_ROW): status, Re m, Im m, flat index of m, n, T
MAX_LOG2 = 22            # NMRFIT_FID_MAX_LOG2
LDS_LOG2 = 12            # NMRFIT_FID_LDS_LOG2: the longest transform that is one LDS-resident block
MAX_VALUES = 1 << 26     # T n summed over the spectra of one library call
OK, ZERO, NOT_FINITE = 0, 1, 2


def ppm_axis(n, sw, sfrq, tof):
    """``core.load``'s grid as ``Data`` holds it: ``np.linspace(sw/sfrq - tof/sfrq, -tof/sfrq, n)[::-1]`` (sw: spectral
    width in Hz, sfrq: spectrometer frequency in MHz, tof: transmitter offset in Hz)."""
    rangeppm, offsetppm = sw / sfrq, tof / sfrq
    return np.linspace(rangeppm - offsetppm, -offsetppm, n)[::-1]


def _as_traces(fid):
    """A FID as a contiguous (T, n_in) complex128 array (complex64 widens exactly)."""
    a = np.asarray(fid)
    if a.dtype not in (np.complex64, np.complex128):
        raise ValueError("fid: a FID is a complex64 or complex128 array (got %s)" % a.dtype)
    if a.ndim not in (1, 2) or a.shape[-1] == 0 or a.shape[0] == 0:
        raise ValueError("fid: a FID has shape (n,) or (T, n) with n, T > 0 (got %r)" % (a.shape,))
    return np.ascontiguousarray(a.reshape(-1, a.shape[-1]), dtype=np.complex128)


def transform_length(n_in, zero_fill=None):
    """The transform length of a trace of n_in points: n_in itself (None), the next power of two ("pow2"), or the int
    given.  ValueError, naming ``zero_fill``, for a length the device refuses."""
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


# -- the device call -----------------------------------------------------------------------------------------------

def _calls(values):
    """(first, last + 1) of consecutive spectra per library call: at most 65535 spectra and MAX_VALUES values."""
    out, i0, acc = [], 0, 0
    for i, val in enumerate(values):
        if i > i0 and (acc + val > MAX_VALUES or i - i0 == _cabi._MAX_SPECTRA_PER_CALL):
            out.append((i0, i))
            i0, acc = i, 0
        acc += val
    if len(values):
        out.append((i0, len(values)))
    return out


def transform_many(fids, zero_fill=None, device=0, return_transform=False):
    """The spectra of K FIDs on the GPU (nmrfit_fid_transform).  Each FID is a complex64 or complex128 array of shape
    (n,) or (T, n): T traces that are summed after the normalisation, as ``core.load`` does.  ``zero_fill``: None (the
    transform length is the trace's), "pow2" (the next power of two) or an int; the zeros are made on the device.
    Returns per FID ``(u, v, row)`` -- fp64 arrays in ``Data``'s order and the library's row (status, Re m, Im m, the
    flat index of m in Y, n, T; status 0 transformed, 1 all-zero FID, 2 not finite: u and v are NaN then) -- plus
    ``Y`` of shape (T, n), the centred transform of every trace, when ``return_transform``.  A length the device
    refuses raises ValueError (see ``zero_fill``); there is no host fallback.  Lists of any length are cut into library
    calls of at most 65535 spectra and 2^26 transformed values."""
    xs = [_as_traces(f) for f in fids]
    ns = [transform_length(x.shape[1], zero_fill) for x in xs]
    values = [x.shape[0] * n for x, n in zip(xs, ns)]
    for k, val in enumerate(values):
        if val > MAX_VALUES:
            raise ValueError("fid: T n = %d exceeds %d values per call (FID %d): a smaller zero_fill, or fewer traces"
                             % (val, MAX_VALUES, k))
    lib = _cabi.lib() if xs else None
    result = []
    for i0, i1 in _calls(values):
        sel = range(i0, i1)
        K = len(sel)
        n_in = np.array([xs[k].shape[1] for k in sel], dtype=np.int64)
        n = np.array([ns[k] for k in sel], dtype=np.int64)
        T = np.array([xs[k].shape[0] for k in sel], dtype=np.int32)
        flat = np.concatenate([xs[k].ravel() for k in sel]).view(np.float64)
        u, v = np.empty(int(n.sum())), np.empty(int(n.sum()))
        rows = np.empty(K * ROW)
        Z = np.empty(2 * sum(values[k] for k in sel)) if return_transform else None
        _cabi.check(lib.nmrfit_fid_transform(int(device), K, _cabi.ptr(n_in), _cabi.ptr(n), _cabi.ptr(T), _cabi.ptr(flat),
                                             _cabi.ptr(u), _cabi.ptr(v), _cabi.ptr(rows), _cabi.ptr(Z)))
        rows = rows.reshape(K, ROW)
        off = np.concatenate(([0], np.cumsum(n)))
        zoff = np.concatenate(([0], np.cumsum(T * n)))
        for i in range(K):
            one = (u[off[i]:off[i + 1]], v[off[i]:off[i + 1]], rows[i].copy())      # (u, v: views of the call's arrays)
            if return_transform:
                # (the library returns every trace in the output order: Y_t[i] is entry n - 1 - i)
                z = Z[2 * zoff[i]:2 * zoff[i + 1]].view(np.complex128).reshape(int(T[i]), int(n[i]))
                one += (z[:, ::-1].copy(),)
            result.append(one)
    return result


def spectra_from_fids(fids, sw, sfrq, tof, zero_fill=None, device=0):
    """``core.load`` without the file reader, for many FIDs at once: a list of ``Data(w, u, v)`` with (u, v) from
    ``transform_many`` and ``w = ppm_axis(n, sw, sfrq, tof)``, ready for ``shift_phase_many`` / ``select_peaks_many`` /
    ``fit_many``.  ``sw``, ``sfrq``, ``tof`` (Hz, MHz, Hz): scalars or one value per FID.  A FID whose transform is not
    finite, or that is all zero, raises ValueError (nothing is returned)."""
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
    got = transform_many(fids, zero_fill=zero_fill, device=device)
    for k, (_, _, row) in enumerate(got):
        if row[0] != OK:
            raise ValueError("spectra_from_fids: FID %d %s" % (k, "is all zero" if row[0] == ZERO else "has a transform that is not finite"))
    return [Data(ppm_axis(len(u), float(sws[k]), float(sfrqs[k]), float(tofs[k])), u, v) for k, (u, v, _) in enumerate(got)]

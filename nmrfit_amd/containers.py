"""
Host mirror of the reference's ``Data`` container (nmrfit/containers.py:8-252) for scripted,
non-interactive use: it carries (w, u, v), the phase estimate and the picked peaks from which
the swarm box and the weights of the hot path are derived.

    data = Data(w, u, v)
    data.shift_phase(method='auto')              # ACME estimate -> p0, p1, V, I
    data.select_bounds(low=3.0, high=4.0)        # crop
    data.select_peaks(method='auto', thresh=0.1, window=0.02)
    lower, upper = data.generate_solution_bounds()
    fit = nmrfit_amd.fit(data, lower, upper)

Kept from the reference: attribute names (w, u, v, V, I, p0, p1, peaks, roibounds), method names,
arguments, defaults and error messages.  Not kept: everything that opens a matplotlib window --
``plot=True``, ``select_bounds()`` without low/high and ``select_peaks(method='manual')`` raise
NotImplementedError (GUI selectors are out of scope).  ``nmrfit.load``
(Varian/Bruker files through nmrglue) is out of scope too: build a Data from arrays.
"""
import numpy as np

from . import peaks as _peaks
from . import proc_autophase
from . import utils


def _no_gui(what):
    raise NotImplementedError(what + " opens a matplotlib window in the reference; interactive selectors and "
                              "plots are out of scope here")


class Data:
    def __init__(self, w, u, v):
        self.w = w
        self.u = u
        self.v = v
        self.V = self.u[:]
        self.I = self.v[:]

    def shift_phase(self, method='auto', p0=0.0, p1=0.0, step=np.pi / 360, plot=False):
        """Set p0, p1 (radians) and the phase-corrected V, I (containers.py:51-96):
        'manual' takes p0, p1 as given, 'auto' minimises the ACME score, 'brute' scans p0."""
        choice = method.lower()
        if choice == 'manual':
            self.p0, self.p1 = p0, p1
        elif choice == 'auto':
            self.p0, self.p1 = proc_autophase.approximate_phase(self.u + 1j * self.v, 'acme')
        elif choice == 'brute':
            self.p0, self.p1 = self._brute_phase(step=step)
        else:
            raise ValueError("Method must be 'auto', 'brute', or 'manual'.")
        self.V, self.I = proc_autophase.ps2(self.u, self.v, self.p0, self.p1)
        if plot is True:
            _no_gui("shift_phase(plot=True)")

    def _brute_phase(self, step=np.pi / 360):
        """Scan p0 over [-pi, pi) (p1 = 0): keep the angle that best levels the two ends of the
        real part while the spectrum stays upright (containers.py:98-110).  Like the reference it
        leaves V, I at the LAST angle scanned; shift_phase recomputes them."""
        best_p0, best_err = 0, np.inf
        n = max(1, int(len(self.V) / 5000))
        for angle in np.arange(-np.pi, np.pi, step):
            self.V, self.I = proc_autophase.ps2(self.u, self.v, angle, 0.0)
            err = np.sqrt((self.V[:n].mean() - self.V[-n:].mean()) ** 2)
            if err < best_err and np.max(self.V) > abs(np.min(self.V)):
                best_p0, best_err = angle, err
        return best_p0, 0.0

    def select_bounds(self, low=None, high=None):
        """Crop w, u, v to low < w < high (containers.py:112-130).  V and I are NOT cropped, as in
        the reference: call shift_phase again afterwards."""
        if low is None or high is None:
            _no_gui("select_bounds() without low and high")
        self.w, self.u, self.v = _peaks.BoundsSelector(self.w, self.u, self.v, supress=True).apply_bounds(low=low, high=high)

    def select_peaks(self, method='auto', n=None, one_click=False, thresh=0.0, window=0.02, plot=False):
        """Pick peaks on (w, V) (containers.py:132-173); sets ``peaks`` and ``roibounds``."""
        choice = method.lower()
        if choice == 'manual':
            if isinstance(n, int) and n > 0:
                _no_gui("select_peaks(method='manual')")
            raise ValueError("Number of peaks must be specified when using 'manual' flag")
        if choice != 'auto':
            raise ValueError("Method must be 'auto' or 'manual'.")
        selector = _peaks.AutoPeakSelector(self.w, self.V, thresh=thresh, window=window)
        selector.find_peaks()
        if plot is True:
            _no_gui("select_peaks(plot=True)")
        self.peaks = selector.peaks
        self.roibounds = [p.bounds for p in self.peaks]

    def generate_solution_bounds(self, force_p0=False, force_p1=False):
        """(lower, upper) lists of the 4 + 3P parameter bounds (containers.py:175-217)."""
        return utils.generate_solution_bounds(self.peaks, p0=getattr(self, "p0", 0.0), p1=getattr(self, "p1", 0.0),
                                              force_p0=force_p0, force_p1=force_p1)

    def approximate_areas(self):
        return [p.area for p in self.peaks]

    def approximate_area_fraction(self):
        """Satellite share of the total approximate area: peaks below the mean area are satellites."""
        areas = np.array(self.approximate_areas())
        mean = np.mean(areas)
        main = areas[areas >= mean].sum()
        sats = areas[areas < mean].sum()
        return sats / (main + sats)


def shift_phase_many(datas, method='auto', p0=0.0, p1=0.0, step=np.pi / 360, device=0):
    """``for d in datas: d.shift_phase(method, p0, p1, step)`` with the phase search of all of them on the GPU (opt-in;
    Data.shift_phase stays the host path).  Sets p0, p1 (radians) and V, I on every object with ``u``, ``v``:
    'auto' runs the ACME optimisation of every spectrum in one launch (from (0, 0), as shift_phase does), 'brute' the
    level test of every angle of np.arange(-pi, pi, step) for every spectrum in one launch and keeps the first strict
    minimum in the reference's loop order, 'manual' takes p0, p1 as given.  V and I come from the host ps2, bit-identical
    to shift_phase for the same p0, p1.  u and v are phased in float64 (float32 input too).

    'brute' picks the host loop's angle exactly where numpy's complex multiply runs its FMA loop (x86-64 with AVX2 or
    AVX-512; the device rounds the rotation as that loop does, proc_autophase.brute_levels).  Its mean length is the
    host's, n = max(1, int(len(d.V) / 5000)) from the V the object holds before the scan: select_bounds crops u, v but
    leaves V, so on a cropped Data n comes from the uncropped length (or from the u of the last shift_phase), not from
    len(u).  It refuses a mean length above 128, len(V) >= 645000 (NmrfitError: longer means would take numpy's
    recursive pairwise order).  Any number of spectra: the library takes at most 65535 per call and the list is cut
    into such calls."""
    datas = list(datas)
    choice = method.lower()
    if choice == 'manual':
        ps = [(p0, p1)] * len(datas)
    elif choice == 'auto':
        x = proc_autophase.estimate_many([np.asarray(d.u, dtype=np.float64) + 1j * np.asarray(d.v, dtype=np.float64)
                                          for d in datas], 'acme', device=device)[0]
        ps = [(a * np.pi / 180, b * np.pi / 180) for a, b in x]
    elif choice == 'brute':
        angles = np.arange(-np.pi, np.pi, step)
        n = [max(1, int(len(d.V) / 5000)) for d in datas]        # (Data._brute_phase: before its scan)
        err = proc_autophase.brute_levels([d.u for d in datas], [d.v for d in datas], angles, device=device, n=n)
        ps = []
        for row in err:
            ok = row < np.inf                      # (NaN: not upright; the host loop's `err < best_err` is False there)
            ps.append((angles[np.flatnonzero(row == row[ok].min())[0]] if ok.any() else 0, 0.0))
    else:
        raise ValueError("Method must be 'auto', 'brute', or 'manual'.")
    for d, (a, b) in zip(datas, ps):
        d.p0, d.p1 = a, b
        d.V, d.I = proc_autophase.ps2(d.u, d.v, d.p0, d.p1)
    return datas


def select_peaks_many(datas, method='auto', thresh=0.0, window=0.02, device=0):
    """``for d in datas: d.select_peaks(method, thresh=thresh, window=window)`` with the picking of all of them on the
    GPU (opt-in; Data.select_peaks stays the host path): peaks.find_peaks_many on every (d.w, d.V).  Sets ``peaks`` and
    ``roibounds``.  ``thresh`` and ``window``: scalars or one value per object.  'manual' and unknown methods raise
    what Data.select_peaks raises; a Data cropped by select_bounds and not re-phased (len(w) != len(V)) raises
    ValueError, as interp1d does on the host.  Every error comes before any device work."""
    datas = list(datas)
    choice = method.lower()
    if choice == 'manual':
        raise ValueError("Number of peaks must be specified when using 'manual' flag")
    if choice != 'auto':
        raise ValueError("Method must be 'auto' or 'manual'.")
    found = _peaks.find_peaks_many([d.w for d in datas], [d.V for d in datas], thresh=thresh, window=window,
                                   device=device)
    for d, p in zip(datas, found):
        d.peaks = p
        d.roibounds = [q.bounds for q in p]
    return datas


def correct_baseline_many(datas, deg=1, exclude=None, margin=1.0, device=0):
    """Fit a polynomial baseline of degree ``deg`` to the channels V and I of every Data, outside its peaks, on the GPU
    (baseline.fit_many, csrc/baseline.hip: a conditioned basis, a fixed summation order) and take it out: sets NEW
    arrays ``V``, ``I``, ``u, v = ps2(V, I, p0, p1, inv=True)`` and ``d.baseline`` (the pair of ``BaselineFit``, with the
    subtracted arrays in ``.baseline``).  The arrays the caller holds are never written in place.

    exclude : per Data a list of ``(lo, hi)`` in units of w that the fit leaves out; default: the bounds of its peaks,
        widened about their centres by ``margin``
    margin : the peaks' bounds are a few widths wide: +-2 FWHM still leaves 1/17 of a Lorentzian's height just outside
        them, and that tail is fitted as baseline.  A larger ``margin`` moves the fitted points further out (3: +-6 FWHM,
        under 1/145 of the height), at the price of fewer of them.

    ValueError if len(w) != len(V) (a Data cropped and not re-phased, as select_peaks_many), and -- before anything is
    written to any Data: all or nothing -- if any job could not be fitted (an empty mask, fewer points than
    coefficients), naming the spectrum."""
    from . import baseline
    datas = list(datas)
    for k, d in enumerate(datas):
        if not len(d.w) == len(d.V) == len(d.I):
            raise ValueError("correct_baseline_many: len(w) != len(V) (spectrum %d): call shift_phase after select_bounds" % k)
    if exclude is None:
        exclude = [baseline.widened([tuple(p.bounds) for p in getattr(d, "peaks", [])], margin) for d in datas]
    if len(exclude) != len(datas):
        raise ValueError("correct_baseline_many: one list of excluded intervals per spectrum")
    got = baseline.fit_many([d.w for d in datas], [np.array([d.V, d.I], dtype=np.float64) for d in datas], deg=deg,
                            intervals=list(exclude), complement=True, device=device, return_baseline=True)
    for k, pair in enumerate(got):
        for name, b in zip("VI", pair):
            if b.status != 0:
                raise ValueError("correct_baseline_many: channel %s of spectrum %d could not be fitted (status %d: %s; "
                                 "%d points outside the excluded intervals, degree %d)"
                                 % (name, k, b.status, "empty mask" if b.status == 1 else "rank", b.n, b.deg))
    for d, (bV, bI) in zip(datas, got):
        V = np.asarray(d.V, dtype=np.float64) - bV.baseline
        I = np.asarray(d.I, dtype=np.float64) - bI.baseline
        d.V, d.I = V, I
        d.u, d.v = proc_autophase.ps2(V, I, getattr(d, "p0", 0.0), getattr(d, "p1", 0.0), inv=True)
        d.baseline = (bV, bI)
    return datas

"""
Host-side mirror of the reference's fit driver (nmrfit/utils.py:96-339 ``FitUtility``):
same constructor, same attributes, same ``options`` keys -- the swarm loop and the objective
run on the MI355X instead of going through pyswarm one particle at a time.

Kept verbatim from the reference interface:
  FitUtility(data, lower, upper, expon=0.5, dynamic_weighting=True, fit_im=False,
             processes=1, summary=True, options={})
  attributes data, lower, upper, expon, dynamic_weighting, fit_im, summary, processes, options;
  after fit(): weights, params, error.
  options: swarmsize (204), maxiter (2000), omega (-0.2134), phip (-0.3344), phig (2.3259)
           (utils.py:177-181).  Extra opt-in keys: minstep, minfunc (pyswarm's 1e-8 defaults,
           which the reference does not forward), seed, device, check_every, polish,
           variant (kernel variant by name or number; default: "farfield" when grid x peaks
           >= 1e5, else "default" -- see default_variant; "farfield32" is the opt-in mixed-precision
           form of the far-field kernel, f within 5e-12 of it, 5 % faster at C3 size), exchange ("rccl" for a
           multi-GPU fit, one process per GPU: the swarm axis is sharded and the global best is
           exchanged by one RCCL all-gather per generation inside libnmrfit_amd.so).

``processes`` is accepted and ignored: the reference's only use of it is to spread the
per-particle objective calls (and the Kramers-Kronig quadratures of generate_result) over a
multiprocessing.Pool (utils.py:182, 259-261), which the batched launches replace.
``fit_im=True`` follows the reference to the letter (equations.py:197-209: the imaginary
model is the last peak's line only); ``fit_im="sum"`` fits the imaginary part of all peaks.
"""
import typing

import numpy as np

from . import _cabi, equations, proc_autophase, pso
from .peaks import (AutoPeakSelector, BoundsSelector, Peak, Peaks, find_peak, rnd_data,  # noqa: F401  (reference names:
                    sample_noise)                                                          # nmrfit.utils.<name>)


def compute_weights(w, peaks, expon=0.5):
    """The ``weights`` array of a fit: what FitUtility._compute_weights produces (nmrfit/utils.py:191-224),
    computed once per fit on the host as the reference does.

    Every peak claims the grid points between the two points nearest to its ``bounds``, at weight
    ``(tallest |height| / its |height|) ** expon``; where regions overlap the LAST peak in ``peaks`` wins (the
    reference assigns the slices in list order); unclaimed points weigh 1.  Ten Laplacian sweeps
    (``equations.laplace1d``) then round the steps off.  Here the claim is resolved for all peaks at once on a
    (peak, point) membership mask -- which peak owns a point is the highest peak index whose region holds it --
    and the weights are gathered through that owner index, instead of one slice assignment per peak."""
    grid = np.asarray(w, dtype=float)
    if len(peaks) == 0:
        return equations.laplace1d(np.ones(grid.size))
    edges = np.array([[pk.bounds[0], pk.bounds[1]] for pk in peaks], dtype=float)           # (P, 2)
    heights = np.abs(np.array([pk.height for pk in peaks], dtype=float))
    # nearest grid point to each region edge (first one on ties, like argmin), edges sorted per region
    nearest = np.abs(grid[None, None, :] - edges[:, :, None]).argmin(axis=2)
    first, last = nearest.min(axis=1), nearest.max(axis=1)
    # per-peak level: scalar power, one value per peak (numpy's array power may take a vectorised libm whose last
    # bit differs from the scalar one the reference's per-peak call goes through)
    top = heights.max()
    level = np.array([np.power(top / h, expon) for h in heights])
    j = np.arange(grid.size)
    member = (j[None, :] >= first[:, None]) & (j[None, :] <= last[:, None])                # (P, N)
    owner = len(peaks) - 1 - member[::-1].argmax(axis=0)                                   # highest claiming peak index
    weights = np.where(member.any(axis=0), level[owner], 1.0)
    return equations.laplace1d(weights)


# grid points a workgroup of the device's fill-and-smooth kernel owns (NMRFIT_WEIGHTS_TILE, include/nmrfit_amd_prep.h)
WEIGHTS_TILE = 1024


def weight_regions(w, peaks, expon=0.5):
    """The host half of ``compute_weights``, for the device form (``compute_weights_many``, ``FitBatch(regions=...)``):
    ``(edges[R, 2], level[R])`` -- every peak's bounds, and its level by the scalar power exactly as ``compute_weights``
    forms it.  The grid ``w`` enters on the device only (the nearest points, the fill, the sweeps; csrc/weights.hip); it
    is accepted here so that the call reads like ``compute_weights``.  No peaks: R = 0."""
    if len(peaks) == 0:
        return np.empty((0, 2)), np.empty(0)
    edges = np.array([[pk.bounds[0], pk.bounds[1]] for pk in peaks], dtype=float)           # (R, 2)
    heights = np.abs(np.array([pk.height for pk in peaks], dtype=float))
    top = heights.max()
    level = np.array([np.power(top / h, expon) for h in heights])
    return edges, level


def pack_regions(regions):
    """K entries ``(edges, level)`` -- or None: no regions, unit weights -- as the three arrays the library takes: the
    region counts ``R`` (int32, K), the bounds (float64, 2 sum R) and the levels (float64, sum R), fit after fit; a
    fit's regions start at ``np.cumsum(R)[k] - R[k]``."""
    R = np.zeros(len(regions), dtype=np.int32)
    edges, level = [np.empty(0)], [np.empty(0)]
    for k, reg in enumerate(regions):
        if reg is None:
            continue
        e, lv = _cabi.f64(reg[0]).reshape(-1, 2), _cabi.f64(reg[1]).ravel()
        if len(e) != len(lv):
            raise ValueError("regions: as many levels as pairs of bounds (entry %d)" % k)
        R[k] = len(lv)
        edges.append(e.ravel())
        level.append(lv)
    return R, np.concatenate(edges), np.concatenate(level)


def _weight_calls(Ns):
    """[k0, k1) ranges of at most 65535 spectra and 2^26 grid points (a lone spectrum above that is its own call; the
    library refuses it)."""
    k0, n = 0, len(Ns)
    while k0 < n:
        k1, pts = k0, 0
        while k1 < n and k1 - k0 < _cabi._MAX_SPECTRA_PER_CALL and (k1 == k0 or pts + Ns[k1] <= _cabi.WEIGHTS_MAX_POINTS):
            pts += Ns[k1]
            k1 += 1
        yield k0, k1
        k0 = k1


def compute_weights_many(ws, peaks_list, expon=0.5, device=0, return_pairs=False):
    """``compute_weights(w, peaks, expon)`` for many spectra on the GPU (nmrfit_weights_build, csrc/weights.hip): the
    list of weight arrays, each bit-identical to the host routine's, alone or in any batch.  The spectra may differ in
    length and in their number of peaks (none: all ones); ``w`` in any order; ``expon``: a scalar or one value per
    spectrum.  The levels are formed here (``weight_regions``), everything that touches the grid on the device.  Lists
    of any length are cut into library calls of at most 65535 spectra and 2^26 grid points.  ``return_pairs``: also the
    (R_k, 2) int64 arrays of every region's first and last grid index."""
    ws = [np.ascontiguousarray(np.asarray(w, dtype=float)).ravel() for w in ws]
    peaks_list = list(peaks_list)
    S = len(ws)
    if len(peaks_list) != S:
        raise ValueError("ws and peaks_list differ in length")
    ex = np.asarray(expon, dtype=float)
    if ex.ndim == 0:
        ex = np.full(S, float(ex))
    elif ex.shape != (S,):
        raise ValueError("expon must be a scalar or one value per spectrum (%d), got shape %s" % (S, ex.shape))
    regions = [weight_regions(w, pk, e) for w, pk, e in zip(ws, peaks_list, ex)]
    out, pairs = [], []
    lib = _cabi.lib()
    for k0, k1 in _weight_calls([len(w) for w in ws]):
        N = np.array([len(w) for w in ws[k0:k1]], dtype=np.int64)
        R, edges, level = pack_regions(regions[k0:k1])
        grid = np.concatenate(ws[k0:k1])
        weights = np.empty(grid.size)
        first_last = np.empty((int(R.sum()), 2), dtype=np.int64)
        _cabi.check(lib.nmrfit_weights_build(int(device), k1 - k0, _cabi.ptr(N), _cabi.ptr(grid), _cabi.ptr(R),
                                             _cabi.ptr(edges), _cabi.ptr(level), _cabi.ptr(weights),
                                             _cabi.ptr(first_last) if return_pairs else None))
        noff = np.concatenate(([0], np.cumsum(N)))
        roff = np.concatenate(([0], np.cumsum(R)))
        for k in range(k1 - k0):
            out.append(weights[noff[k]:noff[k + 1]])
            pairs.append(first_last[roff[k]:roff[k + 1]])
    return (out, pairs) if return_pairs else out


def default_variant(N, P, fit_im=False):
    """Kernel variant ``fit`` uses when options['variant'] is absent: the far-field form
    (distant peaks' Lorentzian tails through one shared expansion per 512-point chunk, values
    within 1e-14 of the direct kernel's) once there is enough grid x peaks for it to pay, the
    direct kernel below that.  The threshold was re-measured in round 4 with the final kernels at 204, 1024
    and 4096 particles (tools/archive/variant_threshold.py, per-generation time of the swarm loop, far-field /
    direct; profiles/r04/variant_threshold.txt):

        grid x peaks      204      1024     4096 particles
        4096 x 6          1.06     1.11     1.25
        4096 x 24         1.09     1.11     1.14      (short grid: few chunks, every peak near)
        8192 x 12         1.02     1.01     1.05
        16384 x 6         1.01     1.05     1.08
        16384 x 12        0.93     0.89     0.88
        8192 x 24         0.99     0.96     0.96
        32768 x 12        0.84     0.77     0.74
        65536 x 24        0.57     0.50     0.47

    i.e. the direct kernel wins everywhere below grid x peaks = 1e5 and the far-field kernel everywhere from 2e5
    on, for every swarm size: the rule stands.  The whole GPU test suite passes with either as the default of every
    context (NMRFIT_DEFAULT_VARIANT), and tests/test_gpu_parity.py::test_farfield_adversarial_spectra
    covers the spectra where no peak is far.  bench.py's headline is always measured on the direct
    kernel; its `fit_default` entry reports this one.

    ``fit_im="sum"`` (every peak's imaginary line): the same rule.  Up to round 5 the far-field kernel needed 190 VGPRs with
    the imaginary sums (two waves per SIMD: 3.0 ms at 4096 x 65536 x 24 against the direct kernel's 2.6) and was never
    selected; round 6 gave it the pair expansions with the imaginary model -- for the real and for the imaginary series --
    and a quarter-interval Dawson table (162 VGPRs, three waves, no scratch): 1.63 ms against 2.38 there, and per swarm
    generation far-field / direct (tools/variant_threshold_im.py, profiles/r06/variant_threshold_im.txt) 1.00-1.03 below
    grid x peaks = 1e5, 0.95-1.00 at 1e5, 0.94-0.99 at 2e5, 0.85-0.94 at 3.9e5, 0.70-0.74 at 65536 x 24."""
    return "farfield" if int(N) * int(P) >= 100000 else "default"


def generate_solution_bounds(peaks, p0=0.0, p1=0.0, force_p0=False, force_p1=False):
    """The parameter box of a fit, as Data.generate_solution_bounds lays it out (nmrfit/containers.py:175-217),
    in the parameter order of the objective (section a4: p0, p1, r, yoff, then width, loc, area per peak):

        p0, p1   [-pi, pi], or the estimate +- 0.001 when ``force_p0`` / ``force_p1`` is True
        r        [0, 1]            yoff  [-0.01, 0.01]
        width    [0.5, 1.5] x the peak's width
        loc      a tenth of the way from the peak's centre to either region bound
        area     [0.5, 1.5] x the peak's area

    Built as two (4 + 3P) arrays -- the per-peak block is one (P, 3) table per side -- and returned as the plain
    lists ``(lower, upper)`` the reference returns."""
    def phase_box(estimate, forced):
        return (estimate - 0.001, estimate + 0.001) if forced is True else (-np.pi, np.pi)
    head = np.array([phase_box(p0, force_p0), phase_box(p1, force_p1), (0.0, 1.0), (-0.01, 0.01)])   # (4, 2)
    if len(peaks) == 0:
        return head[:, 0].tolist(), head[:, 1].tolist()
    width = np.array([pk.width for pk in peaks], dtype=float)
    loc = np.array([pk.loc for pk in peaks], dtype=float)
    area = np.array([pk.area for pk in peaks], dtype=float)
    edge = np.array([[pk.bounds[0], pk.bounds[1]] for pk in peaks], dtype=float)           # (P, 2)
    sides = []
    for side, scale in ((0, 0.5), (1, 1.5)):
        block = np.stack([width * scale, loc - 0.1 * (loc - edge[:, side]), area * scale], axis=1)   # (P, 3)
        sides.append(np.concatenate([head[:, side], block.ravel()]).tolist())
    return sides[0], sides[1]


# A swarm generation costs at least one objective launch plus, sharded, one all-gather and one fold launch (~15-25 us of
# latency on xGMI whatever the payload): below this much work per rank and generation the exchange costs more than
# the shard saves, and the fit is FASTER on one GPU (the reference's default 204 x 4096 x 6 is 5e6 units, 11.7 us).
SMALL_SHARD_UNITS = 1.0e8


def small_shard_warning(S_local, N, P, world, rank=0):
    """Warn (rank 0, once per call) when options['exchange'] shards a swarm whose per-rank generation is shorter than
    the exchange it adds: independent fits scale across GPUs as REPLICAS -- ``nmrfit_amd.fit_many(jobs, shard=True)``
    gives each rank its own spectra and needs no collective (nmrfit/utils.py:182 is the reference's counterpart: a
    process pool over particles).  Returns True when the warning applies."""
    units = float(S_local) * float(N) * float(max(P, 1))
    if world <= 1 or units >= SMALL_SHARD_UNITS:
        return False
    if rank == 0:
        import warnings
        warnings.warn("nmrfit: sharding this swarm over %d GPUs leaves %.2g particle x point x peak units per rank and "
                      "generation (< %.0e): the per-generation exchange costs more than the shard saves, one GPU is "
                      "faster.  For many spectra use nmrfit_amd.fit_many(jobs, shard=True): the ranks fit different "
                      "spectra and exchange nothing." % (world, units, SMALL_SHARD_UNITS), RuntimeWarning, stacklevel=3)
    return True


class BatchKey(typing.NamedTuple):
    """What the fits of one device batch have in common (FitUtility._batch_key; core.fit_many groups by it)."""
    device: int
    variant: int
    maxiter: int
    check_every: int
    fit_im: int          # (the imaginary-channel mode, equations.fit_im_mode)


class FitUtility:
    """Interface used to perform a fit of the data (reference: nmrfit/utils.py:96)."""

    def __init__(self, data, lower, upper, expon=0.5, dynamic_weighting=True, fit_im=False, processes=1,
                 summary=True, options={}):
        self.data = data
        self.lower = lower
        self.upper = upper
        self.expon = expon
        self.dynamic_weighting = dynamic_weighting
        self.fit_im = fit_im
        self.summary = summary
        self.processes = processes
        self.options = options

    def _compute_weights(self):
        return compute_weights(self.data.w, self.data.peaks, self.expon)

    def _host_weights(self):
        weights = self._compute_weights()
        if self.dynamic_weighting is False:
            weights = np.ones_like(weights)
        return weights

    def __getattr__(self, name):
        # (only reached for an attribute that is missing.)  ``weights`` of a fit whose weights were built on the device
        # (core.fit_many(device_weights=True)), or that another rank made: the host routine on first access -- bit for
        # bit what the device plane held -- and kept from then on.
        if name == 'weights':
            self.weights = self._host_weights()
            return self.weights
        raise AttributeError("%r object has no attribute %r" % (type(self).__name__, name))

    def _device(self):
        """The GPU this process works on: options['device'] if given; else, with a ready
        pso.RcclExchange, the device its communicator lives on; else, in a multi-rank fit
        (options['exchange'] = "rccl" or another exchange object: one process per GPU), the launcher's
        LOCAL_RANK -- or device 0 when the launcher shows this rank one device only
        (HIP_VISIBLE_DEVICES / ROCR_VISIBLE_DEVICES isolation; rendezvous.pick_device, which
        raises when the two disagree any other way); else 0.  fit() and generate_result() use the
        same one."""
        device = self.options.get('device')
        exchange = self.options.get('exchange')
        if device is None and isinstance(exchange, pso.RcclExchange):
            device = exchange.ev.device
        if device is None and exchange is not None:
            import sys
            from . import rendezvous
            device, note = rendezvous.pick_device(_cabi.device_count())
            if note and not getattr(self, '_device_note_shown', False):
                sys.stderr.write("nmrfit: %s\n" % note)
                self._device_note_shown = True
        return 0 if device is None else int(device)

    def _plan(self, device_weights=False):
        """What fit() decides before anything touches the GPU (utils.py:164-181): the weights, the swarm's constants and
        size, the seed, the kernel variant.  Shared by fit() and by core.fit_many's device-batched path.
        ``device_weights`` (core.fit_many): the plan carries the fit's weight regions (``weight_regions``; none with
        ``dynamic_weighting=False``: unit weights) for a batch that builds its weights on the device, and ``weights`` is
        left to its first access."""
        if device_weights:
            self.__dict__.pop('weights', None)
            regions = weight_regions(self.data.w, self.data.peaks if self.dynamic_weighting is not False else (), self.expon)
        else:
            self.weights = self._host_weights()
        opt = self.options
        plan = dict(kw=dict(omega=opt.get('omega', pso.DEFAULTS['omega']), phip=opt.get('phip', pso.DEFAULTS['phip']),
                            phig=opt.get('phig', pso.DEFAULTS['phig']), minstep=opt.get('minstep', pso.DEFAULTS['minstep']),
                            minfunc=opt.get('minfunc', pso.DEFAULTS['minfunc'])),
                    swarmsize=opt.get('swarmsize', pso.DEFAULTS['swarmsize']),
                    maxiter=opt.get('maxiter', pso.DEFAULTS['maxiter']), check_every=opt.get('check_every', 64))
        seed = opt.get('seed')
        if seed is None:     # pyswarm draws from numpy's unseeded global RNG: do the equivalent
            seed = int(np.random.SeedSequence().generate_state(1, dtype=np.uint64)[0])
        self.seed = seed     # (extra attribute: the seed this fit ran with -- rank 0's in a multi-rank fit)
        plan['seed'] = seed
        if device_weights:
            plan['regions'] = regions
        # kernel variant: by name or number, default by problem size (default_variant above)
        n_peaks = (len(self.lower) - 4) // 3
        plan['n_peaks'] = n_peaks
        plan['variant'] = _cabi.variant_id(opt.get('variant', default_variant(len(self.data.w), n_peaks, self.fit_im)))
        return plan

    def _batch_key(self, plan):
        """The key under which core.fit_many may put this fit into a device batch with others (csrc/batch_create.hip: equal
        kernel variant, imaginary-channel mode, maxiter and check_every; grid lengths, peak counts and swarm sizes may
        differ) -- or None when it must run on its own."""
        opt = self.options
        mode = equations.fit_im_mode(self.fit_im)
        if opt.get('exchange') is not None:
            return None
        if plan['variant'] not in (_cabi.VARIANT_DEFAULT, _cabi.VARIANT_FARFIELD) or len(self.lower) > 400:
            return None
        return BatchKey(self._device(), plan['variant'], int(plan['maxiter']), int(plan['check_every']), mode)

    def _finish(self, xopt, fopt):
        self.params = xopt
        self.error = fopt
        if self.summary is True:
            self._print_summary()

    def fit(self, plan=None):
        """utils.py:164-189: weights, minimise, store params/error, optional summary.  (``plan``: what ``_plan()``
        returned for this fit, when the caller -- core.fit_many -- has made it already.)"""
        if plan is None:
            plan = self._plan()
        opt = self.options
        kw, swarmsize, maxiter, seed = plan['kw'], plan['swarmsize'], plan['maxiter'], plan['seed']
        # Multi-GPU fits (one process per GPU, every rank makes the same fit() call):
        # options['exchange'] = "rccl" builds the RCCL communicator from the launcher's
        # environment (RANK / WORLD_SIZE / LOCAL_RANK / MASTER_*; nmrfit_amd.rendezvous), or pass a
        # ready pso.RcclExchange (used as it is, fit after fit: a communicator serves any context of its
        # device) / an exchange object with the same interface (tests).
        exchange = opt.get('exchange')
        own_exchange = False
        if isinstance(exchange, str) and exchange.lower() != "rccl":
            raise ValueError("options['exchange'] must be \"rccl\" or an exchange object")
        device = self._device()

        ev = equations.Evaluator(self.data.w, self.data.u, self.data.v, self.weights, device=device)
        try:
            if isinstance(exchange, str):
                exchange = pso.RcclExchange(ev)
                own_exchange = True
            elif isinstance(exchange, pso.RcclExchange) and exchange.ev is not ev:
                # A ready communicator, made on another context of the same device (self._device() took the
                # exchange's): it serves this fit's swarm as it is -- the all-gather runs on the stream of the
                # swarm's own context (csrc/comm.hip), so ONE ncclCommInitRank covers fit after fit.  Collective,
                # like the fit itself: every rank passes its exchange object.
                if exchange.channel is None or not exchange.handle.value:
                    raise ValueError("options['exchange']: this RcclExchange has been closed")
            ev.set_fit_im(self.fit_im)     # True: the reference's imaginary term (equations.py:197-209)
            ev.set_variant(plan['variant'])
            if exchange is None or (exchange.world == 1 and not isinstance(exchange, pso.RcclExchange)):
                xopt, fopt = pso.pso(ev, self.lower, self.upper, swarmsize=swarmsize, maxiter=maxiter, seed=seed,
                                     check_every=plan['check_every'], verbose=True, **kw)
            else:
                # every rank must run the same swarm: rank 0's seed wins (an unseeded fit would
                # otherwise draw a different seed on every rank)
                seed = exchange.broadcast_seed(seed)
                self.seed = seed
                off, n = pso.shard(swarmsize, exchange.rank, exchange.world)
                small_shard_warning(n, len(self.data.w), plan['n_peaks'], exchange.world, rank=exchange.rank)
                sw = pso.DeviceSwarm(ev, self.lower, self.upper, swarmsize, offset=off, S_local=n, seed=seed, **kw)
                try:
                    xopt, fopt = pso.run_sharded(sw, exchange, maxiter, check_every=plan['check_every'],
                                                 verbose=True)
                finally:
                    sw.close()
            if opt.get('polish', False):
                # opt-in extension (no reference counterpart): trust-region least squares on the
                # batched residual kernel, started from the swarm's answer
                from . import lsq
                xopt, fopt, _ = lsq.polish(ev, xopt, self.lower, self.upper, fit_im=self.fit_im)
        finally:
            if own_exchange:
                exchange.close()
            ev.close()
        self._finish(xopt, fopt)

    def _polish(self, xopt, fopt, plan, jac="2-point"):
        """options['polish'] for a fit whose swarm ran in a device batch (core.fit_many): the same least-squares
        refinement fit() applies, on a context made like fit()'s (weights, kernel variant, imaginary-channel mode), so
        the polished answer is the lone call's bit for bit.  The trust-region iterations are scipy's, one fit at a time
        on the host (each Jacobian is one launch of D + 1 residual rows, or with ``jac="analytic"`` -- fit_many's
        ``polish_jac`` -- one pass of csrc/lsq_analytic.hip): they do not run in lock step across fits."""
        from . import lsq
        ev = equations.Evaluator(self.data.w, self.data.u, self.data.v, self.weights, device=self._device())
        try:
            ev.set_fit_im(self.fit_im)
            ev.set_variant(plan['variant'])
            xopt, fopt, _ = lsq.polish(ev, xopt, self.lower, self.upper, fit_im=self.fit_im, jac=jac)
        finally:
            ev.close()
        return xopt, fopt

    def generate_result(self, scale=1):
        """utils.py:226-295: per-peak real and imaginary contributions of the fitted parameters
        on the data grid (or a grid upsampled by ``scale``), their sums V, I, and the fit
        rotated back to the (u, v) frame -- one launch of the reconstruction kernel (csrc/result.hip).
        The imaginary contributions are the Kramers-Kronig partners in closed form (the reference
        integrates each point numerically).  ``core.fit_many(jobs, generate=True)`` does this for all
        the fits of a device batch in one launch."""
        if scale == 1.0:
            w = self.data.w
        else:
            w = np.linspace(self.data.w.min(), self.data.w.max(), int(scale * self.data.w.shape[0]))
        ev = equations.Evaluator(self.data.w, self.data.u, self.data.v, np.ones(len(self.data.w)),
                                 device=self._device())
        try:
            real, imag, fit, rotated = ev.generate_result(self.params, None if scale == 1.0 else w)
        finally:
            ev.close()
        self._store_result(w, real, imag, fit, rotated)

    def _store_result(self, w, real, imag, fit, rotated, call_shift_phase=True):
        """The attributes generate_result leaves behind (utils.py:251, 289-295), from the arrays the reconstruction
        kernel returns (csrc/result.hip) -- for one fit (generate_result) or as views of a batch's arrays
        (core.fit_many(generate=...))."""
        p0, p1 = self.params[0], self.params[1]
        # phase shift data by fit theta (utils.py:251; containers.py:68-78 with method='manual').  A data object that
        # brings the reference's method gets it called; one that does not gets the same attributes set from the kernel's
        # rotation of the spectrum.
        if call_shift_phase and hasattr(self.data, 'shift_phase'):
            self.data.shift_phase(method='manual', p0=p0, p1=p1)
        else:
            self.data.p0, self.data.p1 = p0, p1
            self.data.V, self.data.I = rotated[0], rotated[1]
        # (V_fit, I_fit: the contributions added peak after peak from zero, utils.py:276-277; u_fit, v_fit: the fit
        # rotated back, utils.py:284 -- all four evaluated next to the contributions on the GPU)
        self.u = fit[2]
        self.v = fit[3]
        self.V = fit[0]
        self.I = fit[1]
        self.w = w
        self.real_contribs = [real[k] for k in range(real.shape[0])]
        self.imag_contribs = [imag[k] for k in range(imag.shape[0])]

    def residual_stats(self, regions=None):
        """The ``quality.FitQuality`` of this finished fit: the residual V_fit - V_data at ``params`` reduced on the
        device (nmrfit_quality_stats, csrc/quality.hip; what plot.residual draws, as numbers) per region, over the whole
        grid and over what no region holds.  ``regions``: a list of ``(lo, hi)`` in units of w; default: the peaks'
        bounds.  Kept as ``self.quality``."""
        from . import quality
        if 'params' not in self.__dict__:      # (not hasattr: __getattr__ answers for missing names)
            raise AttributeError("residual_stats: this fit has no params yet (call fit() first)")
        if regions is None:
            regions = [tuple(p.bounds) for p in self.data.peaks]
        self.quality = quality.residual_stats(self.data.w, self.data.u, self.data.v, self.params, regions,
                                              device=self._device())
        return self.quality

    def uncertainty(self, sigma=None, noise_region=None, channels="real"):
        """The ``uncertainty.FitUncertainty`` of this finished fit at ``params``: first-order standard errors of the
        parameters and of the satellite area fraction from ONE launch of the D + 1 residual rows on a context
        (nmrfit_sandwich, csrc/lsq_cov.hip) -- the sandwich A^-1 M A^-1, not sigma^2 (J^T J)^-1 / N: the weights are not
        1/sigma -- and ``distance``, how many of them ``params`` lies from the local minimiser (large after an unpolished
        swarm).  ``sigma``: the noise of the spectrum, a float or a pair (sigma_u, sigma_v); else
        ``noise_region=(xstart, xstop)``, a signal-free stretch -- as ``fit_replicas`` takes them.  Real channel only
        (``fit_im=False``) unless ``channels="both"``: a ``fit_im`` fit then gets the two-channel record
        (nmrfit_sandwich_im, ``uncertainty.covariance_im``), whose errors belong to the minimiser of
        f = (rho_re + rho_im)/2 -- ``distance`` is measured with grad f, and a polish on both channels
        (``batch_polish="both"``) is what reaches that minimiser; a ``fit_im=False`` fit gets the same record either way.
        At most 24 peaks.  The record is returned, not kept: on the fits that
        ``fit_many(uncertainty=...)`` returns, the attribute ``uncertainty`` IS their record (it stands in this method's
        place there)."""
        from . import lsq, noise, uncertainty
        if 'params' not in self.__dict__:      # (not hasattr: __getattr__ answers for missing names)
            raise AttributeError("uncertainty: this fit has no params yet (call fit() first)")
        if channels not in ("real", "both"):
            raise ValueError('uncertainty: channels is "real" or "both"')
        mode = equations.fit_im_mode(self.fit_im)
        if mode and channels != "both":
            raise ValueError("uncertainty: the covariance covers the real channel only (fit_im=False); "
                             'channels="both" is the entrance of a fit_im fit')
        su, sv = noise._job_sigma(dict(sigma=sigma, noise_region=noise_region), self.data)
        lower, upper = _cabi.f64(self.lower), _cabi.f64(self.upper)
        ev = equations.Evaluator(self.data.w, self.data.u, self.data.v, self.weights, device=self._device())
        try:
            if mode:
                parts, meat = lsq.ResidualModel(ev, lower, upper, fit_im=mode).sandwich_im(self.params, su, sv)
                return uncertainty.covariance_im(parts, meat, self.params, lower, upper, sigma=(su, sv))
            A, M, g, _ = lsq.ResidualModel(ev, lower, upper).sandwich(self.params, su, sv)
        finally:
            ev.close()
        return uncertainty.covariance(A, M, g, self.params, lower, upper, sigma=(su, sv))

    def residual_arrays(self):
        """``data_V - V`` of this finished fit on its own grid, from the arrays of ``generate_result`` (one launch of the
        reconstruction kernel: the bits a device batch's ``residual_baseline`` works on); nothing is stored."""
        ev = equations.Evaluator(self.data.w, self.data.u, self.data.v, np.ones(len(self.data.w)), device=self._device())
        try:
            _, _, fit, rotated = ev.generate_result(self.params, None)
        finally:
            ev.close()
        return rotated[0] - fit[0]

    def get_areas(self):
        """utils.py:312-322."""
        return np.array([self.params[i] for i in range(6, len(self.params), 3)])

    def calculate_area_fraction(self):
        """utils.py:297-310: satellites (areas below the mean) over total."""
        areas = self.get_areas()
        m = np.mean(areas)
        peaks = areas[areas >= m].sum()
        sats = areas[areas < m].sum()
        return sats / (peaks + sats)

    def _print_summary(self):
        """What FitUtility._print_summary reports (nmrfit/utils.py:324-339): the four global parameters, one row per
        peak, the error -- through pandas' DataFrame.to_string(index=False) like the reference, so that whoever parses
        the reference's summary parses this one; a plain-text table of the same columns only where pandas is missing."""
        values = np.asarray(self.params, dtype=float)
        head, peak = ['p0', 'p1', 'r', 'y-off'], ['width', 'location', 'area']
        try:
            import pandas as pd
        except ImportError:
            pd = None

        def table(header, rows):
            if pd is not None:
                return pd.DataFrame(np.asarray(rows, dtype=float).reshape(-1, len(header)), columns=header).to_string(index=False)
            cells = [["%.6g" % x for x in row] for row in rows]
            widths = [max(len(h), *(len(c[k]) for c in cells)) for k, h in enumerate(header)]
            lines = [" ".join(h.rjust(n) for h, n in zip(header, widths))]
            lines += [" ".join(c.rjust(n) for c, n in zip(row, widths)) for row in cells]
            return "\n".join(lines)
        print("\nFit Summary:")
        print("------------")
        print("Global parameters")
        print(table(head, [values[:4]]))
        print("\nPeak parameters")
        print(table(peak, values[4:].reshape(-1, 3)))
        print("Error:\t", self.error)

"""
``fit`` -- the reference's entry point (nmrfit/core.py:64-95), same signature and return
value, executed on the MI355X.  ``load`` (instrument file parsing through nmrglue,
core.py:9-61) is outside the hot-path scope: build a ``Data``-like object (attributes
w, u, v, peaks) with the reference package or ``nmrfit_amd.synth`` and pass it in.
"""
import collections
import typing
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from . import _cabi, utils


def fit(data, lower, upper, expon=0.5, dynamic_weighting=True, fit_im=False, processes=1, summary=True,
        options={}):
    """Perform a fit of NMR spectroscopy data (reference: nmrfit/core.py:64).

    data : object with ``w, u, v`` (ndarrays) and ``peaks`` (each with ``bounds``, ``height``)
    lower, upper : parameter box, 4 + 3P floats (nmrfit/containers.py:193-217)
    expon, dynamic_weighting : error weighting (nmrfit/utils.py:191-224)
    fit_im : False (real part only, the default); True = the reference's imaginary term exactly as
             nmrfit/equations.py:197-209 computes it (last peak's line only); "sum" = all peaks.
             The Kramers-Kronig partner is evaluated in closed form on the GPU
    processes : accepted for compatibility; the batched GPU launch replaces the process pool
    summary : print the fit summary table
    options : swarmsize, maxiter, omega, phip, phig (+ minstep, minfunc, seed, device,
              check_every, polish, variant, exchange="rccl" for one process per GPU)

    Returns the FitUtility holding ``params``, ``error``, ``weights``.
    """
    f = utils.FitUtility(data, lower, upper, expon, dynamic_weighting, fit_im, processes, summary, options)
    f.fit()
    return f


def fit_many(jobs, threads=4, batch=True, shard=False, devices=None, generate=False, channel=None, device_weights=False,
             batch_polish=False, quality=False, residual_baseline=None, uncertainty=None, polish_jac="2-point", **kwargs):
    """Fit several spectra: ``jobs`` is a sequence of ``(data, lower, upper)`` triples (or dicts of ``fit``'s
    arguments); every job is fitted as ``fit`` would fit it with the same keyword arguments, and the list of
    FitUtility objects comes back in the order of ``jobs``.  Not in the reference (its users loop over
    ``nmrfit.fit``, nmrfit/core.py:64; its only parallel mode spreads ONE fit's particles over processes,
    nmrfit/utils.py:182).  ``summary`` defaults to False here.

    Shared and per-job arguments: a job's own entries win over the call's keyword arguments; ``options`` are merged key
    by key -- the call's ``options`` first, the job's own keys over them -- and that is the rule on every routing below
    (one device, ``devices=[...]``, ``shard=True``): ``fit_many(jobs_with_their_own_seed, options={"maxiter": 5})`` runs
    5 generations of every job wherever it lands.

    How the jobs run:

    * ``batch=True`` (default): jobs of equal kernel variant, ``fit_im``, ``maxiter`` and ``check_every`` -- grid lengths,
      peak counts and swarm sizes may differ -- are fitted as ONE device batch -- one kernel launch per swarm generation for all of them (nmrfit_amd.batch.FitBatch,
      csrc/batch*.hip).  A 204-particle swarm fills a fraction of an MI355X; a batch fills it.  Each fit's ``params`` and
      ``error`` are bit-identical to what ``fit`` returns for it alone with the same ``options['seed']``.  Job lists go
      through batches of a quarter of the list, between 40 and 200 jobs (``nmrfit_amd.core.BATCH_JOBS`` overrides),
      three stages in flight: a second host thread prepares the next batch (error weights, plans, device state) while
      the device runs two batches side by side (the tail of one -- its last swarms to stop -- overlaps with the other)
      and another thread reads back the one before.
    * ``generate=True`` (or a number: the ``scale`` of ``FitUtility.generate_result``): the rest of the reference's
      per-spectrum script, README.md:64-72 -- every returned fit has had ``generate_result(scale)`` called on it
      (nmrfit/utils.py:226-295: ``u, v, V, I, w, real_contribs, imag_contribs``; ``calculate_area_fraction()`` then
      needs nothing more).  For the fits of a device batch that is ONE launch over the batch's resident spectra and best
      positions (nmrfit_batch_contributions, csrc/result.hip) instead of a context, four uploads and a launch per fit;
      the values are bit-identical to the lone call's.  The data objects get ``p0, p1, V, I`` set to what
      ``data.shift_phase(method='manual', p0, p1)`` computes (nmrfit/containers.py:68-78) from the same launch; the
      method itself is called only on the lone path.
    * ``options['polish']``: the swarm runs in the batch, the least-squares refinement that follows it per fit on
      ``threads`` host threads (scipy's trust-region iterations, a context per fit) -- the answers are the lone call's.
    * whatever cannot be batched (a lone shape, more than 132 peaks, a batch the device refuses) runs
      through ``fit`` on ``threads`` host threads, each fit with its own context and HIP stream -- serially when
      ``options['exchange']`` is given: a communicator serves one swarm at a time.
    * ``shard=True`` in a multi-GPU launch (one process per GPU, RANK / WORLD_SIZE / LOCAL_RANK set by the launcher):
      the JOBS are divided over the ranks -- rank r takes jobs r, r + world, ... on its own GPU -- and the results are
      gathered so that every rank returns the full list (``params``, ``error``, ``seed``; the arrays of ``generate`` stay
      on the rank that made them).  Replicas: no collective touches the fits themselves.  This is the multi-GPU mode
      for many small fits (sharding one 204-particle swarm over GPUs is slower than one GPU).  ``channel``: an open
      ``nmrfit_amd.rendezvous.Channel`` to gather over (a caller that already has one); else one is made.
    * ``devices=[0, 1, ...]`` (or ``"all"``): the same replicas WITHOUT a launcher -- this one process drives several
      GPUs, a host thread per device, job k on ``devices[k % len(devices)]``; each device runs its share as device
      batches of its own.  Nothing crosses devices.  (``shard`` and ``devices`` exclude each other.)
    * ``device_weights=True``: the error weights of the fits of a device batch (``utils.compute_weights``, the one
      O(N x P) stage the preparation thread otherwise runs per fit) are built on the GPU as part of the batch's creation
      (csrc/weights.hip; ``FitBatch(regions=...)``), bit for bit the host's, so ``params`` and ``error`` do not change.
      ``f.weights`` of such a fit is made by the host routine on first access.  Fits that run alone take the host path.
    * ``batch_polish=True``: jobs with ``options['polish']`` and ``fit_im=False`` that ran in a device batch are refined
      by ``FitBatch.polish`` while the batch is still resident -- all of them in lock step, every step one launch of
      every fit's D + 1 residual rows and the normal equations reduced on the device (csrc/lsq.hip; ``lsq.lm_polish``),
      D^2 + D doubles per fit and step to the host -- in place of a context, an upload and scipy's trust-region
      iterations per fit.  Same objective, same start, another solver: ``params`` agree with the per-fit path to the
      minimum's accuracy, not bit for bit; ``error`` is the rows launch's value at the accepted point and never above the
      swarm's; ``generate`` reconstructs from the refined parameters.  Jobs with ``fit_im``, jobs that fell back to lone
      fits and lone ``fit()`` keep the per-fit path.
    * ``batch_polish="both"``: as ``True``, and the jobs with ``options['polish']`` of a ``fit_im`` batch (True or "sum")
      are refined in lock step too, on BOTH channels (``FitBatch.polish(channels="both")``; csrc/objective_rows_im.hip,
      include/nmrfit_amd_lsq_im.h): the loop minimises the objective their swarms minimised, (rho_re + rho_im)/2, where
      the per-fit path refines the real channel and can only accept or reject against it.  ``error`` is that objective
      at the accepted point, never above the swarm's.  ``fit_im=False`` jobs behave as under ``True``; fits that end
      up alone and batches with any D > 76 keep the per-fit path.
    * ``polish_jac="analytic"``: every polish of the call takes the closed-form Jacobian of the real-channel residual
      (include/nmrfit_amd_lsq_analytic.h, csrc/lsq_analytic.hip) instead of the forward differences of D + 1 residual
      rows -- ``FitBatch.polish(jac="analytic")`` under ``batch_polish=True``, ``lsq.polish(jac="analytic")`` on the
      per-fit path.  ``error`` is still the rows launch's value at the accepted point, never above the swarm's.  Real
      channel only: with ``batch_polish="both"`` it raises ValueError up front.  Default "2-point": as ever.
    * ``quality=True``: every returned fit carries ``fit.quality`` (``nmrfit_amd.quality.FitQuality``): the residual
      V_fit - V_data at its FINAL ``params`` reduced on the device per peak region (the peaks' bounds), over the whole
      grid and over what no region holds -- (P + 2) rows of 64 bytes per fit instead of the arrays of ``generate`` --
      bit for bit ``residual_stats(w, u, v, fit.params, bounds)``.  The fits of a device batch go through
      ``FitBatch.residual_stats`` while the batch is resident (those with ``options['polish']`` are refined before
      that, not after the batch has closed), the fits that ran alone through one ``residual_stats_many`` call per
      device.  ``params`` and ``error`` do not change.  With ``shard=True`` the rows stay on the rank that made them,
      like the arrays of ``generate``.
    * ``residual_baseline=deg`` (or a dict: ``deg``, ``margin``, ``intervals``, ``complement``, ``return_baseline``): every
      returned fit carries ``fit.residual_baseline`` (``nmrfit_amd.baseline.BaselineFit``): a least-squares polynomial of
      that degree fitted to the residual ``data_V - V`` at its FINAL ``params`` outside its peaks' bounds (widened about
      their centres by ``margin``; or over the caller's ``intervals``) -- where the Lorentzian tails of the main line are
      already accounted for -- in a conditioned basis and a fixed summation order (include/nmrfit_amd_baseline.h), 17
      doubles per fit.  The fits of a device batch go through ``FitBatch.residual_baseline`` while the batch is resident
      (those with ``options['polish']`` are refined before that), the fits that ran alone through ``generate_result``'s
      arrays and one ``baseline.fit_many`` call per device: the same V and data_V bits, the same rows.  ``params`` and
      ``error`` do not change and nothing is refitted: ``baseline.subtract_rotated`` and a second ``fit_many`` are the
      recipe.  With ``shard=True`` the rows stay on the rank that made them.
    * ``uncertainty=dict(sigma=...)`` (a float or a pair (sigma_u, sigma_v)) or ``dict(noise_region=(xstart, xstop))``,
      optionally with ``device_sigma=True`` -- exactly what they mean in ``fit_replicas_many``; a job's own ``sigma`` /
      ``noise_region`` entry wins over the call's: every returned fit carries ``fit.uncertainty``
      (``nmrfit_amd.uncertainty.FitUncertainty``): first-order standard errors of its FINAL ``params`` and of the
      satellite area fraction from the sandwich covariance A^-1 M A^-1 (include/nmrfit_amd_cov.h, csrc/lsq_cov.hip) --
      one launch of D + 1 residual rows per fit where ``fit_replicas`` runs 32 further fits -- and ``distance``, how many
      standard errors ``params`` lies from the local minimiser: the errors describe the noise alone, and an unpolished
      swarm stops 0.06 ... 76 of them away (ask for ``options['polish']``).  The fits of a device batch go through
      ``FitBatch.uncertainty`` while the batch is resident (those with ``options['polish']`` are refined before that),
      the fits that ran alone through a context (``FitUtility.uncertainty``).  Real channel only: a ``fit_im`` job raises
      ValueError up front -- unless the dict says ``channels="both"``, see below -- so does one with more than 24 peaks.
      ``params`` and ``error`` do not change.  With ``shard=True`` the records stay on the rank that made them.
    * ``uncertainty=dict(..., channels="both")``: the ``fit_im`` jobs of the call get the two-channel record
      (include/nmrfit_amd_cov_im.h, csrc/lsq_cov_im.hip; ``uncertainty.covariance_im``) while their batch is resident,
      after any polish; the ``fit_im=False`` jobs of the same call get the record they always got, bit for bit.  The
      errors of a ``fit_im`` fit belong to the minimiser of f = (rho_re + rho_im)/2 and ``distance`` is measured with
      grad f: ``batch_polish="both"`` is the polish that reaches that minimiser."""
    from . import baseline as _baseline, uncertainty as _uncertainty
    kwargs.setdefault("summary", False)
    jobs = [dict(job) if isinstance(job, dict) else dict(zip(("data", "lower", "upper"), job)) for job in jobs]
    if polish_jac not in ("2-point", "analytic"):
        raise ValueError('fit_many: polish_jac is "2-point" or "analytic"')
    if polish_jac == "analytic" and isinstance(batch_polish, str) and batch_polish == "both":
        raise ValueError('fit_many: polish_jac="analytic" covers the real channel only: not with batch_polish="both"')
    call = _Call(threads, batch, kwargs, 1 if generate is True else generate, bool(device_weights),
                 "both" if isinstance(batch_polish, str) and batch_polish == "both" else bool(batch_polish), bool(quality),
                 _baseline.option(residual_baseline), polish_jac, _uncertainty.option(uncertainty))
    if polish_jac == "analytic" and call.uncertainty is not None and call.uncertainty.get("channels", "real") == "both":
        raise ValueError('fit_many: polish_jac="analytic" covers the real channel only: not with uncertainty channels="both"')
    if call.uncertainty is not None:
        from .equations import fit_im_mode
        for m, job in enumerate(jobs):
            args = dict(kwargs, **job)
            if fit_im_mode(args.get("fit_im", False)) and call.uncertainty.get("channels", "real") != "both":
                raise ValueError("fit_many: uncertainty covers the real channel only: job %d has fit_im=%r" % (m, args["fit_im"]))
            if len(args["lower"]) > _cabi.LSQ_MAX_D:
                raise ValueError("fit_many: uncertainty takes fits of at most %d parameters (24 peaks): job %d has %d"
                                 % (_cabi.LSQ_MAX_D, m, len(args["lower"])))
    if devices is not None:
        if shard:
            raise ValueError("fit_many: shard=True divides the jobs over PROCESSES, devices=[...] over the GPUs of this "
                             "process: use one of them")
        if isinstance(devices, str):
            if devices != "all":
                raise ValueError("fit_many: devices must be a list of device indices or \"all\"")
            devices = list(range(_cabi_device_count()))
        devices = [int(d) for d in devices]
        if not devices:
            raise ValueError("fit_many: no devices")
        return _fit_many_devices(jobs, call, devices)
    if shard:
        from . import rendezvous
        rank, _, world = rendezvous.env_rank_world()
        if world > 1:
            return _fit_many_sharded(jobs, call, rank, world, channel=channel)
    return _fit_many_local(jobs, call)


class _Call(typing.NamedTuple):
    """What one fit_many call asked for: built once by fit_many, passed on unchanged."""
    threads: int
    batch: bool
    kwargs: dict                 # fit's keyword arguments, shared by the jobs
    scale: object                # ``generate``: False (no reconstruction), or generate_result's scale (True -> 1)
    device_weights: bool
    batch_polish: object         # False, True (fit_im=False jobs), or "both" (the jobs of fit_im batches too, on both channels)
    quality: bool = False        # every fit gets ``quality``: its residual statistics per peak region (quality.py)
    residual_baseline: object = None   # None, or baseline.option()'s dict: every fit gets ``residual_baseline`` (baseline.py)
    polish_jac: str = "2-point"  # the Jacobian of every polish: "2-point" (D + 1 residual rows) or "analytic" (lsq_analytic.hip)
    uncertainty: object = None   # None, or uncertainty.option()'s dict: every fit gets ``uncertainty`` (uncertainty.py)


def _result_record(f):
    """What travels between ranks for one finished fit."""
    return dict(params=list(map(float, f.params)), error=float(f.error), seed=getattr(f, "seed", None))


def _merged_options(shared_options, job):
    """The ``options`` one job is fitted with, on every routing: the call's shared options first, the job's own keys
    win."""
    opts = dict(shared_options or {})
    opts.update(job.get("options") or {})
    return opts


def _fit_args(call, job):
    """``fit``'s arguments for one job: the call's keyword arguments, the job's own entries over them -- except
    ``options``, which are merged key by key (``_merged_options``).  A job's ``sigma`` / ``noise_region`` are its noise
    for ``call.uncertainty`` (``uncertainty.job_sigmas``), not arguments of ``fit``."""
    args = {k: v for k, v in dict(call.kwargs, **job).items() if k not in ("sigma", "noise_region")}
    if "options" in call.kwargs or "options" in job:
        args["options"] = _merged_options(call.kwargs.get("options"), job)
    return args


def _with_device(job, shared_options, device, force=False):
    """The job with ``device`` in its own (merged) options.  ``force``: the caller assigns the device
    (devices=[...]); otherwise a device the job or the shared options name wins."""
    opts = _merged_options(shared_options, job)
    if force or opts.get("device") is None:
        opts["device"] = device
    return dict(job, options=opts)


def _fit_many_sharded(jobs, call, rank, world, channel=None, local=None):
    """Jobs r, r + world, ... on this rank's GPU; every rank returns every result (the other ranks' as FitUtility
    objects holding ``params`` / ``error`` / ``seed``; their ``weights`` are recomputed on demand only by ``fit``)."""
    import json
    from . import rendezvous
    mine = list(range(rank, len(jobs), world))
    if local is None:
        device, note = rendezvous.pick_device(_cabi_device_count())
        if note:
            import sys
            sys.stderr.write("nmrfit: %s\n" % note)

        def local(my_jobs):
            return _fit_many_local(my_jobs, call)
    else:
        device = None
    # the ranks meet BEFORE they fit: a mis-launched world shows at once, and the channel's connect deadline does not
    # have to cover the slowest rank's share of the work
    own = channel is None
    if own:
        channel = rendezvous.Channel()
    try:
        shared = call.kwargs.get("options") or {}
        done = local([_with_device(jobs[i], shared, device) if device is not None else jobs[i] for i in mine])
        # (JSON, not pickle: what arrives from another rank is data, never code; repr round-trips a float64 exactly)
        parts = channel.all_gather(json.dumps([[i, _result_record(f)] for i, f in zip(mine, done)]).encode())
    finally:
        if own:
            channel.close()
    out = [None] * len(jobs)
    for i, f in zip(mine, done):
        out[i] = f
    for r, blob in enumerate(parts):
        if r == rank:
            continue
        for i, rec in json.loads(blob.decode()):
            job = jobs[i]
            args = {k: v for k, v in _fit_args(call, job).items() if k not in ("data", "lower", "upper")}
            f = utils.FitUtility(job["data"], job["lower"], job["upper"], **args)
            f.params, f.error, f.seed = np.array(rec["params"]), rec["error"], rec["seed"]
            out[i] = f
    return out


def _fit_many_devices(jobs, call, devices):
    """Job k on devices[k % len(devices)], one host thread per device (the library releases the GIL inside its calls;
    every call binds its own device), results back in job order."""
    shares = [list(range(i, len(jobs), len(devices))) for i in range(len(devices))]
    shared = call.kwargs.get("options") or {}

    def one(i):
        return _fit_many_local([_with_device(jobs[k], shared, devices[i], force=True) for k in shares[i]], call)
    out = [None] * len(jobs)
    with ThreadPoolExecutor(max_workers=len(devices)) as pool:
        for idx, res in zip(shares, pool.map(one, range(len(devices)))):
            for k, f in zip(idx, res):
                out[k] = f
    return out


_cabi_device_count = _cabi.device_count      # (under a name of core's own: the CPU tests replace it)


# Jobs per device batch in fit_many.  From ~40 default-size fits on a batch holds the MI355X's issue rate (DESIGN.md
# 4.5), and a long list wants large batches (1000 default jobs with pyswarm's rule: 2050 fits/s in batches of 64, 2270 in
# batches of 200) while a short one wants at least four of them, so that the three stages overlap -- the host prepares
# batch c + 1 (error weights, plans, device state) on a second thread while the device runs batch c and a third thread
# reads back batch c - 1 (200 jobs: 1970 fits/s in batches of 50, 1740 as one batch; profiles/r06/fit_many_span_sweep.txt).
# BATCH_JOBS = None: that rule (a quarter of the list, between 40 and 200); a number: batches of about that many.
BATCH_JOBS = None
BATCH_JOBS_MIN, BATCH_JOBS_MAX, PIPELINE_BATCHES = 40, 200, 4
# Device batches driven at the same time.  With pyswarm's rule the swarms of a batch stop at different generations (112
# ... 411 for default fits) and the batch's last generations hold a few swarms each, at a launch's latency; a second
# batch running beside it fills the device meanwhile: 4 batches of 50 default fits 93.7 -> 82.4 ms (2134 -> 2427 fits/s
# on the device), three at a time 79.8 (tools/concurrent_batches.py, profiles/r06/concurrent_batches.txt).
# End to end (tools/pipeline_ab.py, profiles/r06/fit_many_pipeline_ab.txt; one box, best of three): 200 default jobs with
# pyswarm's rule 1924 -> 2038 fits/s, 1000 jobs 2349 -> 2405 -- less than on the device alone, the rest of the call being
# the first batch's preparation and the last one's read-back; with the reconstruction 1707 -> 1728 / 2146 -> 2120 (noise).
# (measured and not kept: the first batch of a list cut in two halves to start the device sooner -- no difference; the
# read-back on the thread that ran the batch instead of the storing thread -- same rates, same profile file.)
RUN_AT_ONCE = 2


def _batch_jobs(n):
    if BATCH_JOBS is not None:
        return max(1, int(BATCH_JOBS))
    return min(BATCH_JOBS_MAX, max(BATCH_JOBS_MIN, -(-n // PIPELINE_BATCHES)))


class _Batch:
    """One device batch of a fit_many call: the FitBatch ``fb``, its ``fits`` and their ``plans``, the BatchKey they
    share and their places ``idx`` in the job list.  create, run, read, store -- or close."""

    def __init__(self, fb, fits, plans, key, idx):
        self.fb, self.fits, self.plans, self.key, self.idx = fb, fits, plans, key, idx
        self.quality = None      # read(), ``call.quality``: the fits' FitQuality, made while the batch was resident
        self.residual_baseline = None      # read(), ``call.residual_baseline``: the fits' BaselineFit, likewise
        self.uncertainty = None      # read(), ``call.uncertainty``: the fits' FitUncertainty, likewise

    @classmethod
    def create(cls, fits, plans, key, idx):
        """The device state of one batch (spectra, weights, boxes, swarms) -- everything up to the first launch."""
        from .batch import FitBatch
        swarmsize = [int(p['swarmsize']) for p in plans]
        # (all or nothing: the plans of one fit_many call either all carry their regions -- device_weights -- or none does)
        regions = [p['regions'] for p in plans] if all('regions' in p for p in plans) else None
        if regions is None:
            spectra = [(f.data.w, f.data.u, f.data.v, f.weights) for f in fits]
        else:
            spectra = [(f.data.w, f.data.u, f.data.v) for f in fits]
        kw = {name: [p['kw'][name] for p in plans] for name in ("omega", "phip", "phig", "minstep", "minfunc")}
        fb = FitBatch(spectra, [f.lower for f in fits], [f.upper for f in fits], swarmsize=swarmsize,
                      seeds=[p['seed'] for p in plans], variant=key.variant, fit_im=key.fit_im, device=key.device,
                      regions=regions, **kw)
        return cls(fb, fits, plans, key, idx)

    def run(self):
        self.fb.run(self.key.maxiter, self.key.check_every)

    def close(self):
        self.fb.close()

    def read(self, call):
        """What is read from the device after the batch's generations: stop codes, best positions and -- ``call.scale``
        not False -- the reconstruction of every fit in one launch (FitBatch.generate).  ``call.batch_polish``: the fits
        with options['polish'] and fit_im=False are refined here, in lock step, from the batch's resident spectra
        (FitBatch.polish); their entries of ``best`` are then the refined ones and their indices come back as
        ``refined``: store leaves them alone.  ``call.quality``: the residual statistics of every fit at its final
        parameters, from the resident spectra (FitBatch.residual_stats) -- the fits store would refine one by one are
        refined here first and count as ``refined``.  ``call.residual_baseline``: the same for the polynomial baseline of
        every fit's residual (FitBatch.residual_baseline), ``call.uncertainty`` for the standard errors of every fit's
        parameters under its own noise (FitBatch.uncertainty).  Closes the batch.  Returns (refined, status, best, results)."""
        fits, fb, refined = self.fits, self.fb, set()
        polished = sum(1 for f in fits if f.options.get('polish', False))
        try:
            status = fb.status()
            best = fb.best()
            results = fb.generate(call.scale) if call.scale is not False and polished < len(fits) else None
            if call.batch_polish:
                # (a batch has one fit_im mode: with one, its fits are refined here only under "both", on both channels)
                both = call.batch_polish == "both"
                which = [k for k, f in enumerate(fits) if f.options.get('polish', False) and (both or not f.fit_im)]
                kw = dict(channels="both") if any(fits[k].fit_im for k in which) else {}
                if call.polish_jac != "2-point":
                    kw["jac"] = call.polish_jac
                # (the launch covers the whole batch: one fit beyond the kernel's D leaves all of them to the per-fit path)
                if which and max(len(f.lower) for f in fits) <= _cabi.LSQ_MAX_D:
                    new = fb.polish([x for x, _ in best], which=which, **kw)
                    for k in which:
                        best[k] = new[k]
                    refined = set(which)
            if call.quality:
                refined |= self._refine_per_fit(call, refined, best)
                self.quality = fb.residual_stats([x for x, _ in best], [_peak_regions(f) for f in fits])
            if call.residual_baseline is not None:
                refined |= self._refine_per_fit(call, refined, best)
                self.residual_baseline = _residual_baseline_resident(fb, call.residual_baseline, fits, [x for x, _ in best])
            if call.uncertainty is not None:
                refined |= self._refine_per_fit(call, refined, best)
                # (a batch has one fit_im mode: fit_many has refused such jobs unless the call says channels="both")
                kw = dict(channels="both") if any(f.fit_im for f in fits) else {}
                self.uncertainty = fb.uncertainty([x for x, _ in best], [f.noise_sigma[0] for f in fits],
                                                  [f.noise_sigma[1] for f in fits], **kw)
        finally:
            fb.close()
        return refined, status, best, results

    def _refine_per_fit(self, call, refined, best):
        """FitUtility._polish, ``call.threads`` at a time, for the fits with options['polish'] that are not in
        ``refined``: their entries of ``best`` become the refined ones.  Returns their indices."""
        fits, plans = self.fits, self.plans
        per_fit = [k for k, f in enumerate(fits) if f.options.get('polish', False) and k not in refined]
        if per_fit:
            kw = {} if call.polish_jac == "2-point" else dict(jac=call.polish_jac)

            def refine(k):
                return fits[k]._polish(best[k][0], best[k][1], plans[k], **kw)
            if call.threads > 1 and len(per_fit) > 1:
                with ThreadPoolExecutor(max_workers=int(call.threads)) as pool:
                    new = list(pool.map(refine, per_fit))
            else:
                new = [refine(k) for k in per_fit]
            for k, xf in zip(per_fit, new):
                best[k] = xf
        return set(per_fit)

    def store(self, call, refined, status, best, results):
        """The batch's results into the FitUtility objects (what FitUtility.fit and generate_result leave behind).  Fits
        with options['polish'] that read has not ``refined`` are refined first (FitUtility._polish, ``call.threads`` at a
        time); every polished fit is reconstructed from its refined parameters."""
        from .pso import STOP_MESSAGES
        fits, plans, scale = self.fits, self.plans, call.scale
        polished = [k for k, f in enumerate(fits) if f.options.get('polish', False)]
        self._refine_per_fit(call, refined, best)
        for k, (f, p, st, (x, fx)) in enumerate(zip(fits, plans, status, best)):
            # (pyswarm's closing line, once per fit like the plain loop prints it)
            if st["stop"]:
                print(STOP_MESSAGES[st["stop"]].format(minfunc=p['kw']['minfunc'], minstep=p['kw']['minstep']))
            else:
                print('Stopping search: maximum iterations reached --> {:}'.format(self.key.maxiter))
            f._finish(x, fx)
            if self.quality is not None:
                f.quality = self.quality[k]
            if self.residual_baseline is not None:
                f.residual_baseline = self.residual_baseline[k]
            if self.uncertainty is not None:
                f.uncertainty = self.uncertainty[k]
            if k in polished:
                if scale is not False:
                    f.generate_result(scale)      # (from the refined parameters: the batch's launch used the swarm's)
            elif results is not None:
                r = results[k]
                f._store_result(f.data.w if r["w"] is None else r["w"], r["real"], r["imag"],
                                (r["V"], r["I"], r["u"], r["v"]), (r["data_V"], r["data_I"]), call_shift_phase=False)

    def collect(self, call):
        """Read back and store in one go."""
        self.store(call, *self.read(call))


class _Pipeline:
    """The three stages of _fit_many_local and what is in flight between them: one thread prepares the batches of a
    span (error weights, plans, device state), RUN_AT_ONCE threads run batches, one thread reads back and stores."""

    def __init__(self, call, fits):
        self.call, self.fits, self.plans = call, fits, {}
        self.host, self.post, self.runner = (ThreadPoolExecutor(max_workers=k) for k in (1, 1, RUN_AT_ONCE))
        self.pending = None                     # future of the preparation under way
        self.made = []                          # every batch created and run, or about to (closed by its read, or on an error)
        self.inflight = collections.deque()     # (future of a batch's run, the batch), in job order
        self.posted = []                        # futures of the stores
        self.batched = set()                    # the jobs that went into a batch

    def __enter__(self):
        return self

    def __exit__(self, error, *_):
        """After an error: let everything under way end, then close every batch made.  Always: end the threads."""
        if error is not None:
            waits = [self.pending] if self.pending is not None else []      # (batches made for a span that will not run)
            waits += [fut for fut, _ in self.inflight] + self.posted        # (runs in flight end before their batches close)
            for fut in waits:
                try:
                    got = fut.result()
                    if fut is self.pending:
                        self.made.extend(got[0])
                except Exception:
                    pass
            for b in self.made:
                b.close()
        for pool in (self.runner, self.post, self.host):
            pool.shutdown(wait=True)

    def group(self, members):
        """Device batches of the members (index, key) that have a partner, ready to run; the others as (index, key)."""
        groups = {}
        for i, key in members:
            groups.setdefault(key, []).append(i)
        ready, single = [], []
        for key, idx in groups.items():
            if key is not None and len(idx) > 1:
                try:
                    ready.append(_Batch.create([self.fits[i] for i in idx], [self.plans[i] for i in idx], key, idx))
                    continue
                except _cabi.NmrfitError:
                    # the device refused this batch (LDS budget of its peak counts, memory): its fits run one by one
                    key = None
            single.extend((i, key) for i in idx)
        return ready, single

    def prepare(self, span):
        """Start the preparation of a span's jobs on the preparing thread (``None``: no further span)."""
        def work():
            for i in span:
                self.plans[i] = self.fits[i]._plan(device_weights=self.call.device_weights)
            return self.group([(i, self.fits[i]._batch_key(self.plans[i])) for i in span])
        self.pending = self.host.submit(work) if span is not None else None

    def drain(self, limit):
        """Wait for the oldest runs until at most ``limit`` are in flight; each batch that has run goes to the thread
        that reads back and stores, in job order (pyswarm's closing lines print in job order)."""
        while len(self.inflight) > limit:
            fut, b = self.inflight.popleft()
            fut.result()
            self.posted.append(self.post.submit(b.collect, self.call))

    def run(self, ready, last=False):
        self.made.extend(ready)
        for n, b in enumerate(ready):
            self.batched.update(b.idx)
            if last and n == len(ready) - 1 and not self.posted and not self.inflight:
                # the only batch of the call: nothing to overlap it with -- run and read back here, without a thread's
                # first HIP call in the way (a 40-job list is 30 ms in all)
                b.run()
                b.collect(self.call)
                continue
            # RUN_AT_ONCE batches are driven at the same time (threads of their own: the C calls release the GIL): while
            # the last swarms of one batch finish -- a generation of three swarms costs a launch of 8-20 us whatever it
            # holds -- or its results travel to the host, the other batch fills the device
            self.drain(RUN_AT_ONCE - 1)
            self.inflight.append((self.runner.submit(b.run), b))

    def finish(self):
        self.drain(0)
        for p in self.posted:
            p.result()


def _fit_many_local(jobs, call):
    fits = []
    for job in jobs:
        args = _fit_args(call, job)
        fits.append(utils.FitUtility(args.pop("data"), args.pop("lower"), args.pop("upper"), **args))
    if call.uncertainty is not None:
        # every fit's (sigma_u, sigma_v), before anything runs: a job without noise fails here, not after its fit
        from . import uncertainty
        device = int((call.kwargs.get("options") or {}).get("device") or 0)
        for f, pair in zip(fits, uncertainty.job_sigmas([dict(job, data=f.data) for job, f in zip(jobs, fits)],
                                                        call.uncertainty, device)):
            f.noise_sigma = pair
    if not (call.batch and len(fits) > 1):
        return _fit_alone(fits, {}, range(len(fits)), call)
    n = len(fits)
    size = -(-n // -(-n // _batch_jobs(n)))      # spans of equal size, as many as batches of _batch_jobs(n) need
    spans = [range(a, min(a + size, n)) for a in range(0, n, size)]
    leftover = []
    with _Pipeline(call, fits) as pipe:      # (on an error it waits for what is under way and closes every batch made)
        pipe.prepare(spans[0])
        for c in range(len(spans)):
            ready, single = pipe.pending.result()
            pipe.prepare(spans[c + 1] if c + 1 < len(spans) else None)
            leftover.extend(single)
            pipe.run(ready, last=(c + 1 == len(spans) and not any(key is not None for _, key in leftover)))
        # what found no partner inside its span may have one in another
        ready, _ = pipe.group([(i, key) for i, key in leftover if key is not None])
        pipe.run(ready, last=True)
        pipe.finish()
    return _fit_alone(fits, pipe.plans, [i for i in range(n) if i not in pipe.batched], call)


def _peak_regions(f):
    """The regions of a fit's residual statistics: its peaks' bounds."""
    return [tuple(p.bounds) for p in f.data.peaks]


def _residual_baseline_resident(fb, opts, fits, X):
    """``FitBatch.residual_baseline`` at ``X`` under the call's options (baseline.option)."""
    from . import baseline
    picked = [baseline.fit_intervals(opts, f) for f in fits]
    return fb.residual_baseline(X, deg=opts["deg"], intervals=[iv for iv, _ in picked], complement=[c for _, c in picked],
                                return_baseline=opts["return_baseline"])


def _residual_baseline_alone(fits, idx, opts, device):
    """The same for fits that ran alone: the residual from ``generate_result``'s arrays (scale 1: the reconstruction's V
    and data_V bits), one ``baseline.fit_many`` call."""
    from . import baseline
    ys = [fits[i].residual_arrays() for i in idx]
    picked = [baseline.fit_intervals(opts, fits[i]) for i in idx]
    got = baseline.fit_many([fits[i].data.w for i in idx], ys, deg=opts["deg"], intervals=[iv for iv, _ in picked],
                            complement=[c for _, c in picked], device=device, return_baseline=opts["return_baseline"])
    for i, b in zip(idx, got):
        fits[i].residual_baseline = b


def _fit_alone(fits, plans, alone, call):
    """The fits that ran in no batch, through fit() -- with the plan made for them, if any -- on ``call.threads``
    threads; serially when any carries an ``exchange`` (a communicator serves one swarm at a time).  ``call.quality``:
    their residual statistics in one residual_stats_many call per device."""
    def lone(i):
        fits[i].fit(plan=plans.get(i))
        if call.scale is not False:
            fits[i].generate_result(call.scale)
    if call.threads <= 1 or len(alone) <= 1 or any(fits[i].options.get("exchange") is not None for i in alone):
        for i in alone:
            lone(i)
    else:
        with ThreadPoolExecutor(max_workers=int(call.threads)) as pool:
            list(pool.map(lone, alone))
    if call.quality:
        from . import quality
        by_device = {}
        for i in alone:
            by_device.setdefault(fits[i]._device(), []).append(i)
        for device, idx in by_device.items():
            got = quality.residual_stats_many([(fits[i].data.w, fits[i].data.u, fits[i].data.v) for i in idx],
                                              [fits[i].params for i in idx], [_peak_regions(fits[i]) for i in idx], device=device)
            for i, q in zip(idx, got):
                fits[i].quality = q
    if call.residual_baseline is not None:
        by_device = {}
        for i in alone:
            by_device.setdefault(fits[i]._device(), []).append(i)
        for device, idx in by_device.items():
            _residual_baseline_alone(fits, idx, call.residual_baseline, device)
    if call.uncertainty is not None:
        for i in alone:      # (a context per fit: the record takes the method's place on the fit)
            fits[i].uncertainty = utils.FitUtility.uncertainty(fits[i], sigma=fits[i].noise_sigma,
                                                               channels=call.uncertainty.get("channels", "real"))
    return fits

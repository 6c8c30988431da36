"""
Noise replicas: how far to trust a fitted number.

The classic answer refits noisy copies of the data and reads the spread of the results.  The reference ships the two
helpers for it -- ``utils.sample_noise`` (the sigma of a signal-free stretch) and ``utils.rnd_data`` (data + sigma *
normal deviates) -- and leaves the loop to the user, K fits of minutes each.  Here the K copies are ONE device batch:
``fit_replicas`` tiles the spectrum into ``FitBatch``es, the copies are made on the device in place
(``FitBatch.add_noise``; csrc/noise.hip, include/nmrfit_amd_noise.h) and every replica runs exactly as ``fit`` would run
it on that copy.  No Jacobian, no linearisation at a box-constrained optimum, and the swarm's own scatter -- a real part
of the error of a particle-swarm fit -- is in the spread; with ``options['polish']`` the replicas are refined on the
resident batch (``FitBatch.polish``) and the spread is that of the least-squares minimisers, which
tests/test_gpu_calibration.py holds replica by replica to the linear response of each replica's own noise.

The deviates are a pure function of (noise seed, grid point): one Philox4x32-10 block per point (``pso.philox4x32_10``,
counter ``(j lo, j hi, 0x4E4F4953, 0)``, key the seed) and one Box-Muller pair for the two channels.  ``normals`` is the
numpy mirror of the device function, ``replicas_host`` the mirror applied, ``replicas`` the device call.  Mirror and
device round ``log``, ``sin`` and ``cos`` on their own, so they agree to a few ulp of the deviate, not bit for bit; the
device gives the same bits for the same (seed, point) alone, in any batch, out of place or in place.
"""
import numpy as np

from . import _cabi, pso

NOISE_TAG = 0x4E4F4953                 # counter word 2 of the noise stream (NMRFIT_NOISE_TAG): the swarm's is a particle index < 2^28
_MASK64 = 0xFFFFFFFFFFFFFFFF
_TWO_PI = 6.283185307179586


def normals(seed, N):
    """``(z_u, z_v)``: the two standard normal deviates of grid points 0 .. N-1 under the 64-bit noise ``seed`` -- the
    definition of include/nmrfit_amd_noise.h in numpy."""
    seed = int(seed) & _MASK64
    j = np.arange(int(N), dtype=np.uint64)
    o0, o1, o2, o3 = pso.philox4x32_10(j & np.uint64(0xFFFFFFFF), j >> np.uint64(32), np.full(j.shape, NOISE_TAG, dtype=np.uint64),
                                       np.zeros(j.shape, dtype=np.uint64), seed & 0xFFFFFFFF, seed >> 32)
    ua = (o1 << np.uint64(32)) | o0
    ub = (o3 << np.uint64(32)) | o2
    scale = 2.0 ** -53
    a = ((ua >> np.uint64(11)) + np.uint64(1)).astype(np.float64) * scale      # (0, 1]
    b = (ub >> np.uint64(11)).astype(np.float64) * scale                       # [0, 1)
    r = np.sqrt(-2.0 * np.log(a))
    t = _TWO_PI * b
    return r * np.cos(t), r * np.sin(t)


def _as_list(us, vs, sigma_u, sigma_v, seeds):
    """The five arguments of ``replicas`` as lists of K: contiguous float64 spectra, sigmas (scalars broadcast), seeds."""
    us = [np.ascontiguousarray(u, dtype=np.float64).ravel() for u in us]
    vs = [np.ascontiguousarray(v, dtype=np.float64).ravel() for v in vs]
    K = len(us)
    if len(vs) != K or any(len(u) != len(v) for u, v in zip(us, vs)):
        raise ValueError("replicas: as many v as u, of the same lengths")
    su = np.ascontiguousarray(np.broadcast_to(np.asarray(sigma_u, dtype=np.float64), (K,)))
    sv = np.ascontiguousarray(np.broadcast_to(np.asarray(sigma_v, dtype=np.float64), (K,)))
    sd = np.array([int(s) & _MASK64 for s in (seeds if np.ndim(seeds) else [seeds] * K)], dtype=np.uint64)
    if sd.shape != (K,):
        raise ValueError("replicas: one seed per spectrum")
    return us, vs, su, sv, sd


def replicas_host(u, v, sigma_u, sigma_v, seeds):
    """The mirror applied: ``u + sigma_u * z_u, v + sigma_v * z_v`` (a rounded multiply, then a rounded add) with
    ``normals(seed, N)``.  One spectrum (1-D ``u``, ``v``; scalar sigmas and seed) gives one pair of arrays, a list of
    spectra (sigmas and seeds per spectrum, scalars broadcast) a list of pairs.  A spectrum whose two sigmas are 0 comes
    back as an untouched copy."""
    single = np.ndim(u[0]) == 0
    us, vs, su, sv, sd = _as_list([u] if single else u, [v] if single else v, sigma_u, sigma_v, seeds)
    out = []
    for uk, vk, a, b, s in zip(us, vs, su, sv, sd):
        if a == 0.0 and b == 0.0:
            out.append((uk.copy(), vk.copy()))
            continue
        zu, zv = normals(s, len(uk))
        out.append((uk + a * zu, vk + b * zv))
    return out[0] if single else out


def _calls(Ns):
    """[k0, k1) ranges of at most 65535 spectra and 2^26 grid points per library call (as utils._weight_calls)."""
    from .utils import _weight_calls
    return _weight_calls(Ns)


def replicas(us, vs, sigma_u, sigma_v, seeds, device=0):
    """Noisy copies of K spectra made on the GPU (nmrfit_noise_replicas, csrc/noise.hip): the list of ``(u', v')`` pairs.
    The spectra may differ in length; ``sigma_u``, ``sigma_v``: scalars or one value per spectrum (finite, >= 0);
    ``seeds``: one 64-bit noise seed per spectrum.  Lists of any length are cut into library calls of at most 65535
    spectra and 2^26 grid points.  A spectrum's copy is the same bits alone or in any list."""
    us, vs, su, sv, sd = _as_list(us, vs, sigma_u, sigma_v, seeds)
    lib = _cabi.lib()
    out = []
    for k0, k1 in _calls([len(u) for u in us]):
        N = np.array([len(u) for u in us[k0:k1]], dtype=np.int64)
        u, v = np.concatenate(us[k0:k1]), np.concatenate(vs[k0:k1])
        uo, vo = np.empty_like(u), np.empty_like(v)
        a, b, s = (np.ascontiguousarray(x[k0:k1]) for x in (su, sv, sd))
        _cabi.check(lib.nmrfit_noise_replicas(int(device), k1 - k0, _cabi.ptr(N), _cabi.ptr(u), _cabi.ptr(v), _cabi.ptr(a),
                                              _cabi.ptr(b), _cabi.ptr(s), _cabi.ptr(uo), _cabi.ptr(vo)))
        noff = np.concatenate(([0], np.cumsum(N)))
        out += [(uo[noff[k]:noff[k + 1]], vo[noff[k]:noff[k + 1]]) for k in range(k1 - k0)]
    return out


class ReplicaFits:
    """What ``fit_replicas`` returns for one spectrum.

    fits : the FitUtility objects, ``params`` and ``error`` set (fit 0 the original data when ``include_original``);
           their ``data`` is the caller's object -- fit k's own spectrum is
           ``replicas([data.u], [data.v], sigma[k][0], sigma[k][1], [seeds[k]])``
    params [K, D], errors [K], iterations [K], stop [K] (0 maxiter, 1 minfunc, 2 minstep)
    area_fractions [K] : ``calculate_area_fraction()`` of each fit
    sigma [K, 2], seeds [K] : every fit's (sigma_u, sigma_v) and its seed (swarm and noise)
    area_fraction_std, params_std : ``np.std(..., ddof=1)`` over the NOISY fits only (the original is not a draw)
    percentile(q) : of the noisy fits' area fractions
    """

    def __init__(self, fits, sigma, seeds, iterations=None, stop=None, include_original=True):
        self.fits = list(fits)
        K = len(self.fits)
        self.include_original = bool(include_original)
        self.params = np.array([np.asarray(f.params, dtype=float) for f in self.fits]).reshape(K, -1)
        self.errors = np.array([float(f.error) for f in self.fits])
        self.iterations = np.zeros(K, dtype=np.int64) if iterations is None else np.asarray(iterations, dtype=np.int64)
        self.stop = np.zeros(K, dtype=np.int32) if stop is None else np.asarray(stop, dtype=np.int32)
        self.area_fractions = np.array([f.calculate_area_fraction() for f in self.fits])
        self.sigma = np.asarray(sigma, dtype=float).reshape(K, 2)
        self.seeds = [int(s) for s in seeds]

    @property
    def _noisy(self):
        return slice(1, None) if self.include_original else slice(None)

    @property
    def area_fraction_std(self):
        return float(np.std(self.area_fractions[self._noisy], ddof=1))

    @property
    def params_std(self):
        return np.std(self.params[self._noisy], axis=0, ddof=1)

    def percentile(self, q):
        return np.percentile(self.area_fractions[self._noisy], q)


def _job_sigma(job, data):
    """(sigma_u, sigma_v) of a job: ``sigma`` (a float or a pair), else from ``noise_region=(xstart, xstop)`` through
    ``utils.sample_noise`` on each channel."""
    from .peaks import sample_noise
    sigma, region = job.get("sigma"), job.get("noise_region")
    if sigma is not None:
        pair = (float(sigma),) * 2 if np.ndim(sigma) == 0 else tuple(float(s) for s in sigma)
        if len(pair) != 2:
            raise ValueError("fit_replicas: sigma is a float or a pair (sigma_u, sigma_v)")
    elif region is not None:
        w, (x0, x1) = np.asarray(data.w), region
        pair = (float(sample_noise(w, np.asarray(data.u), x0, x1)), float(sample_noise(w, np.asarray(data.v), x0, x1)))
    else:
        raise ValueError("fit_replicas: give sigma (a float or a pair) or noise_region=(xstart, xstop)")
    if not all(np.isfinite(s) and s >= 0.0 for s in pair):
        raise ValueError("fit_replicas: sigma must be finite and >= 0, got %r" % (pair,))
    return pair


def _device_sigmas(jobs, shared, device):
    """``_job_sigma`` of every job that gives a ``noise_region`` (its own, or the shared one) and no ``sigma``, from ONE
    ``baseline.sample_noise_many`` call on both channels; {job index: (sigma_u, sigma_v)}."""
    from .baseline import sample_noise_many
    idx, regions = [], []
    for m, job in enumerate(jobs):
        src = job if job.get("sigma") is not None or job.get("noise_region") is not None else shared
        if src.get("sigma") is None and src.get("noise_region") is not None:
            idx.append(m)
            regions.append(tuple(src["noise_region"]))
    if not idx:
        return {}
    datas = [dict(shared, **jobs[m])["data"] for m in idx]
    got = sample_noise_many([d.w for d in datas], [np.array([d.u, d.v], dtype=np.float64) for d in datas], regions, device=device)
    out = {}
    for m, pair in zip(idx, got):
        pair = (float(pair[0]), float(pair[1]))
        if not all(np.isfinite(s) and s >= 0.0 for s in pair):
            raise ValueError("fit_replicas: sigma must be finite and >= 0, got %r" % (pair,))
        out[m] = pair
    return out


def fit_replicas_many(jobs, replicas=32, seed=0, include_original=True, device_sigma=False, **kwargs):
    """``fit_replicas`` for several spectra at once: ``jobs`` as ``fit_many`` takes them -- ``(data, lower, upper)``
    triples or dicts of ``fit``'s arguments -- each with its own ``sigma`` or ``noise_region`` (or the shared keyword).
    All M x K fits are packed into ragged device batches of at most ``core.BATCH_JOBS_MAX`` fits.  Fit k of job m
    (k = 0: the original data, k = 1 .. replicas: the noisy copies) has swarm seed and noise seed
    ``seed + m * (replicas + 1) + k``, whether the original is included or not -- ``options['seed']`` is not used: the
    seeds of a replica study come from the ``seed`` keyword alone.  Returns one ``ReplicaFits`` per job.

    ``device_sigma=True``: the sigmas of all jobs that give a ``noise_region`` come from one
    ``baseline.sample_noise_many`` call (csrc/baseline.hip: the same quadratic fit in a conditioned basis, on the device
    ``options['device']`` names) instead of two ``sample_noise`` calls per job on the host; they agree with the host's to
    the conditioning of ``np.polyfit`` on raw ppm values, not bit for bit, so the default stays the host path.

    ``options['polish']``: every fit that has it is refined by ``FitBatch.polish`` while its batch is resident -- in lock
    step, on the fit's own (noisy) spectrum, ``channels="both"`` in the batches of ``fit_im`` jobs -- and ``params`` /
    ``error`` are the refined ones (never worse than the swarm's).  WITHOUT it every replica is a swarm result stopped by
    pyswarm's rule, and the spread includes the optimiser's stopping error, which does not depend on the noise and adds
    in quadrature.  Measured on exactly fitted two- and three-peak spectra at sigma = 1e-3 max|u| (DESIGN.md section 4.11,
    profiles/r18/replica_calibration.txt): the default swarm of 204 stops a median 0.06 .. 0.4, at the 95th percentile
    0.3 .. 4 and at worst 20 .. 76 standard errors from the replica's minimiser, and ``params_std`` comes out 1.0 .. 8.2
    times (``area_fraction_std`` 1.0 .. 1.9 times) the noise-driven spread; with 64 particles 5 .. 70 times (5 .. 220).
    With polish every replica is within 0.05 standard errors of the linear response to its own noise and the spreads are
    the predicted ones to 0.3 %: ask for it when the spread is to be read as the noise's.  Fit 0 is then the lone
    ``fit``'s swarm result refined by the batch's Levenberg-Marquardt loop, where a lone ``fit`` with the option runs
    scipy's TRF: the same minimum to the stopping tolerances, not the same bits.  Fits beyond the least-squares kernel's
    parameter count (``_cabi.LSQ_MAX_D``) in a batch that refines any: ValueError.

    Every fit runs in a device batch: ``options['exchange']`` and kernel variants a batch does not run are refused
    (ValueError)."""
    from . import core, utils
    from .batch import FitBatch
    replicas = int(replicas)
    if replicas < 1:
        raise ValueError("fit_replicas: at least one replica")
    kwargs = dict(kwargs, summary=False)
    kwargs.pop("processes", None)
    jobs = [dict(job) if isinstance(job, dict) else dict(zip(("data", "lower", "upper"), job)) for job in jobs]
    ks = list(range(0 if include_original else 1, replicas + 1))
    sigmas = _device_sigmas(jobs, kwargs, int((kwargs.get("options") or {}).get("device") or 0)) if device_sigma else {}
    entries, per_job = [], []          # every fit of the call: (job, its place in the job's list); per job: plan, fits, ...
    for m, job in enumerate(jobs):
        args = dict(kwargs, **job)
        data = args["data"]
        own = job.get("sigma") is not None or job.get("noise_region") is not None      # (a job's own beats the shared one)
        sigma = sigmas[m] if m in sigmas else _job_sigma(job if own else kwargs, data)
        fa = {k: v for k, v in args.items() if k not in ("data", "lower", "upper", "sigma", "noise_region")}
        base = utils.FitUtility(data, args["lower"], args["upper"], **fa)
        if base.options.get("exchange") is not None:
            raise ValueError("fit_replicas: the replicas run as device batches: options['exchange'] is not supported")
        plan = base._plan()            # ONE plan per job: weights, swarm constants, variant, maxiter -- as fit makes it
        key = base._batch_key(plan)
        if key is None:
            raise ValueError("fit_replicas: kernel variant %r does not run in a device batch" % (plan["variant"],))
        fits = []
        for k in ks:
            f = utils.FitUtility(data, args["lower"], args["upper"], **fa)
            f.weights = base.weights
            f.seed = (int(seed) + m * (replicas + 1) + k) & _MASK64
            fits.append(f)
            entries.append((m, len(fits) - 1))
        per_job.append(dict(plan=plan, key=key, fits=fits, sigma=[(0.0, 0.0) if k == 0 else sigma for k in ks],
                            u=_cabi.f64(data.u), v=_cabi.f64(data.v), iterations=[0] * len(ks), stop=[0] * len(ks)))
    groups = {}
    for e in entries:
        groups.setdefault(per_job[e[0]]["key"], []).append(e)
    for key, members in groups.items():
        # (the rows launch of FitBatch.polish covers the whole batch: every fit of a batch that refines any)
        fits = [per_job[m]["fits"][i] for m, i in members]
        if any(f.options.get("polish", False) for f in fits) and max(len(f.lower) for f in fits) > _cabi.LSQ_MAX_D:
            raise ValueError("fit_replicas: options['polish'] refines device batches of fits with at most %d parameters"
                             % _cabi.LSQ_MAX_D)
    for key, members in groups.items():
        for a in range(0, len(members), core.BATCH_JOBS_MAX):
            chunk = members[a:a + core.BATCH_JOBS_MAX]
            recs = [per_job[m] for m, _ in chunk]
            fits = [per_job[m]["fits"][i] for m, i in chunk]
            sig = np.array([per_job[m]["sigma"][i] for m, i in chunk])
            seeds = [f.seed for f in fits]
            kw = {name: [r["plan"]["kw"][name] for r in recs] for name in ("omega", "phip", "phig", "minstep", "minfunc")}
            # (data.u, data.v are copied into the batch's upload planes: the caller's arrays are never written)
            with FitBatch([(f.data.w, r["u"], r["v"], f.weights) for f, r in zip(fits, recs)], [f.lower for f in fits],
                          [f.upper for f in fits], swarmsize=[int(r["plan"]["swarmsize"]) for r in recs], seeds=seeds,
                          variant=key.variant, fit_im=key.fit_im, device=key.device, **kw) as fb:
                if np.any(sig != 0.0):
                    fb.add_noise(sig[:, 0], sig[:, 1], seeds)
                fb.run(key.maxiter, key.check_every)
                status, best = fb.status(), fb.best()
                which = [j for j, f in enumerate(fits) if f.options.get("polish", False)]
                if which:
                    new = fb.polish([x for x, _ in best], which=which, **(dict(channels="both") if key.fit_im else {}))
                    for j in which:
                        best[j] = new[j]
            for (m, i), f, st, (x, fx) in zip(chunk, fits, status, best):
                f._finish(x, fx)
                per_job[m]["iterations"][i], per_job[m]["stop"][i] = st["iteration"], st["stop"]
    return [ReplicaFits(r["fits"], r["sigma"], [f.seed for f in r["fits"]], r["iterations"], r["stop"],
                        include_original=include_original) for r in per_job]


def fit_replicas(data, lower, upper, replicas=32, sigma=None, noise_region=None, seed=0, include_original=True, expon=0.5,
                 dynamic_weighting=True, fit_im=False, options={}):
    """Refit ``replicas`` noisy copies of a spectrum as one device batch and return the ``ReplicaFits``: the spread of
    the satellite area fraction (``area_fraction_std``, ``percentile``) and of every parameter (``params_std``).

    data, lower, upper, expon, dynamic_weighting, fit_im, options : as ``fit`` takes them; every replica is configured
        exactly as ``fit`` would configure it (one ``FitUtility._plan()``: weights, swarm constants, variant, maxiter)
    sigma : the noise to add, a float or a pair ``(sigma_u, sigma_v)``; else
    noise_region : ``(xstart, xstop)``, a signal-free stretch of ``data.w``: sigma_u, sigma_v are
        ``utils.sample_noise(w, u, xstart, xstop)`` and ``utils.sample_noise(w, v, xstart, xstop)``; neither: ValueError
    seed : fit k (0: the original, 1 .. replicas: the copies) runs with swarm seed ``seed + k`` and noise seed ``seed + k``
        (``options['seed']`` is not used)
    include_original : fit 0 is the data as it is (sigma 0) -- bit for bit
        ``nmrfit_amd.fit(data, ..., options={..., 'seed': seed})`` -- and stays out of the statistics
    options['polish'] : every replica is refined by least squares on the resident batch (``fit_replicas_many``); without
        it the spread includes the swarm's stopping error, which on its own can be several times the noise's

    ``data`` itself is never written."""
    return fit_replicas_many([dict(data=data, lower=lower, upper=upper)], replicas=replicas, seed=seed,
                             include_original=include_original, sigma=sigma, noise_region=noise_region, expon=expon,
                             dynamic_weighting=dynamic_weighting, fit_im=fit_im, options=options)[0]

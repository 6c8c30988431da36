"""
Device-batched fits: K independent spectra fitted together, one kernel launch per swarm generation for all of them
(``nmrfit_batch_*`` of libnmrfit_amd.so, csrc/batch*.hip).

The reference's users call ``nmrfit.fit`` once per spectrum (nmrfit/core.py:64, README.md:64-66), each fit a
204-particle swarm (nmrfit/utils.py:177) -- a fraction of an MI355X.  ``FitBatch`` holds K spectra -- of any lengths:
every dataset is cropped to its own region, nmrfit/containers.py:112-130 -- and K swarms (of any sizes) on the device;
every fit has its own grid, peak count, box, seed and stopping rule, follows exactly the trajectory a lone
``nmrfit_amd.fit`` gives it (bit-identical ``params`` / ``error`` for the same seed) and stops on its own.
``nmrfit_amd.fit_many`` builds these batches from a list of jobs.
"""
import ctypes

import numpy as np

from . import _cabi, equations, pso, utils


class FitBatch:
    """K fits on one GPU.

    spectra : K tuples ``(w, u, v, weights)`` (what FitUtility.fit passes as ``args``, nmrfit/utils.py:176); the K
              spectra may differ in length
    lowers, uppers : K parameter boxes, 4 + 3 P_k floats each (nmrfit/containers.py:193-217)
    swarmsize : particles per fit: one number, or K of them (``options['swarmsize']`` of each fit, nmrfit/utils.py:177)
    seeds : K integers (the swarm's random stream, like options['seed'] of ``fit``)
    omega, phip, phig, minstep, minfunc : scalars or length-K sequences
    variant : "default" or "farfield" (what ``fit`` would select for these shapes)
    fit_im : False, True (the reference's imaginary term) or "sum" (every peak; "default" kernel), for the whole batch
    regions : None, or K entries ``(edges, level)`` (``utils.weight_regions``; None: unit weights) -- the weights of the
              WHOLE batch are then built on the device (nmrfit_batch_create_regions, csrc/weights.hip: bit for bit what
              ``utils.compute_weights`` gives) and the ``spectra`` tuples are ``(w, u, v)`` (a fourth element of None is
              allowed)
    """

    def __init__(self, spectra, lowers, uppers, swarmsize=pso.DEFAULTS["swarmsize"], seeds=None,
                 omega=pso.DEFAULTS["omega"], phip=pso.DEFAULTS["phip"], phig=pso.DEFAULTS["phig"],
                 minstep=pso.DEFAULTS["minstep"], minfunc=pso.DEFAULTS["minfunc"], variant="default", fit_im=False,
                 device=0, regions=None):
        self._lib = _cabi.lib()
        self._h = ctypes.c_void_p()
        K = len(spectra)
        if K == 0 or len(lowers) != K or len(uppers) != K:
            raise ValueError("FitBatch: as many boxes as spectra, at least one")
        Ns = np.array([len(sp[0]) for sp in spectra], dtype=np.int64)
        noff = np.concatenate(([0], np.cumsum(Ns)))
        if regions is not None:
            if len(regions) != K:
                raise ValueError("FitBatch: one entry of regions per spectrum")
            for k, sp in enumerate(spectra):
                if len(sp) not in (3, 4) or (len(sp) == 4 and sp[3] is not None):
                    raise ValueError("FitBatch: with regions a spectrum is (w, u, v): the batch builds every fit's "
                                     "weights or none (fit %d)" % k)
            spectra = [tuple(sp[:3]) for sp in spectra]
            R, edges, level = utils.pack_regions(regions)
        planes = [np.empty(int(noff[-1])) for _ in range(4 if regions is None else 3)]
        for k, sp in enumerate(spectra):
            if regions is not None:
                if any(len(a) != Ns[k] for a in sp) or Ns[k] == 0:
                    raise ValueError("FitBatch: w, u, v of a spectrum have the same non-zero length (fit %d)" % k)
            elif len(sp) != 4 or any(len(a) != Ns[k] for a in sp) or Ns[k] == 0:
                raise ValueError("FitBatch: w, u, v, weights of a spectrum have the same non-zero length (fit %d)" % k)
            for a, plane in zip(sp, planes):
                plane[noff[k]:noff[k + 1]] = a      # (contiguous float64: the reference hands out reversed views, core.py:60)
        self._w_range = [(np.min(sp[0]), np.max(sp[0])) for sp in spectra]      # (generate: the upsampled grids' ends)
        lbs = [_cabi.f64(lo) for lo in lowers]
        ubs = [_cabi.f64(up) for up in uppers]
        self.lowers, self.uppers = lbs, ubs
        self.D = []
        for k, (lo, up) in enumerate(zip(lbs, ubs)):
            assert len(lo) == len(up), 'Lower- and upper-bounds must be the same length'
            assert np.all(up > lo), 'All upper-bound values must be greater than lower-bound values'
            if lo.size < 4 or (lo.size - 4) % 3:
                raise ValueError("bounds must have 4 + 3P entries (fit %d)" % k)
            self.D.append(int(lo.size))
        # N: the common grid length, or None when the spectra differ in length (Ns, noff: per fit)
        # S: the common swarm size, or None when the swarms differ in size (Ss: per fit)
        self.Ss = np.ascontiguousarray(np.broadcast_to(np.asarray(swarmsize, dtype=np.int64), (K,)))
        self.K, self.Ns, self.noff = K, Ns, noff
        self.N = int(Ns[0]) if np.all(Ns == Ns[0]) else None
        self.S = int(self.Ss[0]) if np.all(self.Ss == self.Ss[0]) else None
        self.P = np.array([(d - 4) // 3 for d in self.D], dtype=np.int32)
        self.offsets = np.concatenate(([0], np.cumsum(self.D)))
        lower = np.concatenate(lbs)
        upper = np.concatenate(ubs)
        if seeds is None:
            seeds = np.random.SeedSequence().generate_state(K, dtype=np.uint64)
        om, pp, pg, ms, mf = (np.broadcast_to(np.asarray(x, dtype=np.float64), (K,)) for x in (omega, phip, phig, minstep, minfunc))
        self.minstep, self.minfunc = ms.copy(), mf.copy()
        self.seeds = [int(s) & 0xFFFFFFFFFFFFFFFF for s in seeds]
        prm = (_cabi.PsoParams * K)()
        for k in range(K):
            prm[k] = _cabi.PsoParams(om[k], pp[k], pg[k], ms[k], mf[k], self.seeds[k])
        if regions is not None:
            _cabi.check(self._lib.nmrfit_batch_create_regions(int(device), K, _cabi.ptr(Ns), _cabi.ptr(planes[0]),
                                                              _cabi.ptr(planes[1]), _cabi.ptr(planes[2]), _cabi.ptr(R),
                                                              _cabi.ptr(edges), _cabi.ptr(level), _cabi.ptr(self.P),
                                                              _cabi.ptr(lower), _cabi.ptr(upper), _cabi.ptr(self.Ss), prm,
                                                              _cabi.variant_id(variant), equations.fit_im_mode(fit_im),
                                                              ctypes.byref(self._h)))
            return
        _cabi.check(self._lib.nmrfit_batch_create_ragged(int(device), K, _cabi.ptr(Ns), _cabi.ptr(planes[0]),
                                                         _cabi.ptr(planes[1]), _cabi.ptr(planes[2]), _cabi.ptr(planes[3]),
                                                         _cabi.ptr(self.P), _cabi.ptr(lower), _cabi.ptr(upper), _cabi.ptr(self.Ss), prm,
                                                         _cabi.variant_id(variant), equations.fit_im_mode(fit_im),
                                                         ctypes.byref(self._h)))

    # -- life cycle ----------------------------------------------------------------------------
    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self._lib.nmrfit_batch_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- the product calls -------------------------------------------------------------------------
    def run(self, maxiter=pso.DEFAULTS["maxiter"], check_every=64):
        """Generation 0 (if needed) + up to ``maxiter`` generations of every fit; returns when all have stopped."""
        _cabi.check(self._lib.nmrfit_batch_run(self._h, int(maxiter), int(check_every)))

    def status(self):
        """Per fit: completed generations, stop code (0 running, 1 minfunc, 2 minstep), current fg."""
        it = np.zeros(self.K, dtype=np.int64)
        stop = np.zeros(self.K, dtype=np.int32)
        fg = np.zeros(self.K)
        _cabi.check(self._lib.nmrfit_batch_status(self._h, _cabi.ptr(it), _cabi.ptr(stop), _cabi.ptr(fg)))
        return [dict(iteration=int(i), stop=int(s), fg=float(f)) for i, s, f in zip(it, stop, fg)]

    def best(self):
        """Per fit ``(x_best, f_best)``: after a stop these are pyswarm's return values."""
        x = np.empty(int(self.offsets[-1]))
        f = np.empty(self.K)
        _cabi.check(self._lib.nmrfit_batch_best(self._h, _cabi.ptr(x), _cabi.ptr(f)))
        return [(x[self.offsets[k]:self.offsets[k + 1]].copy(), float(f[k])) for k in range(self.K)]

    def generate(self, scale=1, grids=None):
        """FitUtility.generate_result for every fit of the batch at its best position (nmrfit/utils.py:226-295), ONE launch
        from the batch's resident spectra.  ``scale`` == 1: on each fit's own grid; else on
        ``np.linspace(w.min(), w.max(), int(scale * N_k))`` per fit (utils.py:236; ``grids``: the K output grids, if the
        caller has them).  Returns per fit a dict with ``w`` (None when scale == 1: the fit's own grid), ``real``,
        ``imag`` ([P_k, Nout] each), ``V, I, u, v`` (the fit: utils.py:276-284) and ``data_V, data_I`` (the spectrum rotated
        by the fitted phase, what data.shift_phase(method='manual') stores, utils.py:251) -- all views of four arrays."""
        K, Ns = self.K, self.Ns
        if scale == 1.0 and grids is None:
            wout = nout = None
            n = Ns
        else:
            if grids is None:
                grids = [np.linspace(lo, hi, int(scale * Ns[k])) for k, (lo, hi) in enumerate(self._w_range)]
            if len(grids) != K:
                raise ValueError("FitBatch.generate: one output grid per fit")
            n = np.array([len(g) for g in grids], dtype=np.int64)
            nout = n
            wout = np.concatenate([_cabi.f64(g) for g in grids]) if K else np.empty(0)
        P = self.P.astype(np.int64)
        roff = np.concatenate(([0], np.cumsum(P * n)))          # contributions: P_k rows of n_k per fit
        foff = np.concatenate(([0], np.cumsum(4 * n)))
        woff = np.concatenate(([0], np.cumsum(n)))
        real = np.empty(int(roff[-1]))
        imag = np.empty(int(roff[-1]))
        fit = np.empty(int(foff[-1]))
        data = np.empty(2 * int(self.noff[-1]))
        _cabi.check(self._lib.nmrfit_batch_contributions(self._h, _cabi.ptr(nout), _cabi.ptr(wout), _cabi.ptr(real),
                                                         _cabi.ptr(imag), _cabi.ptr(fit), _cabi.ptr(data)))
        out = []
        for k in range(K):
            nk, Nk = int(n[k]), int(Ns[k])
            f4 = fit[foff[k]:foff[k + 1]].reshape(4, nk)
            d2 = data[2 * self.noff[k]:2 * self.noff[k + 1]].reshape(2, Nk)
            out.append(dict(w=None if wout is None else wout[woff[k]:woff[k + 1]],
                            real=real[roff[k]:roff[k + 1]].reshape(int(P[k]), nk),
                            imag=imag[roff[k]:roff[k + 1]].reshape(int(P[k]), nk),
                            V=f4[0], I=f4[1], u=f4[2], v=f4[3], data_V=d2[0], data_I=d2[1]))
        return out

    # -- noise replicas (include/nmrfit_amd_noise.h) -----------------------------------------------
    def add_noise(self, sigma_u, sigma_v, seeds):
        """Perturb the resident spectra in place on the device: fit k's ``u, v`` become
        ``u + sigma_u[k] * z_u, v + sigma_v[k] * z_v`` with the deviates of noise seed ``seeds[k]`` (csrc/noise.hip; the
        numpy mirror is ``noise.replicas_host``) -- bit for bit what ``noise.replicas`` returns for the uploaded arrays.
        Scalars broadcast to the K fits; a fit whose two sigmas are 0 is not touched.  Allowed once, and only before the
        first generation (``NmrfitError`` with the state code otherwise)."""
        su = np.ascontiguousarray(np.broadcast_to(np.asarray(sigma_u, dtype=np.float64), (self.K,)))
        sv = np.ascontiguousarray(np.broadcast_to(np.asarray(sigma_v, dtype=np.float64), (self.K,)))
        sd = np.array([int(s) & 0xFFFFFFFFFFFFFFFF for s in (seeds if np.ndim(seeds) else [seeds] * self.K)], dtype=np.uint64)
        if sd.shape != (self.K,):
            raise ValueError("FitBatch.add_noise: one seed per fit")
        _cabi.check(self._lib.nmrfit_batch_add_noise(self._h, _cabi.ptr(su), _cabi.ptr(sv), _cabi.ptr(sd)))

    def spectrum(self, k):
        """``(u, v)`` of the spectrum fit ``k`` is fitting, in grid order: what was uploaded, or its replica after
        ``add_noise``.  Any state."""
        k = int(k)
        n = int(self.Ns[k]) if 0 <= k < self.K else 1
        u, v = np.empty(n), np.empty(n)
        _cabi.check(self._lib.nmrfit_batch_spectrum(self._h, k, _cabi.ptr(u), _cabi.ptr(v)))
        return u, v

    # -- residual statistics (include/nmrfit_amd_quality.h) ----------------------------------------
    def residual_stats(self, X=None, regions=None):
        """Per fit its ``quality.FitQuality``: the residual V_fit - V_data reduced on the device over the batch's
        resident spectra (csrc/quality.hip) -- per region, over the whole grid and over what no region holds -- in one
        call for all K fits; (R_k + 2) rows of 8 doubles per fit come back.  ``X``: the K parameter vectors, allowed in
        any state; None: every fit's best position (``NmrfitError`` with the state code before the first generation).
        ``regions``: K lists of ``(lo, hi)`` in units of w; None: no regions.  Bit for bit
        ``quality.residual_stats_host`` of the arrays ``generate()`` returns, and ``quality.residual_stats`` of the
        spectrum alone.  The swarms are not touched."""
        from . import quality
        if regions is None:
            regions = [None] * self.K
        if len(regions) != self.K:
            raise ValueError("FitBatch.residual_stats: one list of regions per fit")
        R, edges = quality.pack_edges(regions)
        x = None
        if X is not None:
            if len(X) != self.K:
                raise ValueError("FitBatch.residual_stats: one parameter vector per fit")
            X = [_cabi.f64(xk).ravel() for xk in X]
            for k, xk in enumerate(X):
                if xk.shape != (self.D[k],):
                    raise ValueError("FitBatch.residual_stats: fit %d takes %d parameters" % (k, self.D[k]))
            x = np.concatenate(X)
        out = np.empty((int(R.sum()) + 2 * self.K) * quality.ROW)
        _cabi.check(self._lib.nmrfit_batch_quality_stats(self._h, _cabi.ptr(x), _cabi.ptr(R),
                                                         _cabi.ptr(edges) if edges.size else None, _cabi.ptr(out)))
        return quality.split_rows(out, R, self.D)

    # -- residual baseline (include/nmrfit_amd_baseline.h) ------------------------------------------
    def residual_baseline(self, X=None, deg=1, intervals=None, complement=True, return_baseline=False):
        """Per fit a ``baseline.BaselineFit``: a least-squares polynomial of degree ``deg`` fitted to the residual
        ``data_V - V`` of every fit over a masked part of its grid, on the batch's resident spectra (csrc/baseline.hip) --
        17 doubles per fit come back instead of the arrays of ``generate``.  ``X``: the K parameter vectors, allowed in any
        state; None: every fit's best position (``NmrfitError`` with the state code before the first generation).
        ``intervals``: None, or K lists of ``(lo, hi)`` in units of w; ``complement=True`` (the default) fits OUTSIDE them
        -- give the peaks' regions; with no intervals that is the whole grid.  ``deg``, ``complement``: one value or one
        per fit.  ``return_baseline``: also the polynomial at every grid point (``BaselineFit.baseline``).  Bit for bit
        ``baseline.fit_many`` on the ``data_V - V`` of ``generate()``.  The swarms are not touched."""
        from . import baseline
        d, R, edges, comp = baseline.pack_jobs(self.K, deg, intervals, complement)
        x = None
        if X is not None:
            if len(X) != self.K:
                raise ValueError("FitBatch.residual_baseline: one parameter vector per fit")
            X = [_cabi.f64(xk).ravel() for xk in X]
            for k, xk in enumerate(X):
                if xk.shape != (self.D[k],):
                    raise ValueError("FitBatch.residual_baseline: fit %d takes %d parameters" % (k, self.D[k]))
            x = np.concatenate(X)
        rows = np.empty(self.K * baseline.ROW)
        base = np.empty(int(self.noff[-1])) if return_baseline else None
        _cabi.check(self._lib.nmrfit_batch_residual_baseline(self._h, _cabi.ptr(x), _cabi.ptr(d), _cabi.ptr(R),
                                                             _cabi.ptr(edges) if edges.size else None, _cabi.ptr(comp),
                                                             _cabi.ptr(rows), _cabi.ptr(base)))
        rows = rows.reshape(self.K, baseline.ROW)
        return [baseline.BaselineFit(rows[k], base[self.noff[k]:self.noff[k + 1]].copy() if return_baseline else None)
                for k in range(self.K)]

    # -- least squares (include/nmrfit_amd_lsq.h) --------------------------------------------------
    def normal_equations(self, X, channels="real", jac="2-point"):
        """Per fit ``(A, g, f)`` at the K parameter vectors ``X``: the forward-difference rows ``lsq.ResidualModel``
        would make for each fit's box, their residual rows for ALL fits in one launch over the batch's resident spectra,
        A = J^T J and g = J^T r reduced on the device (csrc/lsq.hip), f the launch's own objective value at X[k].
        Bit-identical to ``lsq.ResidualModel(Evaluator(spectrum), lower, upper).normal_equations(X[k])`` fit by fit, in
        any batch.  The swarms are not touched.  D <= 76 for every fit.

        ``channels="both"`` (a batch created with a ``fit_im`` mode; nmrfit_batch_normal_equations_im): the rows of both
        channels in the same launch, A and g per channel, and per fit the combined ``(H, grad f, f)`` of the objective
        f = (rho_re + rho_im)/2 the batch's swarms minimise (``lsq.combine_channels``) -- bit-identical to
        ``lsq.ResidualModel(Evaluator(spectrum), lower, upper, fit_im=mode).normal_equations(X[k])``.

        ``jac="analytic"`` (``channels="real"``; nmrfit_batch_normal_equations_analytic, csrc/lsq_analytic.hip): A, g and
        f = ||r|| from the closed-form derivatives of the residual in one pass over the resident spectra -- no residual
        rows, no steps; bit-identical to ``Evaluator(spectrum).jacobian_analytic(X[k], normal=True)`` fit by fit, in any
        batch.  A point with a width of zero or below the kernels' floor is refused."""
        from . import lsq
        if channels not in ("real", "both"):
            raise ValueError('FitBatch.normal_equations: channels is "real" or "both"')
        if lsq._jac_form("FitBatch.normal_equations", jac) == "analytic" and channels == "both":
            raise ValueError('FitBatch.normal_equations: jac="analytic" covers the real channel only (channels="real")')
        if len(X) != self.K:
            raise ValueError("FitBatch.normal_equations: one parameter vector per fit")
        if jac == "analytic":
            xs = []
            for k, x in enumerate(X):
                x = _cabi.f64(x)
                if x.shape != (self.D[k],):
                    raise ValueError("FitBatch.normal_equations: fit %d takes %d parameters" % (k, self.D[k]))
                xs.append(x)
            xs = np.concatenate(xs)
            D = np.asarray(self.D, dtype=np.int64)
            aoff = np.concatenate(([0], np.cumsum(D * D)))
            A, g, f = np.empty(int(aoff[-1])), np.empty(int(self.offsets[-1])), np.empty(self.K)
            _cabi.check(self._lib.nmrfit_batch_normal_equations_analytic(self._h, _cabi.ptr(xs), _cabi.ptr(A), _cabi.ptr(g),
                                                                         _cabi.ptr(f)))
            return [(A[aoff[k]:aoff[k + 1]].reshape(self.D[k], self.D[k]), g[self.offsets[k]:self.offsets[k + 1]], float(f[k]))
                    for k in range(self.K)]
        rows, cs = [], []
        s = 1.0 / np.sqrt(self.Ns.astype(np.float64))
        for k, x in enumerate(X):
            x = _cabi.f64(x)
            if x.shape != (self.D[k],):
                raise ValueError("FitBatch.normal_equations: fit %d takes %d parameters" % (k, self.D[k]))
            r, h = lsq.forward_rows(x, self.lowers[k], self.uppers[k])
            rows.append(r.ravel())
            cs.append(s[k] / h)
        rows, cs = np.concatenate(rows), np.concatenate(cs)
        D = np.asarray(self.D, dtype=np.int64)
        aoff = np.concatenate(([0], np.cumsum(D * D)))
        A = np.empty(int(aoff[-1]))
        g = np.empty(int(self.offsets[-1]))
        if channels == "both":
            A2, g2, f2 = np.empty(2 * int(aoff[-1])), np.empty(2 * int(self.offsets[-1])), np.empty(2 * self.K)
            _cabi.check(self._lib.nmrfit_batch_normal_equations_im(self._h, _cabi.ptr(rows), _cabi.ptr(cs), _cabi.ptr(s),
                                                                   _cabi.ptr(A2), _cabi.ptr(g2), _cabi.ptr(f2)))
            out = []
            for k in range(self.K):
                d = self.D[k]
                Ak = A2[2 * aoff[k]:2 * aoff[k + 1]].reshape(2, d, d)
                gk = g2[2 * self.offsets[k]:2 * self.offsets[k + 1]].reshape(2, d)
                out.append(lsq.combine_channels([(Ak[ch], gk[ch], f2[2 * k + ch]) for ch in (0, 1)]))
            return out
        f = np.empty(self.K)
        _cabi.check(self._lib.nmrfit_batch_normal_equations(self._h, _cabi.ptr(rows), _cabi.ptr(cs), _cabi.ptr(s), _cabi.ptr(A),
                                                            _cabi.ptr(g), _cabi.ptr(f)))
        return [(A[aoff[k]:aoff[k + 1]].reshape(self.D[k], self.D[k]), g[self.offsets[k]:self.offsets[k + 1]], float(f[k]))
                for k in range(self.K)]

    # -- sandwich covariance (include/nmrfit_amd_cov.h) ----------------------------------------------
    def sandwich(self, X, sigma_u, sigma_v):
        """Per fit ``(A, M, g, f)`` at the K parameter vectors ``X``, ONE call for the batch: ``normal_equations``'s A, g
        and f (the same launches, bit for bit) and the meat M = J^T diag(q) J of the sandwich covariance (csrc/lsq_cov.hip),
        q_j the variance of fit k's weighted residual under noise ``sigma_u[k]``, ``sigma_v[k]`` on its two channels
        (scalars broadcast), from the batch's resident weights.  Bit-identical to
        ``lsq.ResidualModel(Evaluator(spectrum), lower, upper).sandwich(X[k], ...)`` fit by fit, in any batch.  A batch
        created with a ``fit_im`` mode is refused (``sandwich_im`` is its call).  The swarms are not touched.  D <= 76 for every fit."""
        from . import lsq
        if len(X) != self.K:
            raise ValueError("FitBatch.sandwich: one parameter vector per fit")
        su = np.ascontiguousarray(np.broadcast_to(np.asarray(sigma_u, dtype=np.float64), (self.K,)))
        sv = np.ascontiguousarray(np.broadcast_to(np.asarray(sigma_v, dtype=np.float64), (self.K,)))
        rows, cs = [], []
        s = 1.0 / np.sqrt(self.Ns.astype(np.float64))
        for k, x in enumerate(X):
            x = _cabi.f64(x)
            if x.shape != (self.D[k],):
                raise ValueError("FitBatch.sandwich: fit %d takes %d parameters" % (k, self.D[k]))
            r, h = lsq.forward_rows(x, self.lowers[k], self.uppers[k])
            rows.append(r.ravel())
            cs.append(s[k] / h)
        rows, cs = np.concatenate(rows), np.concatenate(cs)
        D = np.asarray(self.D, dtype=np.int64)
        aoff = np.concatenate(([0], np.cumsum(D * D)))
        A, M = np.empty(int(aoff[-1])), np.empty(int(aoff[-1]))
        g, f = np.empty(int(self.offsets[-1])), np.empty(self.K)
        _cabi.check(self._lib.nmrfit_batch_sandwich(self._h, _cabi.ptr(rows), _cabi.ptr(cs), _cabi.ptr(s), _cabi.ptr(su),
                                                    _cabi.ptr(sv), _cabi.ptr(A), _cabi.ptr(M), _cabi.ptr(g), _cabi.ptr(f)))
        return [(A[aoff[k]:aoff[k + 1]].reshape(self.D[k], self.D[k]), M[aoff[k]:aoff[k + 1]].reshape(self.D[k], self.D[k]),
                 g[self.offsets[k]:self.offsets[k + 1]], float(f[k])) for k in range(self.K)]

    def sandwich_im(self, X, sigma_u, sigma_v):
        """Per fit ``(parts, meat)`` at the K parameter vectors ``X`` of a batch created with a ``fit_im`` mode, ONE call
        for the batch (nmrfit_batch_sandwich_im): ``parts`` the channels' ``(A_ch, g_ch, rho_ch)`` --
        ``normal_equations(channels="both")``'s launches, bit for bit -- and ``meat`` [3, D + 1, D + 1] the blocks
        (rr, ii, ri) of the two-channel sandwich (csrc/lsq_cov_im.hip) under noise ``sigma_u[k]``, ``sigma_v[k]`` (scalars
        broadcast), from the batch's resident weights.  Bit-identical to
        ``lsq.ResidualModel(Evaluator(spectrum), lower, upper, fit_im=mode).sandwich_im(X[k], ...)`` fit by fit, in any
        batch.  The swarms are not touched.  D <= 76 for every fit."""
        from . import lsq
        if len(X) != self.K:
            raise ValueError("FitBatch.sandwich_im: one parameter vector per fit")
        su = np.ascontiguousarray(np.broadcast_to(np.asarray(sigma_u, dtype=np.float64), (self.K,)))
        sv = np.ascontiguousarray(np.broadcast_to(np.asarray(sigma_v, dtype=np.float64), (self.K,)))
        rows, cs = [], []
        s = 1.0 / np.sqrt(self.Ns.astype(np.float64))
        for k, x in enumerate(X):
            x = _cabi.f64(x)
            if x.shape != (self.D[k],):
                raise ValueError("FitBatch.sandwich_im: fit %d takes %d parameters" % (k, self.D[k]))
            r, h = lsq.forward_rows(x, self.lowers[k], self.uppers[k])
            rows.append(r.ravel())
            cs.append(s[k] / h)
        rows, cs = np.concatenate(rows), np.concatenate(cs)
        D = np.asarray(self.D, dtype=np.int64)
        aoff = np.concatenate(([0], np.cumsum(D * D)))
        moff = np.concatenate(([0], np.cumsum(3 * (D + 1) * (D + 1))))
        A2, g2, f2 = np.empty(2 * int(aoff[-1])), np.empty(2 * int(self.offsets[-1])), np.empty(2 * self.K)
        M = np.empty(int(moff[-1]))
        _cabi.check(self._lib.nmrfit_batch_sandwich_im(self._h, _cabi.ptr(rows), _cabi.ptr(cs), _cabi.ptr(s), _cabi.ptr(su),
                                                       _cabi.ptr(sv), _cabi.ptr(A2), _cabi.ptr(g2), _cabi.ptr(f2), _cabi.ptr(M)))
        out = []
        for k in range(self.K):
            d = self.D[k]
            Ak = A2[2 * aoff[k]:2 * aoff[k + 1]].reshape(2, d, d)
            gk = g2[2 * self.offsets[k]:2 * self.offsets[k + 1]].reshape(2, d)
            out.append(([(Ak[ch], gk[ch], float(f2[2 * k + ch])) for ch in (0, 1)], M[moff[k]:moff[k + 1]].reshape(3, d + 1, d + 1)))
        return out

    def uncertainty(self, X=None, sigma_u=None, sigma_v=None, channels="real"):
        """Per fit its ``uncertainty.FitUncertainty`` -- first-order standard errors of the parameters and of the
        satellite area fraction, and the distance from the local minimiser in standard errors -- from one ``sandwich``
        call and ``uncertainty.covariance`` per fit on the host.  ``X`` None: every fit's best position (``NmrfitError``
        with the state code before the first generation).  ``sigma_u``, ``sigma_v``: the noise of the two channels, one
        value or K; ``sigma_v`` None: ``sigma_u``'s.

        ``channels="both"`` (a batch created with a ``fit_im`` mode): one ``sandwich_im`` call and
        ``uncertainty.covariance_im`` per fit.  The errors belong to the minimiser of f = (rho_re + rho_im)/2, and
        ``distance`` is measured with grad f: ``polish(channels="both")`` is the polish that reaches that minimiser."""
        from . import uncertainty
        if channels not in ("real", "both"):
            raise ValueError('FitBatch.uncertainty: channels is "real" or "both"')
        if sigma_u is None:
            raise ValueError("FitBatch.uncertainty: give sigma_u (and sigma_v): the noise of the two channels")
        if sigma_v is None:
            sigma_v = sigma_u
        if X is None:
            X = [x for x, _ in self.best()]
        su = np.broadcast_to(np.asarray(sigma_u, dtype=np.float64), (self.K,))
        sv = np.broadcast_to(np.asarray(sigma_v, dtype=np.float64), (self.K,))
        if channels == "both":
            return [uncertainty.covariance_im(parts, meat, X[k], self.lowers[k], self.uppers[k],
                                              sigma=(float(su[k]), float(sv[k])))
                    for k, (parts, meat) in enumerate(self.sandwich_im(X, su, sv))]
        got = self.sandwich(X, su, sv)
        return [uncertainty.covariance(A, M, g, X[k], self.lowers[k], self.uppers[k], sigma=(float(su[k]), float(sv[k])))
                for k, (A, M, g, _) in enumerate(got)]

    def polish(self, X=None, which=None, channels="real", jac="2-point", **kwargs):
        """Least-squares refinement of the K fits in lock step (``lsq.lm_polish`` over ``normal_equations``): every
        launch evaluates the trial points of all fits still moving.  ``X`` None: from ``best()``.  ``which``: the fits
        to refine (default all); the others come back as they are.  Real-part objective only (fit_im=False batches).
        Returns per fit ``(x, f)``, f the rows launch's objective value at x -- never above the start's.

        ``channels="both"`` (a batch created with a ``fit_im`` mode): the same loop over the combined normal equations
        of both channels -- it minimises the objective the batch's swarms minimised, f = (rho_re + rho_im)/2.

        ``jac="analytic"`` (``channels="real"``): the loop runs over the analytic normal equations (one pass per step
        instead of D + 1 residual rows) and compares their own f = ||r||, the start's included.  After it ONE forward
        call at the final points gives the rows launch's f, which is what comes back; a fit whose closing f is not below
        its start's keeps its start.  (The two f of one point agree to rounding.  Only where a fit's whole gain is within
        1e-9 of its f -- far above what separates the two sums -- a second forward call, at the start points, decides.)"""
        from . import lsq
        if lsq._jac_form("FitBatch.polish", jac) == "analytic" and channels == "both":
            raise ValueError('FitBatch.polish: jac="analytic" covers the real channel only (channels="real")')
        start = self.best()
        if X is None:
            X = [x for x, _ in start]
        X = [_cabi.f64(x) for x in X]
        which = list(range(self.K)) if which is None else [int(k) for k in which]
        if not which:
            return [(x, fk) for x, (_, fk) in zip(X, start)]
        last = [x.copy() for x in X]

        def provider(trial):
            # (the launch covers the whole batch: a fit that has stopped is evaluated where it stands and ignored)
            full = list(last)
            for k, x in zip(which, trial):
                if x is not None:
                    full[k] = x
            got = self.normal_equations(full, channels=channels, jac=jac)
            return [None if x is None else got[k] for k, x in zip(which, trial)]
        Xw, fw, info = lsq.lm_polish(provider, [X[k] for k in which], [self.lowers[k] for k in which],
                                     [self.uppers[k] for k in which], **kwargs)
        out = [(x, fk) for x, (_, fk) in zip(X, start)]
        if jac == "analytic":
            # the rows launch's f at the final points; where a fit has moved, it must lie below the start's
            X0 = [np.clip(X[k], self.lowers[k], self.uppers[k]) for k in which]
            full = [x.copy() for x in X]
            for k, x in zip(which, Xw):
                full[k] = x
            closing = self.normal_equations(full, channels=channels)
            f_an0 = [h[0] for h in info["history"]]
            moved = [i for i, n in enumerate(info["accepted"]) if n > 0]
            opening = None
            if any(not closing[which[i]][2] < f_an0[i] * (1.0 - 1e-9) for i in moved):
                for k, x in zip(which, X0):
                    full[k] = x
                opening = self.normal_equations(full, channels=channels)
            for i, k in enumerate(which):
                if i in moved and opening is not None and not closing[k][2] < opening[k][2]:
                    out[k] = (X0[i], float(opening[k][2]))
                else:
                    out[k] = (Xw[i], float(closing[k][2]))
            info["kept_start"] = [i in moved and opening is not None and not closing[which[i]][2] < opening[which[i]][2]
                                  for i in range(len(which))]
        else:
            for k, x, fk in zip(which, Xw, fw):
                out[k] = (x, float(fk))
        self.last_polish = info
        return out

    # -- diagnostics (include/nmrfit_amd_diag.h) ----------------------------------------------------
    def step(self):
        """Generation 0 on the first call, then one generation per call (asynchronous)."""
        _cabi.check(self._lib.nmrfit_batch_step(self._h))

    def synchronize(self):
        _cabi.check(self._lib.nmrfit_batch_synchronize(self._h))

    def set_geometry(self, mode):
        """"workgroup" (a workgroup per particle) or "wave" (a wave per particle); bit-identical results."""
        if isinstance(mode, str):
            mode = {"workgroup": 0, "wave": 1}[mode.lower()]
        _cabi.check(self._lib.nmrfit_batch_set_geometry(self._h, int(mode)))

    def geometry(self):
        m, w, s = ctypes.c_int32(0), ctypes.c_int32(0), ctypes.c_int32(0)
        n = ctypes.c_int64(0)
        _cabi.check(self._lib.nmrfit_batch_geometry(self._h, ctypes.byref(m), ctypes.byref(w), ctypes.byref(s),
                                                    ctypes.byref(n)))
        return dict(mode=("workgroup", "wave")[m.value], waves_per_workgroup=w.value, segments=s.value,
                    workgroups=n.value)

    def state(self, k):
        D, S = self.D[k], int(self.Ss[k])
        x = np.empty((S, D)); v = np.empty_like(x); p = np.empty_like(x)
        fx = np.empty(S); fp = np.empty(S)
        _cabi.check(self._lib.nmrfit_batch_get_state(self._h, int(k), _cabi.ptr(x), _cabi.ptr(v), _cabi.ptr(p),
                                                     _cabi.ptr(fx), _cabi.ptr(fp)))
        return dict(x=x, v=v, p=p, fx=fx, fp=fp)

"""
nmrfit_amd -- MI355X (gfx950) evaluator for nmrfit's objective function and the swarm loop
around it, behind the reference's own API for that path:

    nmrfit_amd.fit(data, lower, upper, ...) -> FitUtility        (nmrfit/core.py:64)
    nmrfit_amd.fit_many([(data, lower, upper), ...])             several spectra: one DEVICE BATCH, a launch per generation
    nmrfit_amd.batch.FitBatch(spectra, lowers, uppers, ...)      the batch itself (nmrfit_batch_* of the library)
    nmrfit_amd.equations.objective(x, w, u, v, weights)          (nmrfit/equations.py:152)
    nmrfit_amd.equations.Evaluator(...).objective_batch(X)       one launch per swarm generation
    nmrfit_amd.pso.DeviceSwarm / pso.pso                         (replaces pyswarm.pso)
    nmrfit_amd.Data(w, u, v)                                     (nmrfit/containers.py:8, scripted use)
    nmrfit_amd.shift_phase_many(datas, method='auto')            Data.shift_phase for many spectra: the phase search on the DEVICE
    nmrfit_amd.select_peaks_many(datas, method='auto')           Data.select_peaks for many spectra: peak picking on the DEVICE
    nmrfit_amd.utils.compute_weights_many(ws, peaks_list)        FitUtility._compute_weights for many spectra on the DEVICE
    nmrfit_amd.fit_replicas(data, lower, upper, replicas=32, sigma=...)   noise-replica uncertainty: the noisy copies made on the
                                                                 DEVICE, all refits one batch -> ReplicaFits (area_fraction_std, ...)
    nmrfit_amd.fit_replicas_many(jobs, replicas=32)              the same for several spectra, packed into ragged batches
    nmrfit_amd.noise.replicas(us, vs, sigma_u, sigma_v, seeds)   the noisy copies alone (noise.normals / replicas_host: the numpy mirror)
    nmrfit_amd.fit_many(jobs, quality=True)                      every fit carries fit.quality: residual statistics per peak region,
                                                                 reduced on the DEVICE (residual_stats / residual_stats_many alone)
    nmrfit_amd.sample_noise_many(ws, ys, regions)                utils.sample_noise for many spectra on the DEVICE (baseline.fit_many:
                                                                 a conditioned polynomial fit over a masked part of a grid)
    nmrfit_amd.correct_baseline_many(datas, deg=1)               a polynomial baseline fitted outside the peaks and taken out of V, I, u, v
    nmrfit_amd.fit_many(jobs, residual_baseline=1)               every fit carries fit.residual_baseline: the baseline of data_V - V
    nmrfit_amd.fit_many(jobs, uncertainty=dict(sigma=s))         every fit carries fit.uncertainty: first-order standard errors of its
                                                                 parameters and area fraction (the sandwich covariance, one launch)
    nmrfit_amd.fit_many(jobs, fit_im="sum", batch_polish="both", uncertainty=dict(sigma=s, channels="both"))
                                                                 the same for fit_im fits: the two-channel sandwich

    nmrfit_amd.spectra_from_fids(fids, sw, sfrq, tof, zero_fill="pow2")   raw FIDs to Data on the DEVICE: a batched fp64 Fourier
                                                                 transform, core.load's centring, reversal, normalisation and
                                                                 trace sum (fid.transform_many alone; the file readers stay out)

Everything that evaluates the objective goes through libnmrfit_amd.so (include/nmrfit_amd.h);
there is no CPU fallback.  The automatic phase estimate and the automatic peak picking run on the device too when
asked for by shift_phase_many / proc_autophase.approximate_phase_many and select_peaks_many / peaks.find_peaks_many
(opt-in: Data.shift_phase and Data.select_peaks stay the reference's host paths).  The error weights of a fit are host
code as in the reference unless fit_many(jobs, device_weights=True) / FitBatch(regions=...) /
utils.compute_weights_many ask for them on the device (include/nmrfit_amd_prep.h; bit-identical to the host's); the
bounds are host code.  Instrument I/O (nmrfit.load), the
matplotlib click selectors and plotting are out of scope.
"""
from .core import fit, fit_many  # noqa: F401
from . import baseline, batch, containers, equations, fid, noise, peaks, proc_autophase, pso, quality, synth, uncertainty, utils  # noqa: F401
from .uncertainty import FitUncertainty  # noqa: F401
from .quality import FitQuality, residual_stats, residual_stats_many  # noqa: F401
from .noise import fit_replicas, fit_replicas_many  # noqa: F401
from .containers import Data, correct_baseline_many, select_peaks_many, shift_phase_many  # noqa: F401
from .baseline import BaselineFit, sample_noise_many, subtract_rotated  # noqa: F401
from .fid import spectra_from_fids  # noqa: F401

__version__ = "0.1.0"

#!/usr/bin/env python3
"""What the polynomial baselines on the device cost, against the host loops they replace.

200 default synthetic spectra (4096 points, 6 peaks, 204 particles), pyswarm's stopping rule on:

  noise level
    A   baseline.sample_noise_many on both channels of every spectrum: one library call (csrc/baseline.hip)
    B   the host loop: peaks.sample_noise (np.polyfit on raw ppm values) on both channels, spectrum after spectrum
  residual baseline
    A'  fit_many(jobs, residual_baseline=1): 17 doubles per fit, fitted while each batch is resident
    B'  fit_many(jobs, generate=True), then np.polyfit per spectrum on data_V - V outside the peaks' bounds: the
        (2 P + 6) N doubles of the reconstruction to the host
    C   fit_many(jobs): the fits alone

Same process, alternating sides, wall clock around whole calls, after a warm-up of every side; best of --reps and the
spread (max - min) / min of each side's own runs; A' / C and B' / C are ratios of RATES (1: the baseline is free).

    python tools/baseline_ab.py [--reps 3] [--jobs 200] [--out profiles/r17/baseline_ab.txt]

The kernels' own times are not a wall clock's to give: --kernel-only runs sides A and A' a few times and nothing else,
for a run of its own under the profiler,

    rocprofv3 --kernel-trace --stats -d DIR -- python tools/baseline_ab.py --kernel-only

whose kernel statistics hold the lines of baseline_jobs_kernel and baseline_residual_kernel.
"""
import argparse
import contextlib
import io
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import nmrfit_amd  # noqa: E402
from nmrfit_amd import baseline, peaks, synth  # noqa: E402

NOISE_REGION = (3.0, 3.1)      # 410 of the 4096 points


def make_jobs(n, **options):
    jobs = []
    for k in range(n):
        sp = synth.make_spectrum(4096, 6, seed=1 + k)
        jobs.append(dict(data=synth.SynthData(sp["w"], sp["u"], sp["v"], sp["peaks"]), lower=list(sp["lower"]),
                         upper=list(sp["upper"]), options=dict(options, seed=1000 + k)))
    return jobs


def noise_a(jobs):
    ds = [j["data"] for j in jobs]
    return baseline.sample_noise_many([d.w for d in ds], [np.array([d.u, d.v]) for d in ds], NOISE_REGION)


def noise_b(jobs):
    return [(peaks.sample_noise(j["data"].w, j["data"].u, *NOISE_REGION), peaks.sample_noise(j["data"].w, j["data"].v, *NOISE_REGION))
            for j in jobs]


def fits_a(jobs):
    return [f.residual_baseline for f in nmrfit_amd.fit_many(jobs, residual_baseline=1)]


def fits_b(jobs):
    out = []
    for f in nmrfit_amd.fit_many(jobs, generate=True):
        m = baseline.mask_of(f.data.w, [tuple(p.bounds) for p in f.data.peaks], True)
        out.append(np.polyfit(f.data.w[m], (f.data.V - f.V)[m], 1))
    return out


def fits_c(jobs):
    return nmrfit_amd.fit_many(jobs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--jobs", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                  "profiles", "r17", "baseline_ab.txt"))
    ap.add_argument("--kernel-only", action="store_true", help="only sides A and A', three times (for rocprofv3)")
    a = ap.parse_args()
    n = a.jobs
    sides = (("A", noise_a), ("B", noise_b), ("A'", fits_a), ("B'", fits_b), ("C", fits_c))
    with contextlib.redirect_stdout(io.StringIO()):
        if a.kernel_only:
            for _ in range(3):
                noise_a(make_jobs(n))
                fits_a(make_jobs(n))
            return
        for name, side in sides:                                   # warm-up of every side
            side(make_jobs(min(n, 40), maxiter=20))
        runs = {name: [] for name, _ in sides}
        got = {}
        for _ in range(a.reps):
            for name, side in sides:
                jobs = make_jobs(n)
                t0 = time.perf_counter()
                got[name] = side(jobs)
                runs[name].append(time.perf_counter() - t0)
    sa, sb = np.array(got["A"], dtype=float), np.array(got["B"], dtype=float)
    best = {k: min(v) for k, v in runs.items()}
    row = dict(jobs=n, reps=a.reps, runs_s=runs, per_s={k: n / best[k] for k in best},
               spread={k: (max(v) - min(v)) / min(v) for k, v in runs.items()},
               A_over_B=best["B"] / best["A"], A1_over_C=best["C"] / best["A'"], B1_over_C=best["C"] / best["B'"],
               sigma_max_rel_diff_A_B=float(np.max(np.abs(sa - sb) / sb)),
               residual_baseline_status0=int(sum(1 for r in got["A'"] if r.status == 0)))
    print(json.dumps(row), flush=True)
    lines = ["%-4s %12s %12s %8s" % ("side", "best s", "spectra/s", "spread")]
    for k, _ in sides:
        lines.append("%-4s %12.4f %12.1f %7.1f%%" % (k, best[k], n / best[k], 100 * row["spread"][k]))
    lines.append("A / B = %.3f   A' / C = %.3f   B' / C = %.3f   (rates; A: sample_noise_many, B: the host loop of peaks.sample_noise;"
                 % (row["A_over_B"], row["A1_over_C"], row["B1_over_C"]))
    lines.append("A': fit_many(residual_baseline=1), B': generate=True + np.polyfit per spectrum, C: the fits alone;")
    lines.append("%d default jobs 4096 x 6, 204 particles, pyswarm's stopping rule; alternating, best of %d;" % (n, a.reps))
    lines.append("largest relative difference of A's sigmas from B's: %.3g; A' fitted %d of %d residuals)"
                 % (row["sigma_max_rel_diff_A_B"], row["residual_baseline_status0"], n))
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(json.dumps(row) + "\n" + text + "\n")


if __name__ == "__main__":
    main()

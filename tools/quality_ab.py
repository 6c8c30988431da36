#!/usr/bin/env python3
"""What the residual statistics on the device cost a fit_many call, against reading the reconstruction back for them.

200 default synthetic spectra (4096 points, 6 peaks, 204 particles), pyswarm's stopping rule on:

  A  fit_many(jobs, quality=True): the rows reduced on the device while each batch is resident (csrc/quality.hip),
     (P + 2) x 64 bytes per fit to the host
  B  fit_many(jobs, generate=True), then quality.residual_stats_host per fit: the (2 P + 6) N doubles of the
     reconstruction to the host and the numpy mirror on them
  C  fit_many(jobs): the fits alone

Same process, alternating A, B, C, wall clock around whole calls, after a warm-up of all three; best of --reps and the
spread (max - min) / min of each side's own runs; A / C and B / C are ratios of RATES (1: the statistics are free).

    python tools/quality_ab.py [--reps 3] [--jobs 200] [--out profiles/r08/quality_ab.txt]

The two kernels' own times are not a wall clock's to give: --kernel-only runs side A a few times and nothing else, for a
run of its own under the profiler,

    rocprofv3 --kernel-trace --stats -d DIR -- python tools/quality_ab.py --kernel-only

whose kernel statistics hold the lines of quality_tiles_kernel and quality_fold_kernel.
"""
import argparse
import contextlib
import io
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import nmrfit_amd  # noqa: E402
from nmrfit_amd import quality, synth  # noqa: E402


def make_jobs(n, **options):
    jobs = []
    for k in range(n):
        sp = synth.make_spectrum(4096, 6, seed=1 + k)
        jobs.append(dict(data=synth.SynthData(sp["w"], sp["u"], sp["v"], sp["peaks"]), lower=list(sp["lower"]),
                         upper=list(sp["upper"]), options=dict(options, seed=1000 + k)))
    return jobs


def side_a(jobs):
    return [f.quality for f in nmrfit_amd.fit_many(jobs, quality=True)]


def side_b(jobs):
    out = []
    for f in nmrfit_amd.fit_many(jobs, generate=True):
        bounds = [tuple(p.bounds) for p in f.data.peaks]
        out.append(quality.FitQuality(quality.residual_stats_host(f.V, f.data.V, f.data.w, bounds), nparams=len(f.lower)))
    return out


def side_c(jobs):
    return nmrfit_amd.fit_many(jobs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--jobs", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                  "profiles", "r08", "quality_ab.txt"))
    ap.add_argument("--kernel-only", action="store_true", help="only side A, three times (for rocprofv3)")
    a = ap.parse_args()
    n = a.jobs
    sides = (("A", side_a), ("B", side_b), ("C", side_c))
    with contextlib.redirect_stdout(io.StringIO()):
        if a.kernel_only:
            for _ in range(3):
                side_a(make_jobs(n))
            return
        for _, side in sides:                                   # warm-up of all three
            side(make_jobs(min(n, 40), maxiter=20))
        runs = {name: [] for name, _ in sides}
        got = {}
        for _ in range(a.reps):
            for name, side in sides:
                jobs = make_jobs(n)
                t0 = time.perf_counter()
                got[name] = side(jobs)
                runs[name].append(time.perf_counter() - t0)
    same = all(qa.rows.tobytes() == qb.rows.tobytes() for qa, qb in zip(got["A"], got["B"]))
    best = {k: min(v) for k, v in runs.items()}
    row = dict(jobs=n, reps=a.reps, runs_s=runs, fits_per_s={k: n / best[k] for k in best},
               spread={k: (max(v) - min(v)) / min(v) for k, v in runs.items()},
               A_over_C=best["C"] / best["A"], B_over_C=best["C"] / best["B"], rows_of_A_equal_rows_of_B=same)
    print(json.dumps(row), flush=True)
    lines = ["%-4s %12s %10s %8s" % ("side", "best s", "fits/s", "spread")]
    for k in ("A", "B", "C"):
        lines.append("%-4s %12.4f %10.1f %7.1f%%" % (k, best[k], n / best[k], 100 * row["spread"][k]))
    lines.append("A / C = %.3f   B / C = %.3f   (rates; A: quality=True, B: generate=True + residual_stats_host, C: the fits alone;"
                 % (row["A_over_C"], row["B_over_C"]))
    lines.append("%d default jobs 4096 x 6, 204 particles, pyswarm's stopping rule; alternating, best of %d; rows of A == rows of B: %s)"
                 % (n, a.reps, same))
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(json.dumps(row) + "\n" + text + "\n")


if __name__ == "__main__":
    main()

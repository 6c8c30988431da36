#!/usr/bin/env python3
"""The error weights on the host against the device, and what that is worth to fit_many.

1. utils.compute_weights spectrum after spectrum against utils.compute_weights_many, whole calls with the copies, for
   200 x (4096 points, 6 peaks) and 50 x (65536, 24): wall clock after a warm-up call, best of --reps.
2. nmrfit_amd.fit_many on 200 and 1000 default synthetic jobs (4096 x 6, 204 particles), with pyswarm's stopping rule
   and with all 2000 generations (minstep = minfunc = -1), without and with device_weights=True: same process,
   alternating, best of --reps, and the spread (max - min) / min of each configuration's own runs.

    python tools/weights_timing.py [--reps 3] [--jobs 200 1000] [--out profiles/weights_timing.txt]
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
from nmrfit_amd import synth, utils  # noqa: E402


def weights_rows(reps):
    rows = []
    for S, N, P in ((200, 4096, 6), (50, 65536, 24)):
        sps = [synth.make_spectrum(N, P, seed=100 + k) for k in range(S)]
        ws, pks = [s["w"] for s in sps], [s["peaks"] for s in sps]
        utils.compute_weights_many(ws[:2], pks[:2])          # warm-up (library load, first launch)
        host, dev = [], []
        for _ in range(reps):
            t0 = time.perf_counter()
            want = [utils.compute_weights(w, pk) for w, pk in zip(ws, pks)]
            host.append(time.perf_counter() - t0)
            t0 = time.perf_counter()
            got = utils.compute_weights_many(ws, pks)
            dev.append(time.perf_counter() - t0)
        same = all(np.array_equal(a, b) for a, b in zip(got, want))
        rows.append(dict(kind="weights", S=S, N=N, P=P, host_s=min(host), device_s=min(dev), host_ms_per_fit=1e3 * min(host) / S,
                         device_ms_per_fit=1e3 * min(dev) / S, speedup=min(host) / min(dev), bit_identical=same))
        print(json.dumps(rows[-1]), flush=True)
    return rows


def fit_many_rows(reps, job_counts):
    specs = [synth.make_spectrum(4096, 6, seed=100 + k % 8) for k in range(8)]

    def jobs(n, extra):
        return [dict(data=synth.SynthData(specs[k % 8]["w"], specs[k % 8]["u"], specs[k % 8]["v"], specs[k % 8]["peaks"]),
                     lower=list(specs[k % 8]["lower"]), upper=list(specs[k % 8]["upper"]), options=dict(extra, seed=7 + k))
                for k in range(n)]

    def run(n, extra, flag):
        with contextlib.redirect_stdout(io.StringIO()):
            t0 = time.perf_counter()
            fits = nmrfit_amd.fit_many(jobs(n, extra), device_weights=flag)
            return time.perf_counter() - t0, fits
    run(8, {}, False)
    run(8, {}, True)
    rows = []
    for n in job_counts:
        for rule, extra in (("pyswarm", {}), ("all 2000", {"minstep": -1.0, "minfunc": -1.0})):
            times = {False: [], True: []}
            same = True
            for _ in range(reps):
                results = {}
                for flag in (False, True):
                    t, results[flag] = run(n, extra, flag)
                    times[flag].append(t)
                same = same and all(np.array_equal(a.params, b.params) and a.error == b.error
                                    for a, b in zip(results[False], results[True]))
            host, dev = times[False], times[True]
            rows.append(dict(kind="fit_many", jobs=n, rule=rule, host_weights_fits_per_s=n / min(host),
                             device_weights_fits_per_s=n / min(dev), host_runs_s=host, device_runs_s=dev,
                             host_spread=(max(host) - min(host)) / min(host), ratio=min(host) / min(dev), same_results=same))
            print(json.dumps(rows[-1]), flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--jobs", type=int, nargs="*", default=[200, 1000])
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                  "profiles", "weights_timing.txt"))
    a = ap.parse_args()
    rows = weights_rows(a.reps) + fit_many_rows(a.reps, a.jobs)
    lines = ["%4s x (%6s, %2s)  %14s %14s %9s  %s" % ("S", "N", "P", "host ms / fit", "device ms / fit", "speed-up", "bits")]
    for r in rows:
        if r["kind"] == "weights":
            lines.append("%4d x (%6d, %2d)  %14.3f %14.4f %8.1fx  %s" % (r["S"], r["N"], r["P"], r["host_ms_per_fit"],
                                                                       r["device_ms_per_fit"], r["speedup"],
                                                                       "identical" if r["bit_identical"] else "DIFFER"))
    lines.append("(host: utils.compute_weights per spectrum; device: utils.compute_weights_many, whole call; best of %d)" % a.reps)
    lines.append("%5s %-9s %16s %18s %7s %12s  %s" % ("jobs", "rule", "host weights f/s", "device weights f/s", "ratio",
                                                     "host spread", "results"))
    for r in rows:
        if r["kind"] == "fit_many":
            lines.append("%5d %-9s %16.1f %18.1f %7.3f %11.1f%%  %s" % (r["jobs"], r["rule"], r["host_weights_fits_per_s"],
                                                                       r["device_weights_fits_per_s"], r["ratio"],
                                                                       100 * r["host_spread"],
                                                                       "identical" if r["same_results"] else "DIFFER"))
    lines.append("(fit_many on default synthetic jobs, 4096 x 6, 204 particles; alternating, best of %d; ratio > 1: the "
                 "flagged call is faster; host spread: (max - min) / min of the unflagged call's own runs)" % a.reps)
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(json.dumps(r) for r in rows) + "\n" + text + "\n")


if __name__ == "__main__":
    main()

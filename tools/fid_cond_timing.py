#!/usr/bin/env python3
"""What the conditioning of raw FIDs on the device costs (Bruker group-delay removal, form "fid", and a window), against
the plain device transform and against the numpy restatement.

K = 200 FIDs of 2^16 complex points (one trace each), g = 68.0, an exponential window with first-point scaling, zero
fill x 2 (n = 2^17); host arrays in and host arrays out on every side:

  A    fid.transform_many(grpdly=68.0, window=W, zero_fill=2^17): one library call (csrc/fid_cond.hip)
  P    fid.transform_many(zero_fill=2^17) on the same FIDs: the call without conditioning -- A - P is the price of
       conditioning on the device
  B    fid.condition_host + fid.finish_host, FID after FID, on one thread
  B16  the same loop over a pool of at most 16 threads

Same process, alternating sides, wall clock around whole calls, after a warm-up of every side; best of 2 x --reps and
the spread (max - min) / min of each side's own runs.  No ratio is a pass condition.

    python tools/fid_cond_timing.py [--reps 5] [--fids 200] [--log2 16] [--out profiles/fid_cond_timing.txt]

The kernels' own times are not a wall clock's to give: --kernel-only runs side A a few times and nothing else, for a
run of its own under the profiler (no counters in that run),

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/fid_cond_timing.py --kernel-only

whose kernel statistics hold one line per fid_*_kernel and fidc_*_kernel.
"""
import argparse
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nmrfit_amd import fid, synth  # noqa: E402

G = 68.0


def make_fids(K, n):
    lines = [(-0.2, 40.0 / n, 1.0), (0.05, 40.0 / n, 0.7, 0.2), (0.31, 60.0 / n, 0.5, -0.4)]
    return [synth.make_fid(n, lines, seed=1 + k, noise=0.01, grpdly=G).fid for k in range(K)]


def timed(fn, reps):
    runs = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        runs.append(time.perf_counter() - t0)
    return min(runs), (max(runs) - min(runs)) / min(runs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--fids", type=int, default=200)
    ap.add_argument("--log2", type=int, default=16)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--out", default=None)
    ap.add_argument("--kernel-only", action="store_true")
    args = ap.parse_args()
    s, K = 1 << args.log2, args.fids
    n = 2 * s
    fids = make_fids(K, s)
    W = fid.window_em(fid.conditioned_length(s, G), 1.0, 10000.0, first_point=0.5)
    side_a = lambda: fid.transform_many(fids, zero_fill=n, grpdly=G, window=W)      # noqa: E731
    if args.kernel_only:
        for _ in range(4):
            side_a()
        return
    threads = max(1, min(args.threads, 16, os.cpu_count() or 1))
    pool = ThreadPoolExecutor(max_workers=threads)
    host_one = lambda x: fid.finish_host(fid.condition_host(x, G, "fid", W, n)[1])      # noqa: E731
    side_p = lambda: fid.transform_many(fids, zero_fill=n)      # noqa: E731
    side_b = lambda: [host_one(x) for x in fids]      # noqa: E731
    side_b16 = lambda: list(pool.map(host_one, fids))      # noqa: E731
    got, want = side_a(), side_b()      # (the warm-up, and a look at the agreement)
    side_p()
    side_b16()
    worst = max(float(np.abs(g[0] - w[0]).max()) for g, w in zip(got, want))
    sides = (("A", side_a), ("P", side_p), ("B", side_b), ("B16", side_b16))
    results = {}
    for _ in range(2):      # alternate
        for name, fn in sides:
            best, spread = timed(fn, args.reps)
            if name not in results or best < results[name][0]:
                results[name] = (best, spread)
    label = {"A": "fid.transform_many(grpdly=, window=) (device)", "P": "fid.transform_many, no conditioning (device)",
             "B": "condition_host + finish_host, one thread", "B16": "condition_host + finish_host, %2d threads" % threads}
    text = ["tools/fid_cond_timing.py: %d FIDs of 2^%d complex points, one trace each, g = %.1f (form fid), exponential window, "
            "n = 2^%d, best of 2 x %d runs per side" % (K, args.log2, G, args.log2 + 1, args.reps)]
    for name, _ in sides:
        text.append("  %-4s %-48s %9.3f ms   %8.4f ms per FID   spread %.2f"
                    % (name, label[name], 1e3 * results[name][0], 1e3 * results[name][0] / K, results[name][1]))
    text.append("  A - P %.3f ms (%.4f ms per FID)   A / P %.2f   B / A %.2f   B16 / A %.2f   worst |u_A - u_B| %.3g (max u = 1)"
                % (1e3 * (results["A"][0] - results["P"][0]), 1e3 * (results["A"][0] - results["P"][0]) / K,
                   results["A"][0] / results["P"][0], results["B"][0] / results["A"][0], results["B16"][0] / results["A"][0], worst))
    print("\n".join(text))
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(text) + "\n")


if __name__ == "__main__":
    main()

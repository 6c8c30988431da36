#!/usr/bin/env python3
"""What the FID transform on the device costs, against the numpy restatement of the reference's lines.

K = 200 FIDs of 2^16 complex points (one trace each), host arrays in and host arrays out on both sides:

  A   fid.transform_many: one library call -- upload, at most six launches (csrc/fid.hip), u, v and rows back
  B   fid.transform_host, FID after FID, on one thread (np.fft.fft + fftshift, complex max, complex division)
  B16 the same loop over a pool of at most 16 threads (np.fft releases the interpreter lock)

Same process, alternating sides, wall clock around whole calls, after a warm-up of every side; best of --reps and the
spread (max - min) / min of each side's own runs.  The comparison of record is A against B / B16, never the device
code against itself.

    python tools/fid_timing.py [--reps 5] [--fids 200] [--log2 16] [--out profiles/fid_timing.txt]

The kernels' own times are not a wall clock's to give: --kernel-only runs side A a few times and nothing else, for a
run of its own under the profiler,

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/fid_timing.py --kernel-only

whose kernel statistics hold one line per fid_*_kernel.
"""
import argparse
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nmrfit_amd import fid, synth  # noqa: E402


def make_fids(K, n):
    lines = [(-0.2, 40.0 / n, 1.0), (0.05, 40.0 / n, 0.7, 0.2), (0.31, 60.0 / n, 0.5, -0.4)]
    return [synth.make_fid(n, lines, seed=1 + k, noise=0.01).fid for k in range(K)]


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
    n, K = 1 << args.log2, args.fids
    fids = make_fids(K, n)
    side_a = lambda: fid.transform_many(fids)      # noqa: E731
    if args.kernel_only:
        for _ in range(4):
            side_a()
        return
    threads = max(1, min(args.threads, 16, os.cpu_count() or 1))
    pool = ThreadPoolExecutor(max_workers=threads)
    side_b = lambda: [fid.transform_host(x) for x in fids]      # noqa: E731
    side_b16 = lambda: list(pool.map(fid.transform_host, fids))      # noqa: E731
    got, want = side_a(), side_b()      # (the warm-up, and a look at the agreement)
    side_b16()
    worst = max(float(np.abs(g[0] - w[0]).max()) for g, w in zip(got, want))
    results = {}
    for _ in range(2):      # alternate
        for name, fn in (("A", side_a), ("B", side_b), ("B16", side_b16)):
            best, spread = timed(fn, args.reps)
            if name not in results or best < results[name][0]:
                results[name] = (best, spread)
    text = ["tools/fid_timing.py: %d FIDs of 2^%d complex points, one trace each, best of 2 x %d runs per side" % (K, args.log2, args.reps),
            "  A    fid.transform_many (device, host arrays in and out)   %9.3f ms   %8.4f ms per FID   spread %.2f"
            % (1e3 * results["A"][0], 1e3 * results["A"][0] / K, results["A"][1]),
            "  B    fid.transform_host, one thread                        %9.3f ms   %8.4f ms per FID   spread %.2f"
            % (1e3 * results["B"][0], 1e3 * results["B"][0] / K, results["B"][1]),
            "  B16  fid.transform_host, %2d threads                         %9.3f ms   %8.4f ms per FID   spread %.2f"
            % (threads, 1e3 * results["B16"][0], 1e3 * results["B16"][0] / K, results["B16"][1]),
            "  B / A %.2f   B16 / A %.2f   worst |u_A - u_B| %.3g (max u = 1)" % (results["B"][0] / results["A"][0],
                                                                                  results["B16"][0] / results["A"][0], worst)]
    print("\n".join(text))
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(text) + "\n")


if __name__ == "__main__":
    main()

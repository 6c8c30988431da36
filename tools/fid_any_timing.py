#!/usr/bin/env python3
"""What the exact-length transform of raw FIDs on the device costs (any_length=True: the chirp-z path of
csrc/fid_any.hip), against what the device could do before for the same FIDs and against numpy at the exact length.

K = 200 FIDs of 65466 = 2^16 - 70 complex points (one trace each: what form 1 leaves of 2^16 points at g = 68.0); host
arrays in and host arrays out on every side:

  A    fid.transform_many(any_length=True): one library call, n = 65466, M = 2^17
  P    fid.transform_many(zero_fill="pow2") on the same FIDs: n = 2^16, the grid the device could make before
  B    fid.transform_host at the exact length (np.fft), FID after FID, on one thread
  B16  the same loop over a pool of at most 16 threads

Same process, alternating sides, wall clock around whole calls, after a warm-up of every side; best of 2 x --reps and
the spread (max - min) / min of each side's own runs.  No ratio is a pass condition.

    python tools/fid_any_timing.py [--reps 5] [--fids 200] [--points 65466] [--out profiles/fid_any_timing.txt]

The kernels' own times are not a wall clock's to give: --kernel-only runs side A, --kernel-only-pow2 side P, a few
times and nothing else, for runs of their own under the profiler (no counters in those runs),

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/fid_any_timing.py --kernel-only

--probe: the errors and call times at the lengths of the device tests and at N = 65466 and 2^21 - 1 (T = 1), run once,
outside the suite: the device's error and that of numpy's own fp64 np.fft.fft at the same length on the same FID, both
against fid.bluestein_host in long double, in units of u ||Y||_2, and the device's error over the header's bar.
"""
import argparse
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nmrfit_amd import fid, synth  # noqa: E402

U = 2.0 ** -53


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


def header_bar(x, N):
    """include/nmrfit_amd_fid_any.h's first-order bar on || Y^ - Y ||_2 for x given exactly (mu = u)."""
    g2, g4 = 2 * U / (1 - 2 * U), 4 * U / (1 - 4 * U)
    eta, kappa = U + g4 * (np.sqrt(2.0) + U), U + np.sqrt(2.0) * g2 * (1 + U)
    eps, beta = np.log2(fid.conv_length(N)) * eta, fid.filter_peak(N)
    norm = float(np.sqrt((np.abs(x) ** 2).sum()))
    return (beta * (2 * eps + 2 * kappa + np.sqrt(2.0) * g2) + (eps + U) * np.sqrt(x.shape[-1] * (2.0 * N - 1))) * norm


def probe(out):
    text = ["tools/fid_any_timing.py --probe: one FID of N points (T = 1) per length; errors against fid.bluestein_host in long "
            "double, in units of u ||Y||_2",
            "%9s %9s  %12s %12s %12s  %10s" % ("N", "M", "device", "np.fft fp64", "device / bar", "call ms")]
    for N in (3, 7, 12, 1000, 2047, 2049, 4027, 4099, 5000, 65466, (1 << 21) - 1):
        x = make_fids(1, N)[0]
        fid.transform_many([x], any_length=True)                                  # (warm-up)
        t0 = time.perf_counter()
        Y = fid.transform_many([x], any_length=True, return_transform=True)[0][3]
        ms = 1e3 * (time.perf_counter() - t0)
        want = fid.bluestein_host(x.astype(np.clongdouble), N)
        norm = float(np.sqrt((np.abs(want) ** 2).sum()))
        err = float(np.sqrt((np.abs(Y.astype(np.clongdouble) - want) ** 2).sum()))
        own = np.fft.fftshift(np.fft.fft(x, axis=-1), axes=-1)
        err_np = float(np.sqrt((np.abs(own.astype(np.clongdouble) - want) ** 2).sum()))
        text.append("%9d %9d  %12.3f %12.3f %12.3g  %10.2f" % (N, fid.conv_length(N), err / norm / U, err_np / norm / U,
                                                              err / header_bar(x, N), ms))
        print(text[-1], flush=True)
    if out:
        with open(out, "w") as fh:
            fh.write("\n".join(text) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--fids", type=int, default=200)
    ap.add_argument("--points", type=int, default=(1 << 16) - 70)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--out", default=None)
    ap.add_argument("--kernel-only", action="store_true")
    ap.add_argument("--kernel-only-pow2", action="store_true")
    ap.add_argument("--probe", action="store_true")
    args = ap.parse_args()
    if args.probe:
        probe(args.out)
        return
    N, K = args.points, args.fids
    fids = make_fids(K, N)
    side_a = lambda: fid.transform_many(fids, any_length=True)      # noqa: E731
    side_p = lambda: fid.transform_many(fids, zero_fill="pow2")      # noqa: E731
    if args.kernel_only or args.kernel_only_pow2:
        for _ in range(4):
            (side_a if args.kernel_only else side_p)()
        return
    threads = max(1, min(args.threads, 16, os.cpu_count() or 1))
    pool = ThreadPoolExecutor(max_workers=threads)
    side_b = lambda: [fid.transform_host(x) for x in fids]      # noqa: E731
    side_b16 = lambda: list(pool.map(fid.transform_host, fids))      # noqa: E731
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
    n2 = fid.transform_length(N, "pow2")
    label = {"A": "fid.transform_many(any_length=True), n = %d (device)" % N, "P": "fid.transform_many(zero_fill='pow2'), n = %d (device)" % n2,
             "B": "transform_host at n = %d, one thread" % N, "B16": "transform_host at n = %d, %2d threads" % (N, threads)}
    text = ["tools/fid_any_timing.py: %d FIDs of %d complex points, one trace each, best of 2 x %d runs per side" % (K, N, args.reps)]
    for name, _ in sides:
        text.append("  %-4s %-58s %9.3f ms   %8.4f ms per FID   spread %.2f"
                    % (name, label[name], 1e3 * results[name][0], 1e3 * results[name][0] / K, results[name][1]))
    text.append("  A / P %.2f   B / A %.2f   B16 / A %.2f   worst |u_A - u_B| %.3g (max u = 1)"
                % (results["A"][0] / results["P"][0], results["B"][0] / results["A"][0], results["B16"][0] / results["A"][0], worst))
    print("\n".join(text))
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(text) + "\n")


if __name__ == "__main__":
    main()

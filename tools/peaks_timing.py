#!/usr/bin/env python3
"""Host loop against the device for the automatic peak picking: AutoPeakSelector(w, u, thresh, window).find_peaks()
spectrum after spectrum against nmrfit_amd.peaks.find_peaks_many, for 200 spectra of 4096 points, 50 of 65536 and a lone
spectrum of each size (synthetic, synth.make_spectrum, 6 and 24 peaks, thresh 0.1, window 0.02).

The host loop is timed on up to --host-spectra spectra of each shape and scaled to S (its cost is per spectrum); the
device call is timed whole (host preparation, copies and the Python objects included), wall clock, after a warm-up call,
median of --reps.  One JSON line per shape, then a table.

    python tools/peaks_timing.py [--reps 3] [--host-spectra 10] [--out profiles/peaks_timing.txt]
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nmrfit_amd import peaks, synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--host-spectra", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                  "profiles", "peaks_timing.txt"))
    a = ap.parse_args()
    rows = []
    for N, P, S in ((4096, 6, 1), (4096, 6, 200), (65536, 24, 1), (65536, 24, 50)):
        sps = [synth.make_spectrum(N, P, seed=100 + k) for k in range(S)]
        ws, us = [s["w"] for s in sps], [s["u"] for s in sps]
        h = min(S, a.host_spectra if N <= 4096 else max(1, a.host_spectra // 5))
        t0 = time.perf_counter()
        counts = []
        for w, u in zip(ws[:h], us[:h]):
            sel = peaks.AutoPeakSelector(w, u, 0.1, 0.02)
            sel.find_peaks()
            counts.append(len(sel.peaks))
        host_s = (time.perf_counter() - t0) / h * S
        peaks.find_peaks_many(ws, us, thresh=0.1, window=0.02)         # warm-up (library load, first launch)
        times = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            got = peaks.find_peaks_many(ws, us, thresh=0.1, window=0.02)
            times.append(time.perf_counter() - t0)
        dev_s = statistics.median(times)
        same = all(len(g) == c for g, c in zip(got[:h], counts))
        row = dict(S=S, N=N, P=P, host_s=host_s, host_spectra_timed=h, device_s=dev_s, device_min_s=min(times),
                   speedup=host_s / dev_s, same_counts_as_host=same)
        rows.append(row)
        print(json.dumps(row), flush=True)
    lines = ["%4s %6s %12s %12s %10s" % ("S", "N", "host (s)", "device (s)", "speed-up")]
    for r in rows:
        lines.append("%4d %6d %12.3f %12.5f %9.1fx" % (r["S"], r["N"], r["host_s"], r["device_s"], r["speedup"]))
    lines.append("(host: AutoPeakSelector.find_peaks per spectrum, timed on up to %d spectra per shape and scaled to S; "
                 "device: peaks.find_peaks_many, whole call, median of %d)" % (a.host_spectra, a.reps))
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(json.dumps(r) for r in rows) + "\n" + text + "\n")


if __name__ == "__main__":
    main()

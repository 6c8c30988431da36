#!/usr/bin/env python3
"""Host loop against the device for the automatic phase correction: Data.shift_phase(method) spectrum after spectrum
against nmrfit_amd.shift_phase_many(datas, method), for S in {1, 200} spectra of N in {4096, 65536} points (synthetic,
6 peaks, synth.make_spectrum(..., physical=True)), methods 'auto' (ACME + Nelder-Mead) and 'brute' (720 angles).

The host loop is timed on up to --host-spectra spectra of each shape and scaled to S (its cost is per spectrum); the
device call is timed whole, wall clock, after a warm-up call (median of --reps).  One JSON line per shape and method,
then a table.

    python tools/phase_timing.py [--reps 5] [--host-spectra 8] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nmrfit_amd import synth  # noqa: E402
from nmrfit_amd.containers import Data, shift_phase_many  # noqa: E402


def datas(S, N):
    out = []
    for k in range(S):
        sp = synth.make_spectrum(N, 6, seed=100 + k, physical=True)
        out.append(Data(sp["w"], sp["u"], sp["v"]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-spectra", type=int, default=8)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rows = []
    for N in (4096, 65536):
        for S in (1, 200):
            ds = datas(S, N)
            for method in ("auto", "brute"):
                h = min(S, a.host_spectra if N <= 4096 else max(1, a.host_spectra // 4))
                t0 = time.perf_counter()
                for d in ds[:h]:
                    d.shift_phase(method=method)
                host_s = (time.perf_counter() - t0) / h * S
                host_p = [(d.p0, d.p1) for d in ds[:h]]
                shift_phase_many(ds, method=method)          # warm-up (library load, first launch)
                times = []
                for _ in range(a.reps):
                    t0 = time.perf_counter()
                    shift_phase_many(ds, method=method)
                    times.append(time.perf_counter() - t0)
                dev_s = statistics.median(times)
                dp = max(abs(d.p0 - p[0]) + abs(d.p1 - p[1]) for d, p in zip(ds, host_p)) * 180 / np.pi
                row = dict(method=method, S=S, N=N, host_s=host_s, host_spectra_timed=h, device_s=dev_s,
                           device_min_s=min(times), speedup=host_s / dev_s, max_dp_deg_vs_host=dp)
                rows.append(row)
                print(json.dumps(row), flush=True)
    lines = ["%-6s %4s %6s %12s %12s %9s %12s" % ("method", "S", "N", "host (s)", "device (s)", "speed-up", "max |dp| deg")]
    for r in rows:
        lines.append("%-6s %4d %6d %12.4f %12.5f %8.1fx %12.2g" % (r["method"], r["S"], r["N"], r["host_s"], r["device_s"],
                                                                  r["speedup"], r["max_dp_deg_vs_host"]))
    lines.append("(host: Data.shift_phase per spectrum, timed on up to %d spectra per shape and scaled to S; device: "
                 "shift_phase_many, whole call incl. copies and the host ps2 of V, I, median of %d)" % (a.host_spectra, a.reps))
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(json.dumps(r) for r in rows) + "\n" + text + "\n")


if __name__ == "__main__":
    main()

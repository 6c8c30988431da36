#!/usr/bin/env python3
"""What least squares on both channels costs and is worth (include/nmrfit_amd_lsq_im.h; csrc/objective_rows_im.hip).

1. One nmrfit_jacobian_im (J, r of both channels; and A, g, f2 alone) against one nmrfit_jacobian at the C5 shape
   (P = 12, N = 16384), for both imaginary-channel modes: wall clock after a warm-up call, the forms alternating in the
   same process, best of --reps with every run shown.
2. nmrfit_amd.fit_many on --jobs default synthetic jobs (4096 x 6, 204 particles, pyswarm's stopping rule; physical
   spectra: the imaginary channel carries the dispersion lines) with fit_im=True and options['polish']:
   batch_polish="both" against the only path such jobs had before -- the per-fit scipy polish on the real channel, accepted
   or rejected against the fit_im objective -- alternating, best of --reps with every run shown; mean and worst final
   error of both, and of the same list without polish.

    python tools/lsq_im_timing.py [--reps 3] [--jobs 200] [--out profiles/lsq_im_timing.txt]
"""
import argparse
import contextlib
import io
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import nmrfit_amd  # noqa: E402
from nmrfit_amd import lsq, synth  # noqa: E402


def jac_rows(reps):
    from nmrfit_amd.equations import Evaluator
    sp = synth.make_spectrum(16384, 12, seed=5, physical=True)
    x = synth.make_swarm(sp["lower"], sp["upper"], 2, seed=6)[1]
    out = []
    with Evaluator(sp["w"], sp["u"], sp["v"], sp["weights"]) as ev:
        m = lsq.ResidualModel(ev, sp["lower"], sp["upper"])
        rows, h = m.rows(x)
        c, s = m._scale / h, m._scale
        forms = [("nmrfit_jacobian: J, r", lambda: ev.jacobian(rows, c, s, J=True, r=True)),
                 ("nmrfit_jacobian: A, g, f", lambda: ev.jacobian(rows, c, s, normal=True))]
        for mode, name in ((True, "fit_im=True"), ("sum", 'fit_im="sum"')):
            forms.append(("nmrfit_jacobian_im %s: J, r of both channels" % name,
                          lambda mode=mode: ev.jacobian_im(rows, c, s, mode, J=True, r=True)))
            forms.append(("nmrfit_jacobian_im %s: A, g, f2 of both channels" % name,
                          lambda mode=mode: ev.jacobian_im(rows, c, s, mode, normal=True)))
        for _, fn in forms:          # warm-up: buffers, staging memory
            fn()
        ts = {name: [] for name, _ in forms}
        for _ in range(max(reps, 5)):
            for name, fn in forms:   # alternating
                t0 = time.perf_counter()
                fn()
                ts[name].append(time.perf_counter() - t0)
        for name, _ in forms:
            out.append(dict(kind="jac", form=name, N=16384, P=12, ms=1e3 * min(ts[name]), runs_ms=[1e3 * t for t in ts[name]]))
            print(json.dumps(out[-1]), flush=True)
    return out


def fit_many_rows(reps, n):
    specs = [synth.make_spectrum(4096, 6, seed=100 + k % 8, physical=True) for k in range(8)]

    def jobs(extra):
        return [dict(data=synth.SynthData(specs[k % 8]["w"], specs[k % 8]["u"], specs[k % 8]["v"], specs[k % 8]["peaks"]),
                     lower=list(specs[k % 8]["lower"]), upper=list(specs[k % 8]["upper"]), fit_im=True,
                     options=dict(extra, seed=7 + k)) for k in range(n)]

    def run(extra, flag):
        with contextlib.redirect_stdout(io.StringIO()):
            t0 = time.perf_counter()
            fits = nmrfit_amd.fit_many(jobs(extra), batch_polish=flag)
            return time.perf_counter() - t0, fits
    paths = (("fit only", {}, False), ("per-fit polish (real channel)", {"polish": True}, False),
             ('batch_polish="both"', {"polish": True}, "both"))
    run({"polish": True, "maxiter": 20}, "both")             # warm-up
    times = {name: [] for name, _, _ in paths}
    err = {}
    for _ in range(reps):
        for name, extra, flag in paths:                      # alternating
            t, fits = run(extra, flag)
            times[name].append(t)
            err[name] = np.array([f.error for f in fits])
    rows = []
    for name, ts in times.items():
        rows.append(dict(kind="fit_many", jobs=n, fit_im=True, path=name, fits_per_s=n / min(ts), runs_s=ts,
                         mean_error=float(err[name].mean()), worst_error=float(err[name].max()),
                         worse_than_swarm=int(np.sum(err[name] > err["fit only"])),
                         above_per_fit=int(np.sum(err[name] > err["per-fit polish (real channel)"]))))
        print(json.dumps(rows[-1]), flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--jobs", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lsq_im_timing.txt"))
    a = ap.parse_args()
    jr = jac_rows(a.reps)
    fr = fit_many_rows(a.reps, a.jobs)
    lines = ["one Jacobian at P = 12, N = 16384 (wall clock, alternating, best of %d; every run in ms):" % max(a.reps, 5)]
    for r in jr:
        lines.append("  %-62s %8.3f ms   [%s]" % (r["form"], r["ms"], " ".join("%.3f" % t for t in r["runs_ms"])))
    lines.append("fit_many, %d default synthetic fit_im=True jobs (4096 x 6, 204 particles, pyswarm's rule), alternating, best of %d "
                 "(every run in s):" % (a.jobs, a.reps))
    for r in fr:
        lines.append("  %-30s %8.1f fits/s  [%s]   mean error %.9g   worst %.9g   fits above the swarm's error: %d   above the "
                     "per-fit polish's: %d" % (r["path"], r["fits_per_s"], " ".join("%.2f" % t for t in r["runs_s"]), r["mean_error"],
                                               r["worst_error"], r["worse_than_swarm"], r["above_per_fit"]))
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(json.dumps(r) for r in jr + fr) + "\n" + text + "\n")


if __name__ == "__main__":
    main()

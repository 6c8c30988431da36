#!/usr/bin/env python3
"""What the first-order standard errors cost (include/nmrfit_amd_cov.h; csrc/lsq_cov.hip), on --jobs default synthetic jobs
(4096 x 6, 204 particles, pyswarm's stopping rule; physical spectra).  Wall clock after a warm-up, the forms alternating
in ONE process, best of --reps with every run kept.

1. nmrfit_batch_sandwich (A, M, g, f) against nmrfit_batch_normal_equations (A, g, f: the call the polish makes) on one
   resident batch of the jobs at their generating parameters: what the meat adds to a launch of the residual rows.
2. nmrfit_amd.fit_many(batch_polish=True) with options['polish'], without and with uncertainty=dict(sigma=...), in fits/s.
3. The same jobs through nmrfit_amd.fit_replicas_many(replicas=32) with options['polish']: the path the option replaces
   for a first-order answer (33 fits per job).

    python tools/uncertainty_timing.py [--reps 5] [--jobs 200] [--out profiles/uncertainty_timing.txt]
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
from nmrfit_amd import synth  # noqa: E402
from nmrfit_amd.batch import FitBatch  # noqa: E402


def specs8():
    return [synth.make_spectrum(4096, 6, seed=100 + k, physical=True) for k in range(8)]


def alternate(forms, reps):
    for _, fn in forms:          # warm-up: buffers, staging memory, a thread's first HIP call
        fn()
    ts = {name: [] for name, _ in forms}
    for _ in range(reps):
        for name, fn in forms:   # alternating
            t0 = time.perf_counter()
            fn()
            ts[name].append(time.perf_counter() - t0)
    return ts


def call_rows(reps, n):
    specs = specs8()
    pick = [specs[k % 8] for k in range(n)]
    X = [sp["x_true"] for sp in pick]
    su = [1e-3 * float(np.max(np.abs(sp["u"]))) for sp in pick]
    with FitBatch([(sp["w"], sp["u"], sp["v"], sp["weights"]) for sp in pick], [sp["lower"] for sp in pick],
                  [sp["upper"] for sp in pick], seeds=list(range(n))) as fb:
        forms = [("nmrfit_batch_normal_equations: A, g, f", lambda: fb.normal_equations(X)),
                 ("nmrfit_batch_sandwich: A, M, g, f", lambda: fb.sandwich(X, su, su)),
                 ("FitBatch.uncertainty: + the D x D algebra on the host", lambda: fb.uncertainty(X, su, su))]
        ts = alternate(forms, reps)
    out = []
    for name, _ in forms:
        out.append(dict(kind="call", form=name, jobs=n, N=4096, P=6, ms=1e3 * min(ts[name]), runs_ms=[1e3 * t for t in ts[name]]))
        print(json.dumps(out[-1]), flush=True)
    return out


def fit_rows(reps, n, replicas):
    specs = specs8()
    sig = [1e-3 * float(np.max(np.abs(sp["u"]))) for sp in specs]

    def jobs():
        return [dict(data=synth.SynthData(specs[k % 8]["w"], specs[k % 8]["u"], specs[k % 8]["v"], specs[k % 8]["peaks"]),
                     lower=list(specs[k % 8]["lower"]), upper=list(specs[k % 8]["upper"]), sigma=sig[k % 8],
                     options=dict(polish=True, seed=7 + k)) for k in range(n)]

    def quiet(fn):
        def run():
            with contextlib.redirect_stdout(io.StringIO()):
                return fn()
        return run
    forms = [("fit_many(batch_polish=True)", quiet(lambda: nmrfit_amd.fit_many(jobs(), batch_polish=True))),
             ("fit_many(batch_polish=True, uncertainty=...)",
              quiet(lambda: nmrfit_amd.fit_many(jobs(), batch_polish=True, uncertainty={}))),
             ("fit_replicas_many(replicas=%d), polish" % replicas,
              quiet(lambda: nmrfit_amd.fit_replicas_many(jobs(), replicas=replicas, options=dict(polish=True))))]
    ts = alternate(forms, reps)
    out = []
    for name, _ in forms:
        out.append(dict(kind="fit", path=name, jobs=n, spectra_per_s=n / min(ts[name]), runs_s=ts[name]))
        print(json.dumps(out[-1]), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--jobs", type=int, default=200)
    ap.add_argument("--replicas", type=int, default=32)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "uncertainty_timing.txt"))
    a = ap.parse_args()
    cr = call_rows(a.reps, a.jobs)
    fr = fit_rows(a.reps, a.jobs, a.replicas)
    lines = ["one call on a resident batch of %d default jobs (4096 x 6) at their generating parameters (wall clock, alternating, "
             "best of %d; every run in ms):" % (a.jobs, a.reps)]
    for r in cr:
        lines.append("  %-58s %8.3f ms   [%s]" % (r["form"], r["ms"], " ".join("%.3f" % t for t in r["runs_ms"])))
    lines.append("  the meat adds %.3f ms (%.1f %%) to the normal-equations call" % (cr[1]["ms"] - cr[0]["ms"],
                                                                                  100.0 * (cr[1]["ms"] / cr[0]["ms"] - 1.0)))
    lines.append("%d default jobs with options['polish'] (204 particles, pyswarm's rule), alternating, best of %d (every run in s):"
                 % (a.jobs, a.reps))
    for r in fr:
        lines.append("  %-48s %8.1f spectra/s  [%s]" % (r["path"], r["spectra_per_s"], " ".join("%.2f" % t for t in r["runs_s"])))
    lines.append("  uncertainty= costs %.1f %% of fit_many's rate; the replica study runs at 1 / %.1f of it"
                 % (100.0 * (1.0 - fr[1]["spectra_per_s"] / fr[0]["spectra_per_s"]), fr[1]["spectra_per_s"] / fr[2]["spectra_per_s"]))
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(json.dumps(r) for r in cr + fr) + "\n" + text + "\n")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""What the analytic Jacobian costs and is worth (csrc/lsq_analytic.hip; include/nmrfit_amd_lsq_analytic.h).

1. A, g, f of one fit at P = 12, N = 16384 and at P = 24, N = 65536: the forward-difference path (nmrfit_jacobian: D + 1
   residual rows, then the sums) against the analytic one (nmrfit_jacobian_analytic: one pass), wall clock after a warm-up
   call, alternating in one process, best of max(--reps, 5); every run kept.
2. nmrfit_amd.fit_many on 200 default synthetic jobs (4096 x 6, 204 particles, pyswarm's stopping rule) with
   options['polish'] and batch_polish=True, polish_jac "2-point" against "analytic": fits/s, the mean and the worst final
   error; alternating, best of --reps.
--cpu: no GPU -- the largest relative gap of the final objective between lsq.lm_polish over lsq.analytic_provider and over
   lsq.rows_provider on the host residual (lsq.jacobian_host), over the cases of tests/lsq_support.py: what
   tests/lsq_analytic_support.MEASURED_GAP records.

    python tools/lsq_analytic_timing.py [--cpu] [--reps 3] [--jobs 200] [--out profiles/lsq_analytic_timing.txt]
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


def gap_rows():
    from tests import lsq_analytic_support as A
    from tests import lsq_support as S
    rows = []
    for case in S.polish_cases():
        gap, fa, fr, f0 = A.polish_gap(case)
        rows.append(dict(kind="gap", P=(len(case[1]) - 4) // 3, N=len(case[0]["w"]), start_f=f0, analytic_f=fa, rows_f=fr,
                         relative_gap=float(gap)))
        print(json.dumps(rows[-1]), flush=True)
    return rows


def normal_rows(reps):
    from nmrfit_amd.equations import Evaluator
    out = []
    for N, P in ((16384, 12), (65536, 24)):
        sp = synth.make_spectrum(N, P, seed=5)
        x = synth.make_swarm(sp["lower"], sp["upper"], 2, seed=6)[1]
        with Evaluator(sp["w"], sp["u"], sp["v"], sp["weights"]) as ev:
            forms = (("2-point", lsq.ResidualModel(ev, sp["lower"], sp["upper"])),
                     ("analytic", lsq.ResidualModel(ev, sp["lower"], sp["upper"], jac="analytic")))
            got = {name: m.normal_equations(x) for name, m in forms}     # warm-up
            ts = {name: [] for name, _ in forms}
            for _ in range(max(reps, 5)):
                for name, m in forms:
                    t0 = time.perf_counter()
                    m.normal_equations(x)
                    ts[name].append(time.perf_counter() - t0)
            A2, g2, f2 = got["2-point"]
            Aa, ga, fa = got["analytic"]
            for name, _ in forms:
                out.append(dict(kind="normal", form=name, N=N, P=P, ms=1e3 * min(ts[name]), runs_ms=[1e3 * t for t in ts[name]],
                                f=float(got[name][2]), g_rel_to_analytic=float(np.linalg.norm(got[name][1] - ga) / np.linalg.norm(ga)),
                                A_rel_to_analytic=float(np.linalg.norm(got[name][0] - Aa) / np.linalg.norm(Aa))))
                print(json.dumps(out[-1]), flush=True)
    return out


def fit_many_rows(reps, n):
    specs = [synth.make_spectrum(4096, 6, seed=100 + k % 8) for k in range(8)]

    def jobs(extra):
        return [dict(data=synth.SynthData(specs[k % 8]["w"], specs[k % 8]["u"], specs[k % 8]["v"], specs[k % 8]["peaks"]),
                     lower=list(specs[k % 8]["lower"]), upper=list(specs[k % 8]["upper"]), options=dict(extra, seed=7 + k))
                for k in range(n)]

    def run(extra, jac):
        with contextlib.redirect_stdout(io.StringIO()):
            t0 = time.perf_counter()
            fits = nmrfit_amd.fit_many(jobs(extra), batch_polish=True, polish_jac=jac)
            return time.perf_counter() - t0, fits
    for jac in ("2-point", "analytic"):
        run({"polish": True, "maxiter": 20}, jac)          # warm-up
    paths = (("fit only", {}, "2-point"), ("batch polish, 2-point", {"polish": True}, "2-point"),
             ("batch polish, analytic", {"polish": True}, "analytic"))
    times = {name: [] for name, _, _ in paths}
    err = {}
    for _ in range(reps):
        for name, extra, jac in paths:
            t, fits = run(extra, jac)
            times[name].append(t)
            err[name] = np.array([f.error for f in fits])
    rows = []
    for name, ts in times.items():
        rows.append(dict(kind="fit_many", jobs=n, path=name, fits_per_s=n / min(ts), runs_s=ts, mean_error=float(err[name].mean()),
                         worst_error=float(err[name].max()), worse_than_swarm=int(np.sum(err[name] > err["fit only"]))))
        print(json.dumps(rows[-1]), flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cpu", action="store_true")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--jobs", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lsq_analytic_timing.txt"))
    a = ap.parse_args()
    rows = gap_rows()
    lines = ["lm_polish over analytic normal equations against the same loop over forward differences (host residual, 100 D "
             "launches), N = 1024:"]
    for r in rows:
        lines.append("  P = %d  start %.9g  analytic %.17g  forward differences %.17g  relative gap %.3g"
                     % (r["P"], r["start_f"], r["analytic_f"], r["rows_f"], r["relative_gap"]))
    lines.append("  largest relative gap %.3g" % max(r["relative_gap"] for r in rows))
    if not a.cpu:
        nr = normal_rows(a.reps)
        fr = fit_many_rows(a.reps, a.jobs)
        rows += nr + fr
        lines.append("A, g, f of one fit (wall clock per call, best of %d, alternating):" % max(a.reps, 5))
        for r in nr:
            lines.append("  P = %2d  N = %5d  %-9s %9.3f ms   f %.17g   |g - g_analytic| / |g_analytic| %.3g" % (
                r["P"], r["N"], r["form"], r["ms"], r["f"], r["g_rel_to_analytic"]))
        lines.append("fit_many, %d default synthetic jobs (4096 x 6, 204 particles, pyswarm's rule), best of %d:" % (a.jobs, a.reps))
        for r in fr:
            lines.append("  %-24s %8.1f fits/s   mean error %.9g   worst error %.9g   fits above the swarm's error: %d"
                         % (r["path"], r["fits_per_s"], r["mean_error"], r["worst_error"], r["worse_than_swarm"]))
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(json.dumps(r) for r in rows) + "\n" + text + "\n")


if __name__ == "__main__":
    main()

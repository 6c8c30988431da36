#!/usr/bin/env python3
"""What the device-side least-squares pieces cost and are worth (csrc/lsq.hip, lsq.lm_polish).

1. One ResidualModel.jac() at the C5 shape (P = 12, N = 16384; wall clock after a warm-up call, best of --reps): the
   parent commit's form -- nmrfit_residual_batch to pageable memory, subtract and transpose on the host -- against this
   commit's nmrfit_jacobian, and the normal equations alone (D^2 + D doubles back instead of N D).
2. nmrfit_amd.fit_many on 200 default synthetic jobs (4096 x 6, 204 particles, pyswarm's stopping rule) with
   options['polish']: the per-fit scipy path against batch_polish=True; same process, alternating, best of --reps.
3. The same list without polish: the fit-only rate both are to be read against.
--cpu: no GPU -- the largest relative gap between lm_polish's and scipy TRF's final objective over the cases of
   tests/lsq_support.py, both on the C restatement of the residual (what tests/lsq_support.MEASURED_GAP records).

    python tools/lsq_timing.py [--cpu] [--reps 3] [--jobs 200] [--out profiles/lsq_timing.txt]
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
    from oracle import c_oracle
    from tests import lsq_support as S
    rows = []
    for sp, x0 in S.polish_cases():
        def res(r, sp=sp):
            return c_oracle.residual_batch(r, *S.spectrum_tuple(sp))
        D = len(x0)
        X, f, info = lsq.lm_polish(lsq.rows_provider([res], [sp["lower"]], [sp["upper"]]), [x0], [sp["lower"]], [sp["upper"]],
                                   max_launches=100 * D)
        _, ft = S.trf_on_rows(res, x0, sp["lower"], sp["upper"])
        rows.append(dict(kind="gap", P=(D - 4) // 3, N=len(sp["w"]), lm_f=float(f[0]), trf_f=ft, launches=info["launches"],
                         stop=info["stop"][0], relative_gap=abs(float(f[0]) - ft) / ft))
        print(json.dumps(rows[-1]), flush=True)
    return rows


def jac_rows(reps):
    from nmrfit_amd.equations import Evaluator
    sp = synth.make_spectrum(16384, 12, seed=5)
    x = synth.make_swarm(sp["lower"], sp["upper"], 2, seed=6)[1]
    with Evaluator(sp["w"], sp["u"], sp["v"], sp["weights"]) as ev:
        m = lsq.ResidualModel(ev, sp["lower"], sp["upper"])

        def parent():
            rows, h = m.rows(x)
            R = ev.residual_batch(rows)
            return np.ascontiguousarray(((R[1:] - R[0]) * (m._scale / h[:, None])).T)
        forms = (("parent: rows to the host, subtract, transpose", parent), ("nmrfit_jacobian: J", lambda: m.jac(x)),
                 ("nmrfit_jacobian: A, g, f", lambda: m.normal_equations(x)))
        same = np.array_equal(parent(), m.jac(x))
        m.normal_equations(x)
        out = []
        for name, fn in forms:
            ts = []
            for _ in range(max(reps, 5)):
                t0 = time.perf_counter()
                fn()
                ts.append(time.perf_counter() - t0)
            out.append(dict(kind="jac", form=name, N=16384, P=12, ms=1e3 * min(ts), runs_ms=[1e3 * t for t in ts], J_bits_equal=same))
            print(json.dumps(out[-1]), flush=True)
    return out


def fit_many_rows(reps, n):
    specs = [synth.make_spectrum(4096, 6, seed=100 + k % 8) for k in range(8)]

    def jobs(extra):
        return [dict(data=synth.SynthData(specs[k % 8]["w"], specs[k % 8]["u"], specs[k % 8]["v"], specs[k % 8]["peaks"]),
                     lower=list(specs[k % 8]["lower"]), upper=list(specs[k % 8]["upper"]), options=dict(extra, seed=7 + k))
                for k in range(n)]

    def run(extra, flag):
        with contextlib.redirect_stdout(io.StringIO()):
            t0 = time.perf_counter()
            fits = nmrfit_amd.fit_many(jobs(extra), batch_polish=flag)
            return time.perf_counter() - t0, fits
    for flag in (False, True):
        run({"polish": True, "maxiter": 20}, flag)          # warm-up
    times = {"fit only": [], "per-fit polish": [], "batch polish": []}
    err = {}
    for _ in range(reps):
        for name, extra, flag in (("fit only", {}, False), ("per-fit polish", {"polish": True}, False),
                                  ("batch polish", {"polish": True}, True)):
            t, fits = run(extra, flag)
            times[name].append(t)
            err[name] = np.array([f.error for f in fits])
    rows = []
    for name, ts in times.items():
        rows.append(dict(kind="fit_many", jobs=n, path=name, fits_per_s=n / min(ts), runs_s=ts,
                         mean_error=float(err[name].mean()),
                         worse_than_swarm=int(np.sum(err[name] > err["fit only"])),
                         max_rel_above_per_fit=float(np.max((err[name] - err["per-fit polish"]) / err["per-fit polish"]))))
        print(json.dumps(rows[-1]), flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cpu", action="store_true")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--jobs", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lsq_timing.txt"))
    a = ap.parse_args()
    rows = gap_rows()
    lines = ["lm_polish against scipy TRF (both at tolerance 1e-12, 100 D evaluations) on the C restatement, N = 1024:"]
    for r in rows:
        lines.append("  P = %d  lm %.17g (%d launches, %s)  trf %.17g  relative gap %.3g" % (r["P"], r["lm_f"], r["launches"], r["stop"],
                                                                                          r["trf_f"], r["relative_gap"]))
    lines.append("  largest relative gap %.3g" % max(r["relative_gap"] for r in rows))
    if not a.cpu:
        jr = jac_rows(a.reps)
        fr = fit_many_rows(a.reps, a.jobs)
        rows += jr + fr
        lines.append("one Jacobian at P = 12, N = 16384 (wall clock, best of %d; J bits equal: %s):" % (max(a.reps, 5), jr[0]["J_bits_equal"]))
        for r in jr:
            lines.append("  %-48s %8.3f ms" % (r["form"], r["ms"]))
        lines.append("fit_many, %d default synthetic jobs (4096 x 6, 204 particles, pyswarm's rule), best of %d:" % (a.jobs, a.reps))
        for r in fr:
            lines.append("  %-16s %8.1f fits/s   mean error %.9g   fits above the swarm's error: %d   max relative excess over "
                         "the per-fit polish: %.2e" % (r["path"], r["fits_per_s"], r["mean_error"], r["worse_than_swarm"],
                                                       r["max_rel_above_per_fit"]))
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(json.dumps(r) for r in rows) + "\n" + text + "\n")


if __name__ == "__main__":
    main()

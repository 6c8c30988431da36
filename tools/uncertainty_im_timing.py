#!/usr/bin/env python3
"""What the first-order standard errors of fit_im fits cost (include/nmrfit_amd_cov_im.h; csrc/lsq_cov_im.hip), on --jobs
default synthetic fit_im="sum" jobs (4096 x 6, 204 particles, pyswarm's stopping rule; physical spectra).  Wall clock after
a warm-up, the forms alternating in ONE process, best of --reps with every run kept.

1. nmrfit_batch_sandwich_im (A, g, rho per channel and the three blocks) against nmrfit_batch_normal_equations_im (A, g,
   rho: the call the polish on both channels makes) on one resident batch of the jobs at their generating parameters: what
   the two-channel meat adds to a launch of the residual rows -- and FitBatch.uncertainty(channels="both"), which adds
   uncertainty.covariance_im's numpy on the host.
2. nmrfit_amd.fit_many(batch_polish="both") with options['polish'], without and with
   uncertainty=dict(..., channels="both"), in fits/s.
3. The replica comparison: one spectrum's --replicas noisy copies (made on the device) refitted as one batch by
   FitBatch.polish(channels="both") from the base's parameters -- the cheapest replica study there is, no swarm -- scaled
   per spectrum.

    python tools/uncertainty_im_timing.py [--reps 5] [--jobs 200] [--out profiles/uncertainty_im_timing.txt]
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
from nmrfit_amd import noise, synth  # noqa: E402
from nmrfit_amd.batch import FitBatch  # noqa: E402
from tools.uncertainty_timing import alternate, specs8  # noqa: E402


def batch(specs, **kw):
    return FitBatch([(sp["w"], sp["u"], sp["v"], sp["weights"]) for sp in specs], [sp["lower"] for sp in specs],
                    [sp["upper"] for sp in specs], fit_im="sum", **kw)


def call_rows(reps, n):
    specs = specs8()
    pick = [specs[k % 8] for k in range(n)]
    X = [sp["x_true"] for sp in pick]
    su = [1e-3 * float(np.max(np.abs(sp["u"]))) for sp in pick]
    sv = [2.0 * s for s in su]
    with batch(pick, seeds=list(range(n))) as fb:
        forms = [("nmrfit_batch_normal_equations_im: A, g, rho", lambda: fb.normal_equations(X, channels="both")),
                 ("nmrfit_batch_sandwich_im: A, g, rho, Mt_rr, Mt_ii, Mt_ri", lambda: fb.sandwich_im(X, su, sv)),
                 ("FitBatch.uncertainty(channels='both'): + the algebra on the host", lambda: fb.uncertainty(X, su, sv, channels="both"))]
        ts = alternate(forms, reps)
    out = []
    for name, _ in forms:
        out.append(dict(kind="call", form=name, jobs=n, N=4096, P=6, ms=1e3 * min(ts[name]), runs_ms=[1e3 * t for t in ts[name]]))
        print(json.dumps(out[-1]), flush=True)
    return out


def quiet(fn):
    def run():
        with contextlib.redirect_stdout(io.StringIO()):
            return fn()
    return run


def fit_rows(reps, n):
    specs = specs8()
    sig = [1e-3 * float(np.max(np.abs(sp["u"]))) for sp in specs]

    def jobs():
        return [dict(data=synth.SynthData(specs[k % 8]["w"], specs[k % 8]["u"], specs[k % 8]["v"], specs[k % 8]["peaks"]),
                     lower=list(specs[k % 8]["lower"]), upper=list(specs[k % 8]["upper"]), sigma=(sig[k % 8], 2.0 * sig[k % 8]),
                     fit_im="sum", options=dict(polish=True, seed=7 + k)) for k in range(n)]
    forms = [("fit_many(batch_polish='both')", quiet(lambda: nmrfit_amd.fit_many(jobs(), batch_polish="both"))),
             ("fit_many(batch_polish='both', uncertainty=dict(channels='both'))",
              quiet(lambda: nmrfit_amd.fit_many(jobs(), batch_polish="both", uncertainty=dict(channels="both"))))]
    ts = alternate(forms, reps)
    out = []
    for name, _ in forms:
        out.append(dict(kind="fit", path=name, jobs=n, spectra_per_s=n / min(ts[name]), runs_s=ts[name]))
        print(json.dumps(out[-1]), flush=True)
    return out


def replica_rows(reps, replicas):
    sp = specs8()[0]
    su = 1e-3 * float(np.max(np.abs(sp["u"])))

    def study():
        uv = noise.replicas([sp["u"]] * replicas, [sp["v"]] * replicas, su, 2.0 * su, list(range(1000, 1000 + replicas)))
        with batch([dict(sp, u=u, v=v) for u, v in uv], swarmsize=8, seeds=list(range(replicas))) as fb:
            fb.run(1, 1)      # (polish reads best() first; nothing of the generation is used)
            return fb.polish([sp["x_true"]] * replicas, channels="both", max_launches=100)
    ts = alternate([("study", study)], reps)["study"]
    row = dict(kind="replicas", path="%d replicas of one spectrum, FitBatch.polish(channels='both'), no swarm" % replicas,
               replicas=replicas, s_per_spectrum=min(ts), runs_s=ts)
    print(json.dumps(row), flush=True)
    return [row]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--jobs", type=int, default=200)
    ap.add_argument("--replicas", type=int, default=63)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "uncertainty_im_timing.txt"))
    a = ap.parse_args()
    cr = call_rows(a.reps, a.jobs)
    fr = fit_rows(a.reps, a.jobs)
    rr = replica_rows(a.reps, a.replicas)
    lines = ["one call on a resident batch of %d default fit_im='sum' jobs (4096 x 6) at their generating parameters (wall clock, "
             "alternating, best of %d; every run in ms):" % (a.jobs, a.reps)]
    for r in cr:
        lines.append("  %-66s %8.3f ms   [%s]" % (r["form"], r["ms"], " ".join("%.3f" % t for t in r["runs_ms"])))
    lines.append("  the two-channel meat adds %.3f ms (ratio %.2f) to the normal-equations call; the host algebra %.3f ms (%.3f ms per fit)"
                 % (cr[1]["ms"] - cr[0]["ms"], cr[1]["ms"] / cr[0]["ms"], cr[2]["ms"] - cr[1]["ms"], (cr[2]["ms"] - cr[1]["ms"]) / a.jobs))
    lines.append("%d default fit_im='sum' jobs with options['polish'] (204 particles, pyswarm's rule), alternating, best of %d "
                 "(every run in s):" % (a.jobs, a.reps))
    for r in fr:
        lines.append("  %-66s %8.1f spectra/s  [%s]" % (r["path"], r["spectra_per_s"], " ".join("%.2f" % t for t in r["runs_s"])))
    per_fit = 1.0 / fr[1]["spectra_per_s"] - 1.0 / fr[0]["spectra_per_s"]
    lines.append("  uncertainty= runs at %.2f of fit_many's rate: %.3f ms per spectrum" % (fr[1]["spectra_per_s"] / fr[0]["spectra_per_s"], 1e3 * per_fit))
    r = rr[0]
    lines.append("replica comparison, best of %d (every run in s):" % a.reps)
    lines.append("  %-66s %8.1f ms per spectrum  [%s]" % (r["path"], 1e3 * r["s_per_spectrum"], " ".join("%.3f" % t for t in r["runs_s"])))
    lines.append("  the replica polish alone costs %.0f times what uncertainty= adds per spectrum" % (r["s_per_spectrum"] / per_fit))
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(json.dumps(r) for r in cr + fr + rr) + "\n" + text + "\n")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""What making the noise replicas on the device is worth to a replica study.

200 replicas of a default synthetic spectrum (4096 points, 6 peaks, 204 particles), with pyswarm's stopping rule and
with all 2000 generations (minstep = minfunc = -1):

  A  nmrfit_amd.fit_replicas: the spectrum tiled into FitBatches, the copies made in place on the device
     (FitBatch.add_noise, csrc/noise.hip)
  B  the same batches, the same plan and seeds, built from host-made copies: np.tile + Generator.standard_normal, then a
     plain FitBatch (other deviates: the fits differ, the work does not)

Same process, alternating, wall clock around whole calls (each ends in a device synchronise), after a warm-up of both
sides; best of --reps and the spread (max - min) / min of each side's own runs.  Also the synchronous
FitBatch.add_noise call alone on a resident 200-fit batch (the job table's upload, the launch, the synchronise), and
noise.replicas (whole call with the copies both ways) against the host's tile + standard_normal for the same 200 copies.

    python tools/replicas_ab.py [--reps 3] [--replicas 200] [--out profiles/r07/replicas_ab.txt]

The noise kernel's own time is not a wall clock's to give: --kernel-only makes the resident 200-fit batches and calls
add_noise on each and nothing else, for a run of its own under the profiler,

    rocprofv3 --kernel-trace --stats -d DIR -- python tools/replicas_ab.py --kernel-only

whose kernel statistics hold the line of noise_kernel<true>.
"""
import argparse
import contextlib
import io
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import nmrfit_amd  # noqa: E402
from nmrfit_amd import core, noise, synth, utils  # noqa: E402
from nmrfit_amd.batch import FitBatch  # noqa: E402


def host_side(data, lower, upper, replicas, sigma, seed, options, rng):
    """Side B: fit_replicas's steps with the copies made on the host."""
    base = utils.FitUtility(data, lower, upper, summary=False, options=options)
    plan = base._plan()
    key = base._batch_key(plan)
    kw = {name: [plan["kw"][name]] * replicas for name in ("omega", "phip", "phig", "minstep", "minfunc")}
    u = np.tile(data.u, (replicas, 1)) + sigma * rng.standard_normal((replicas, len(data.u)))
    v = np.tile(data.v, (replicas, 1)) + sigma * rng.standard_normal((replicas, len(data.v)))
    out = []
    for a in range(0, replicas, core.BATCH_JOBS_MAX):
        ks = range(a, min(a + core.BATCH_JOBS_MAX, replicas))
        with FitBatch([(data.w, u[k], v[k], base.weights) for k in ks], [lower] * len(ks), [upper] * len(ks),
                      swarmsize=[int(plan["swarmsize"])] * len(ks), seeds=[seed + 1 + k for k in ks], variant=key.variant,
                      fit_im=key.fit_im, device=key.device, **{n: x[:len(ks)] for n, x in kw.items()}) as fb:
            fb.run(key.maxiter, key.check_every)
            fb.status()
            out += fb.best()
    return out


def area_fraction(x):
    """FitUtility.calculate_area_fraction of a parameter vector."""
    areas = np.asarray(x)[6::3]
    sats = areas[areas < areas.mean()].sum()
    return sats / areas.sum()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--replicas", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                  "profiles", "r07", "replicas_ab.txt"))
    ap.add_argument("--kernel-only", action="store_true", help="only add_noise on resident batches (for rocprofv3)")
    a = ap.parse_args()
    R = a.replicas
    spec = synth.make_spectrum(4096, 6, seed=1)
    data = synth.SynthData(spec["w"], spec["u"], spec["v"], spec["peaks"])
    lower, upper, sigma = list(spec["lower"]), list(spec["upper"]), float(spec["sigma"])
    rng = np.random.default_rng(5)
    rows = []
    if a.kernel_only:
        n = min(R, core.BATCH_JOBS_MAX)
        for _ in range(5):
            with FitBatch([(data.w, data.u, data.v, spec["weights"])] * n, [lower] * n, [upper] * n, seeds=list(range(n))) as fb:
                fb.add_noise(sigma, sigma, list(range(n)))
        return

    def side_a(options):
        return nmrfit_amd.fit_replicas(data, lower, upper, replicas=R, sigma=sigma, seed=7, include_original=False,
                                       options=options)

    for rule, options in (("pyswarm", {}), ("all 2000", {"minstep": -1.0, "minfunc": -1.0})):
        with contextlib.redirect_stdout(io.StringIO()):
            side_a(dict(options, maxiter=20))                                           # warm-up of both sides
            host_side(data, lower, upper, R, sigma, 7, dict(options, maxiter=20), rng)
        ta, tb = [], []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            rf = side_a(options)
            ta.append(time.perf_counter() - t0)
            t0 = time.perf_counter()
            hb = host_side(data, lower, upper, R, sigma, 7, options, rng)
            tb.append(time.perf_counter() - t0)
        rows.append(dict(kind="ab", rule=rule, replicas=R, device_runs_s=ta, host_runs_s=tb, device_s=min(ta), host_s=min(tb),
                         device_fits_per_s=R / min(ta), host_fits_per_s=R / min(tb), ratio=min(tb) / min(ta),
                         device_spread=(max(ta) - min(ta)) / min(ta), host_spread=(max(tb) - min(tb)) / min(tb),
                         area_fraction_std=rf.area_fraction_std,
                         host_area_fraction_std=float(np.std([area_fraction(x) for x, _ in hb], ddof=1))))
        print(json.dumps(rows[-1]), flush=True)

    # the in-place call alone, and the copies alone
    n = min(R, core.BATCH_JOBS_MAX)
    calls = []
    for _ in range(max(a.reps, 3)):
        with FitBatch([(data.w, data.u, data.v, spec["weights"])] * n, [lower] * n, [upper] * n, seeds=list(range(n))) as fb:
            fb.synchronize()
            t0 = time.perf_counter()
            fb.add_noise(sigma, sigma, list(range(n)))
            calls.append(time.perf_counter() - t0)
    us, vs = [data.u] * R, [data.v] * R
    noise.replicas(us[:2], vs[:2], sigma, sigma, [1, 2])
    td, th = [], []
    for _ in range(max(a.reps, 3)):
        t0 = time.perf_counter()
        noise.replicas(us, vs, sigma, sigma, list(range(R)))
        td.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        np.tile(data.u, (R, 1)) + sigma * rng.standard_normal((R, len(data.u)))
        np.tile(data.v, (R, 1)) + sigma * rng.standard_normal((R, len(data.v)))
        th.append(time.perf_counter() - t0)
    rows.append(dict(kind="copies", fits=n, add_noise_call_s=min(calls), add_noise_runs_s=calls, replicas=R,
                     replicas_call_s=min(td), host_tile_normal_s=min(th)))
    print(json.dumps(rows[-1]), flush=True)

    lines = ["%-9s %9s %13s %13s %11s %11s %7s %8s %8s" % ("rule", "replicas", "A device s", "B host s", "A fits/s", "B fits/s",
                                                            "B / A", "A spread", "B spread")]
    for r in rows:
        if r["kind"] == "ab":
            lines.append("%-9s %9d %13.4f %13.4f %11.1f %11.1f %7.3f %7.1f%% %7.1f%%" % (
                r["rule"], r["replicas"], r["device_s"], r["host_s"], r["device_fits_per_s"], r["host_fits_per_s"], r["ratio"],
                100 * r["device_spread"], 100 * r["host_spread"]))
    c = rows[-1]
    lines.append("(A: fit_replicas, copies made in place on the device; B: the same batches from np.tile + standard_normal; "
                 "4096 x 6, 204 particles; alternating, best of %d; B / A > 1: the device path is faster)" % a.reps)
    lines.append("FitBatch.add_noise on a resident batch of %d fits (upload of the job table, launch, synchronise): %.1f us"
                 % (c["fits"], 1e6 * c["add_noise_call_s"]))
    lines.append("%d copies alone: noise.replicas (whole call, copies both ways) %.2f ms; host tile + standard_normal %.2f ms"
                 % (c["replicas"], 1e3 * c["replicas_call_s"], 1e3 * c["host_tile_normal_s"]))
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(json.dumps(r) for r in rows) + "\n" + text + "\n")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Recorded outputs of tests/test_gpu_lsq_parent_bits.py: the least-squares sums of the device -- J, r, A, g of the normal
equations, the meat of the sandwich on the real channel and on both -- on the smallest shapes that reach each path of their
kernels, evaluated by ONE build of the library and kept bit for bit.

    tools/build_at.sh <commit>
    NMRFIT_LIB=nmrfit_amd/lib/libab_<commit>.so python tools/record_lsq_bits.py --commit <commit>

writes tests/golden/lsq_parent_bits.npz (needs a GPU; the commit's full hash goes into the file).  The test loads this
module for `run_cases` and compares what the working tree's library returns with np.array_equal.

The file holds data only: the seeds of the inputs, a SHA-256 of every regenerated input (so that a machine whose numpy
makes other inputs is told apart from a library that computes other sums), and the outputs -- an array above 32 KiB as the
SHA-256 of its bytes.  The inputs are `synth.make_spectrum(N, P, seed=SPEC_SEED + P, noise=1e-3, physical=True)` and its
generating parameters moved by up to 1 % of the box (seed START_SEED + P).

(N, P)                   the path
(63, 2)                  one ragged tile
(65, 2)                  two segments, the second of one point
(4160, 2)                65 tiles: two per segment, a last segment of one tile
(130, 1)                 the smallest D
(130, 24), (256, 24)     D = 76: every accumulator in use, cross bands of 39 and 38 rows
(40, 1)                  the smallest grid of the both-channel tests
Per shape the context calls jacobian (J, r, A, g, f), sandwich, and sandwich_im in both modes, each sandwich with
sigma_v = 2 sigma_u and sigma_v = sigma_u; then RAGGED as one batch through nmrfit_batch_sandwich and
nmrfit_batch_sandwich_im (both modes), under the default workspace budget and under NMRFIT_LSQ_WORKSPACE_MB=1.  The
smallest budget is 131072 doubles and RAGGED's residual rows are 47510 doubles (both channels: 95020), so RAGGED stays one group
under either; SPLIT goes through the same calls and does divide under the small budget: its (D + 1) N doubles are 45760,
1430, 45760, 45760 -- groups of three fits and one -- and twice that on both channels: groups of two, one and one.
"""
import argparse
import hashlib
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, "tests", "golden", "lsq_parent_bits.npz")

SHAPES = ((63, 2), (65, 2), (4160, 2), (130, 1), (130, 24), (256, 24), (40, 1))
RAGGED = ((130, 2), (4160, 2), (40, 1))
SPLIT = ((4160, 2), (130, 2), (4160, 2), (4160, 2))
MODES = (1, 2)
RATIOS = (2.0, 1.0)                 # sigma_v / sigma_u
BUDGETS = (None, "1")               # NMRFIT_LSQ_WORKSPACE_MB
SPEC_SEED, START_SEED = 300, 310
HASH_ABOVE = 32 * 1024              # bytes


def problem(N, P):
    """(spectrum, a point near its optimum, sigma_u)."""
    from nmrfit_amd import synth
    sp = synth.make_spectrum(N, P, seed=SPEC_SEED + P, noise=1e-3, physical=True)
    rng = np.random.default_rng(START_SEED + P)
    lo, hi = np.asarray(sp["lower"], float), np.asarray(sp["upper"], float)
    x = np.clip(np.asarray(sp["x_true"], float) + 0.01 * (hi - lo) * rng.uniform(-1.0, 1.0, lo.size), lo, hi)
    return sp, x, float(sp["sigma"])


def digest(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a, dtype=np.float64).tobytes())
    return h.hexdigest()


def input_digests():
    """{key: SHA-256 of (w, u, v, weights, lower, upper, x)} of every problem: no GPU."""
    out = {}
    for N, P in sorted(set(SHAPES + RAGGED + SPLIT)):
        sp, x, _ = problem(N, P)
        out["in/%d/%d" % (N, P)] = np.array(digest(sp["w"], sp["u"], sp["v"], sp["weights"], sp["lower"], sp["upper"], x))
    return out


def stored(a):
    """What the file keeps of an output: the array, or above HASH_ABOVE bytes the SHA-256 of its bytes."""
    a = np.ascontiguousarray(a, dtype=np.float64)
    return a if a.nbytes <= HASH_ABOVE else np.array(digest(a))


def run_cases():
    """Every recorded output, from the library this process loads: {key: array}, nothing hashed yet."""
    from nmrfit_amd import lsq
    from nmrfit_amd.batch import FitBatch
    from nmrfit_amd.equations import Evaluator
    out = {}
    for N, P in SHAPES:
        sp, x, su = problem(N, P)
        s = 1.0 / np.sqrt(N)
        with Evaluator(sp["w"], sp["u"], sp["v"], sp["weights"]) as ev:
            rows, h = lsq.ResidualModel(ev, sp["lower"], sp["upper"]).rows(x)
            got = ev.jacobian(rows, s / h, s, J=True, r=True, normal=True)
            for name in ("J", "r", "A", "g", "f"):
                out["ctx/%d/%d/jacobian/%s" % (N, P, name)] = np.asarray(got[name])
            for ratio in RATIOS:
                got = ev.sandwich(rows, s / h, s, su, ratio * su)
                for name in ("A", "M", "g", "f"):
                    out["ctx/%d/%d/sandwich/%g/%s" % (N, P, ratio, name)] = np.asarray(got[name])
                for mode in MODES:
                    got = ev.sandwich_im(rows, s / h, s, mode, su, ratio * su)
                    for name in ("A", "g", "f2", "M"):
                        out["ctx/%d/%d/sandwich_im/%d/%g/%s" % (N, P, mode, ratio, name)] = np.asarray(got[name])
    before = os.environ.get("NMRFIT_LSQ_WORKSPACE_MB")
    try:
        for batch, shapes in (("batch", RAGGED), ("split", SPLIT)):
            probs = [problem(N, P) for N, P in shapes]
            X = [p[1] for p in probs]
            su = [p[2] for p in probs]
            sv = [2.0 * p[2] for p in probs]
            for mode in (0,) + MODES:
                with FitBatch([(p[0]["w"], p[0]["u"], p[0]["v"], p[0]["weights"]) for p in probs], [p[0]["lower"] for p in probs],
                              [p[0]["upper"] for p in probs], swarmsize=8, seeds=list(range(len(probs))), fit_im=mode) as fb:
                    for budget in BUDGETS:
                        os.environ.pop("NMRFIT_LSQ_WORKSPACE_MB", None)
                        if budget is not None:
                            os.environ["NMRFIT_LSQ_WORKSPACE_MB"] = budget
                        key = "%s/%d/%s" % (batch, mode, budget or "default")
                        if mode == 0:
                            for k, (A, M, g, f) in enumerate(fb.sandwich(X, su, sv)):
                                for name, a in (("A", A), ("M", M), ("g", g), ("f", f)):
                                    out["%s/%d/%s" % (key, k, name)] = np.asarray(a)
                        else:
                            for k, (parts, meat) in enumerate(fb.sandwich_im(X, su, sv)):
                                out["%s/%d/A" % (key, k)] = np.array([p[0] for p in parts])
                                out["%s/%d/g" % (key, k)] = np.array([p[1] for p in parts])
                                out["%s/%d/rho" % (key, k)] = np.array([p[2] for p in parts])
                                out["%s/%d/M" % (key, k)] = np.array(meat)
    finally:
        os.environ.pop("NMRFIT_LSQ_WORKSPACE_MB", None)
        if before is not None:
            os.environ["NMRFIT_LSQ_WORKSPACE_MB"] = before
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", required=True, help="the commit the loaded library (NMRFIT_LIB) was built from")
    ap.add_argument("--out", default=GOLDEN)
    a = ap.parse_args()
    from nmrfit_amd import _cabi
    full = subprocess.run(["git", "-C", ROOT, "rev-parse", a.commit], capture_output=True, text=True)
    commit = full.stdout.strip() if full.returncode == 0 and full.stdout.strip() else a.commit
    if a.commit[:7] not in os.path.basename(_cabi.lib_path()):
        sys.exit("NMRFIT_LIB (%s) is not the library tools/build_at.sh built from %s" % (_cabi.lib_path(), a.commit))
    out = run_cases()
    assert all(np.all(np.isfinite(v)) for v in out.values()), [k for k, v in out.items() if not np.all(np.isfinite(v))]
    d = input_digests()
    d.update({"out/" + k: stored(v) for k, v in out.items()})
    d["parent_commit"] = np.array(commit)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    np.savez_compressed(a.out, **d)
    print("wrote %s: %d recorded arrays of commit %s, %d bytes" % (a.out, len(out), commit, os.path.getsize(a.out)))


if __name__ == "__main__":
    main()

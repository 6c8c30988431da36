#!/usr/bin/env python3
"""Inputs and recorded outputs of tests/test_gpu_chunk_body_bits.py: every path of the objective kernels' chunk body on
the smallest shapes that reach it, evaluated by ONE build of the library and kept bit for bit.

    tools/build_at.sh <commit>
    NMRFIT_LIB=nmrfit_amd/lib/libab_<commit>.so python tools/record_chunk_body_bits.py --commit <commit>

writes tests/golden/chunk_body_parent_bits.npz (needs a GPU; the commit's full hash goes into the file).  The test
loads this module for `run_cases` and compares what the working tree's library returns with np.array_equal.

The file holds data only.  What it stores in float32 (u, v, weights, the grid perturbation) is exact in float32, so the
float64 arrays the library sees are the same on every machine; the grids are w0 + step * arange(N), two IEEE operations.
A case is five particles, one per situation of the chunk body:
  0  positive amplitudes, every line outside the grid by more than its Gaussian window: no chunk is hit
  1  positive amplitudes, lines as broad as the grid: every chunk is hit (and the Gaussian recurrence applies on the
     uniformly spaced grid)
  2  narrow lines inside the grid, ONE negative amplitude: the general Lorentzian form for the whole particle
  3  the same with positive amplitudes, peak 0 so narrow and weak that its group fails the exponent budget of the
     scaled form
  4  positive amplitudes, peak 0 centred on a chunk boundary
"""
import argparse
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, "tests", "golden", "chunk_body_parent_bits.npz")

W_LO, W_HI = 3.0, 4.0
# one full chunk; full + ragged; three full + ragged; 18 chunks: blocks of two chunks, a wave's chunk loop runs twice
GRID_N = (512, 700, 1573, 8741)
PEAKS = (0, 1, 2, 7, 8, 9, 16, 24, 65)
SPACINGS = ("lin", "pert")
VARIANTS = (("default", 0), ("norec", 7), ("farfield", 6))
S = 5
# residual_batch: (N, spacing, variant, P)
ROWS = ((700, "lin", 0, 0), (700, "lin", 0, 7), (700, "lin", 0, 24), (700, "pert", 6, 8), (512, "lin", 0, 9),
        (512, "pert", 7, 65))
ROWS_IM = ((512, "lin", 9, "sum"),)               # residual rows of both channels
FIT_IM = ((1573, "lin", 9, True), (1573, "lin", 9, "sum"))
SWARM = dict(N=1573, P=8, S=16, seed=7, steps=3)
BATCH = dict(N=4096, P=6, S=12, seeds=(7, 8, 9), generations=3)


def grid(d, N, spacing):
    """The grid of length N: uniformly spaced, or the same with the stored smooth perturbation (1e-3 of the spacing)."""
    w = W_LO + float(d["step/%d" % N]) * np.arange(N, dtype=np.float64)
    if spacing == "pert":
        w = w + d["pert/%d" % N].astype(np.float64)
    return w


def spectrum(d, N, spacing):
    return (grid(d, N, spacing),) + tuple(d["%s/%d" % (k, N)].astype(np.float64) for k in ("u", "v", "weights"))


def swarm_rows(d, N, P, w):
    """X[5, 4 + 3P] of a case: the stored rows, peak 0 of particle 4 moved onto a chunk boundary of THIS grid."""
    X = np.array(d["X/%d" % P], dtype=np.float64)
    if P > 0:
        X[4, 5] = w[512 if N > 512 else 256]
    return X


def _make_rows(P, rng):
    X = np.zeros((S, 4 + 3 * P))
    X[:, 0] = rng.uniform(-0.3, 0.3, S)
    X[:, 1] = rng.uniform(-0.3, 0.3, S)
    X[:, 2] = rng.uniform(0.2, 0.8, S)
    X[:, 3] = rng.uniform(0.0, 0.01, S)
    for i in range(S):
        for k in range(P):
            width, loc, a = rng.uniform(0.005, 0.03), rng.uniform(W_LO + 0.1, W_HI - 0.1), rng.uniform(0.5, 1.5)
            if i == 0:      # outside the grid, beyond the Gaussian window (3.97 widths)
                loc = (W_HI + 0.2 + 0.01 * k) if k % 2 == 0 else (W_LO - 0.2 - 0.01 * k)
            elif i == 1:    # as broad as the grid
                width, loc = rng.uniform(0.5, 1.0), rng.uniform(W_LO + 0.2, W_HI - 0.2)
            elif i == 2 and k == P // 2:
                a = -a
            elif i == 3 and k == 0:
                width, a = 1e-13, 1e-80
            elif i == 4 and k == 0:
                width = 0.02
            X[i, 4 + 3 * k:7 + 3 * k] = (width, loc, a)
    return X


def scaled_form_ok(x, wspan=W_HI - W_LO, w0=W_LO):
    """The staging rule of the scaled Lorentzian form (objective_kernel.h, stage_peaks) for one particle, on the host:
    every aligned group of eight peaks has positive amplitudes and an exponent budget within +-250."""
    P = (len(x) - 4) // 3
    ok = True
    for g0 in range(0, P, 8):
        ehi = elo = 0
        for k in range(g0, min(P, g0 + 8)):
            width, loc, a = x[4 + 3 * k:7 + 3 * k]
            it = 2.0 / width
            lim = 1e18 / (wspan + abs(loc - w0))
            it = np.copysign(lim, it) if abs(it) > lim else it
            al = a * x[2] * it / np.pi
            if not (0.0 < al < 1e300):
                return False
            tmax = abs(it) * (wspan + abs(loc - w0))
            ehi += int(np.floor(np.log2((tmax * tmax + 1.0) / al))) + 2
            elo += int(np.floor(np.log2(1.0 / al)))
        ok = ok and ehi < 250 and elo > -250
    return ok


def make_inputs():
    from nmrfit_amd import synth
    d = {}
    for N in GRID_N:
        step = (W_HI - W_LO) / (N - 1)
        d["step/%d" % N] = np.float64(step)
        i = np.arange(N)
        d["pert/%d" % N] = (1e-3 * step * np.sin(2.0 * np.pi * 3.0 * i / N)).astype(np.float32)
        sp = synth.make_spectrum(N, 6, seed=N)
        d["u/%d" % N] = sp["u"].astype(np.float32)
        d["v/%d" % N] = sp["v"].astype(np.float32)
        wt = np.ones(N, dtype=np.float32)
        wt[N // 3:N // 2] = 0.5
        d["weights/%d" % N] = wt
    for P in PEAKS:
        d["X/%d" % P] = _make_rows(P, np.random.default_rng(1000 + P))
    # the swarm's box: narrow lines inside the grid
    rng = np.random.default_rng(77)
    lo, up = [-0.5, -0.5, 0.0, -0.01], [0.5, 0.5, 1.0, 0.01]
    for k in range(SWARM["P"]):
        c = rng.uniform(W_LO + 0.1, W_HI - 0.1)
        lo += [0.004, c - 0.03, 0.1]
        up += [0.04, c + 0.03, 2.0]
    d["swarm/lower"], d["swarm/upper"] = np.array(lo), np.array(up)
    sp = synth.make_spectrum(BATCH["N"], BATCH["P"], seed=1)
    d["step/%d" % BATCH["N"]] = np.float64((W_HI - W_LO) / (BATCH["N"] - 1))
    for k in ("u", "v"):
        d["%s/%d" % (k, BATCH["N"])] = sp[k].astype(np.float32)
    d["weights/%d" % BATCH["N"]] = np.ones(BATCH["N"], dtype=np.float32)
    d["batch/lower"], d["batch/upper"] = sp["lower"], sp["upper"]
    return d


def check_inputs(d):
    """On the CPU, before anything is recorded: the oracle's f is finite for every case (an all-NaN case would compare
    nothing), and the particles are in the form of the chunk body they are there for."""
    from oracle import c_oracle
    for N in GRID_N:
        for spacing in SPACINGS:
            w, u, v, wt = spectrum(d, N, spacing)
            for P in PEAKS:
                X = swarm_rows(d, N, P, w)
                f = c_oracle.objective_batch(X, w, u, v, wt)
                assert np.all(np.isfinite(f)), (N, spacing, P, f)
                if P > 0:
                    form = [scaled_form_ok(x) for x in X]
                    assert form == [True, True, False, False, True], (N, P, form)


def run_cases(d):
    """Every recorded output, from the library this process loads: {key: array}."""
    from nmrfit_amd.equations import Evaluator
    from nmrfit_amd.pso import DeviceSwarm
    from nmrfit_amd.batch import FitBatch
    out = {}
    for N in GRID_N:
        for spacing in SPACINGS:
            w, u, v, wt = spectrum(d, N, spacing)
            with Evaluator(w, u, v, wt) as ev:
                for vname, var in VARIANTS:
                    ev.set_variant(var)
                    for P in PEAKS:
                        out["f/%d/%s/%s/%d" % (N, spacing, vname, P)] = ev.objective_batch(swarm_rows(d, N, P, w))
                    for (n2, s2, P, mode) in FIT_IM:
                        if (n2, s2) == (N, spacing):
                            out["f_im/%d/%s/%s/%d/%s" % (N, spacing, vname, P, mode)] = ev.objective_batch(
                                swarm_rows(d, N, P, w), fit_im=mode)
                for (n2, s2, var, P) in ROWS:
                    if (n2, s2) == (N, spacing):
                        ev.set_variant(var)
                        R, f = ev.residual_batch(swarm_rows(d, N, P, w), return_f=True)
                        out["rows/%d/%s/%d/%d" % (N, spacing, var, P)] = R
                        out["rows_f/%d/%s/%d/%d" % (N, spacing, var, P)] = f
                ev.set_variant(0)
                for (n2, s2, P, mode) in ROWS_IM:
                    if (n2, s2) == (N, spacing):
                        Rre, Rim, f2 = ev.residual_batch_im(swarm_rows(d, N, P, w), mode)
                        out["rows_im/%d/%s/%d/%s" % (N, spacing, P, mode)] = np.stack([Rre, Rim])
                        out["rows_im_f/%d/%s/%d/%s" % (N, spacing, P, mode)] = f2
                if (N, spacing) == (SWARM["N"], "lin"):
                    # fused swarm generations: the objective kernel moves the particles and keeps their personal bests
                    sw = DeviceSwarm(ev, d["swarm/lower"], d["swarm/upper"], swarmsize=SWARM["S"], seed=SWARM["seed"])
                    sw.init()
                    for _ in range(1 + SWARM["steps"]):     # (the first call only folds generation 0)
                        sw.step()
                    ev.synchronize()
                    for k, a in sw.state().items():
                        out["swarm/%s" % k] = a
                    sw.close()
    # three fits as one device batch, in both geometries: the wave = particle kernels
    N = BATCH["N"]
    sp4 = spectrum(d, N, "lin")
    for mode in ("workgroup", "wave"):
        with FitBatch([sp4] * 3, [d["batch/lower"]] * 3, [d["batch/upper"]] * 3, swarmsize=BATCH["S"],
                      seeds=list(BATCH["seeds"]), minstep=0.0, minfunc=0.0) as batch:
            batch.set_geometry(mode)
            for _ in range(1 + BATCH["generations"]):
                batch.step()
            batch.synchronize()
            for k in range(3):
                for name, a in batch.state(k).items():
                    out["batch/%s/%d/%s" % (mode, k, name)] = a
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
    d = make_inputs()
    check_inputs(d)
    out = run_cases(d)
    assert all(np.all(np.isfinite(v)) for k, v in out.items()), [k for k, v in out.items() if not np.all(np.isfinite(v))]
    d.update({"out/" + k: v for k, v in out.items()})
    d["parent_commit"] = np.array(commit)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    np.savez_compressed(a.out, **d)
    print("wrote %s: %d recorded arrays of commit %s, %d bytes" % (a.out, len(out), commit, os.path.getsize(a.out)))


if __name__ == "__main__":
    main()

"""
The objective kernel's pair form (csrc/objective_pair.h: a workgroup is two particles, a wave holds a segment of both and
fetches every chunk of the grid once for the two) against the single form, bit for bit.

Every case makes two contexts in this process, one created with NMRFIT_PAIR_WAVES=1 and one with =0, and compares what
they return with np.array_equal.  The shapes are the smallest on which the pair form can go wrong:
  * grids cut into four segments: four blocks of one chunk (2048 points), the same with a ragged last chunk (1700), eight
    blocks of one chunk, two to a segment, ragged (3900), and twelve blocks of TWO chunks, three to a segment, ragged
    (12000).  (A grid of exactly four blocks of two chunks does not exist: block_plan makes up to sixteen blocks before a
    block gets a second chunk.)  The last two get their four segments through NMRFIT_TARGET_WAVES = 4 S.
  * uniform spacing (Gaussian recurrence on) and the same grid perturbed by 1e-3 of its spacing (off);
  * 0, 1, 7, 8, 9, 24 and 65 peaks; swarms of 1, 2, 5 and 8 particles (a last workgroup without a second particle);
  * rows of the five kinds of tools/record_chunk_body_bits.py -- no window hit (0), every chunk hit (1), a negative
    amplitude (2), a group outside the scaled form's exponent budget (3), a peak on a chunk boundary (4) -- ordered so that
    (scaled, general) and (general, scaled) pairs occur, and pairs of a broad-lined particle (recurrence) with a
    narrow-lined one (none) in both orders.
Then the whole state of 5- and 8-particle swarms after three fused generations, one of them stopped by the second.  At that
size the whole generation rides in the launch: this is the DEFERRED-FOLD mode (three row copies per particle, six per
workgroup, personal bests written through pflip), which the plan reaches only with NMRFIT_PAIR_WAVES=1 -- left alone it
takes the pair form from S = 8 x compute units on, beyond the 1024 particles of the deferred fold.  The modes the pair form
runs in by itself (personal best in the launch with the fold in the select kernel, personal best outside the launch, the
rank protocol, shards at odd offsets, up to 739 peaks, the plan's own choice, a change of kernel under a waiting fold) are
held in tests/test_gpu_pair_swarm_modes.py, which uses this file's helpers.
"""
import contextlib
import importlib.util
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRIDS = (2048, 1700, 3900, 12000)
NEEDS_TARGET = (3900, 12000)
PEAKS = (0, 1, 7, 8, 9, 24, 65)
# kinds of the rows, by swarm size (two orders for the two-particle swarm)
ORDERS = {1: ((4,),), 2: ((2, 1), (1, 2)), 5: ((1, 3, 2, 4, 0),), 8: ((0, 2, 3, 1, 1, 4, 2, 0),)}


def _recorder():
    spec = importlib.util.spec_from_file_location("record_chunk_body_bits",
                                                  os.path.join(ROOT, "tools", "record_chunk_body_bits.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@contextlib.contextmanager
def _env(**kv):
    old = {k: os.environ.get(k) for k in kv}
    try:
        for k, v in kv.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = str(v)
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _spectrum(N, spacing):
    from nmrfit_amd import synth
    rec = _recorder()
    step = (rec.W_HI - rec.W_LO) / (N - 1)
    w = rec.W_LO + step * np.arange(N, dtype=np.float64)
    if spacing == "pert":
        w = w + 1e-3 * step * np.sin(2.0 * np.pi * 3.0 * np.arange(N) / N)
    sp = synth.make_spectrum(N, 6, seed=N)
    wt = np.ones(N)
    wt[N // 3:N // 2] = 0.5
    return w, np.asarray(sp["u"], dtype=np.float64), np.asarray(sp["v"], dtype=np.float64), wt


def _evaluator(spec, pair, target=None):
    """A context created with the pair form forced on (1) or off (0); the knobs are read at creation."""
    from nmrfit_amd.equations import Evaluator
    with _env(NMRFIT_PAIR_WAVES=pair, NMRFIT_TARGET_WAVES=target):
        return Evaluator(*spec)


def _rows(rec, base, order, w, N):
    X = np.array([base[k] for k in order], dtype=np.float64)
    P = (X.shape[1] - 4) // 3
    if P > 0:
        for i, k in enumerate(order):
            if k == 4:
                X[i, 5] = w[512]    # peak 0 of the fifth kind: centred on a chunk boundary of this grid
    return X


def _assert_pair(ev, S):
    g = ev.last_launch()
    assert g["segments"] == 4 and g["waves_per_workgroup"] == 4, g
    assert g["waves"] == 4 * ((S + 1) // 2), (g, S)     # a wave holds a segment of TWO particles


def _assert_single(ev, S):
    g = ev.last_launch()
    assert g["segments"] == 4 and g["waves"] == 4 * S, (g, S)


@pytest.mark.gpu
@pytest.mark.parametrize("spacing", ("lin", "pert"))
@pytest.mark.parametrize("N", GRIDS)
def test_objective_values_of_the_pair_form_are_the_single_forms_bits(N, spacing):
    rec = _recorder()
    spec = _spectrum(N, spacing)
    base = {P: rec._make_rows(P, np.random.default_rng(1000 + P)) for P in PEAKS}
    bad = []
    for S, orders in ORDERS.items():
        target = 4 * S if N in NEEDS_TARGET else None
        ev1, ev0 = _evaluator(spec, 1, target), _evaluator(spec, 0, target)
        try:
            for order in orders:
                for P in PEAKS:
                    X = _rows(rec, base[P], order, spec[0], N)
                    if P > 0:   # the kinds are what they are there for: scaled form for 0, 1, 4, general for 2, 3
                        assert [rec.scaled_form_ok(x) for x in X] == [k in (0, 1, 4) for k in order]
                    f1 = ev1.objective_batch(X)
                    _assert_pair(ev1, S)
                    f0 = ev0.objective_batch(X)
                    _assert_single(ev0, S)
                    assert np.all(np.isfinite(f0)), (N, spacing, S, P, f0)
                    if not np.array_equal(f1, f0):
                        bad.append("N %d %s S %d order %s P %d: pair %r single %r" % (N, spacing, S, order, P, f1, f0))
        finally:
            ev1.close()
            ev0.close()
    assert not bad, "\n".join(bad)


def _swarm_box(rec, P):
    rng = np.random.default_rng(77)
    lo, up = [-0.5, -0.5, 0.0, -0.01], [0.5, 0.5, 1.0, 0.01]
    for _ in range(P):
        c = rng.uniform(rec.W_LO + 0.1, rec.W_HI - 0.1)
        lo += [0.004, c - 0.03, 0.1]
        up += [0.04, c + 0.03, 2.0]
    return np.array(lo), np.array(up)


def _generations(ev, box, S, seed, minfunc, steps, watch=False):
    """State, best and status of a swarm after `steps` fused generations (the first step only folds generation 0);
    watch: the swarm's best value after every step as well (reading it folds the generation in a launch of its own)."""
    from nmrfit_amd.pso import DeviceSwarm
    sw = DeviceSwarm(ev, box[0], box[1], swarmsize=S, seed=seed, minstep=0.0, minfunc=minfunc)
    try:
        sw.init()
        fg = []
        for _ in range(1 + steps):
            sw.step()
            if watch:
                fg.append(sw.status()["fg"])
        ev.synchronize()
        out = dict(sw.state())
        out["best_x"], out["best_f"] = sw.best()
        st = sw.status()
        out["status"] = np.array([st["iteration"], st["stop"], st["fg"]])
        return out, fg
    finally:
        sw.close()


@pytest.mark.gpu
@pytest.mark.parametrize("S", (5, 8))
def test_swarm_state_after_three_fused_generations_is_the_single_forms(S):
    rec = _recorder()
    N, P = 1700, 8
    spec = _spectrum(N, "lin")
    box = _swarm_box(rec, P)
    ev1, ev0 = _evaluator(spec, 1), _evaluator(spec, 0)
    try:
        # a swarm that runs on, and one that a stop ends at its second generation: the first seed whose best value
        # improves in generation 2, with minfunc between that improvement and generation 1's (found with the single form)
        cases = [(7, 0.0, False)]
        for seed in range(1, 40):
            _, fg = _generations(ev0, box, S, seed, 0.0, 3, watch=True)
            d1, d2 = fg[0] - fg[1], fg[1] - fg[2]
            if d2 > 0.0 and (d1 == 0.0 or d1 > d2):
                cases.append((seed, d2, True))
                break
        assert len(cases) == 2, "no seed below 40 whose second generation can be made the stopping one"
        for seed, minfunc, stops in cases:
            a, _ = _generations(ev1, box, S, seed, minfunc, 3)
            _assert_pair(ev1, S)
            b, _ = _generations(ev0, box, S, seed, minfunc, 3)
            _assert_single(ev0, S)
            assert (b["status"][1] != 0) == stops, (seed, minfunc, b["status"])
            if stops:
                assert b["status"][0] == 2, b["status"]     # two generations completed, the third launch carried the rows over
            for k in b:
                assert np.all(np.isfinite(b[k])), (k, b[k])
                assert np.array_equal(a[k], b[k]), "S %d seed %d minfunc %g: %s differs\n%r\n%r" % (S, seed, minfunc, k, a[k], b[k])
    finally:
        ev1.close()
        ev0.close()

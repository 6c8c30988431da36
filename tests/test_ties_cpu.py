"""
CPU tier: every swarm of tests/test_gpu_swarm_ties.py -- the same (S, N, P, Y, seed, generations) -- through the numpy
mirror (tests/swarm_support.HostSwarm) fed by the numpy oracle, with the recorder of tests/ties_support.py: each case must
really put equal finite values in front of the argmin ((a): at least two holders of the minimum, the lowest not particle
0), the personal best ((b): fx == fp with x != p) and the fold ((c): fc == fg with another row), at the exact level, and
must not stop with pyswarm's default thresholds armed.  This is where the seeds of the GPU cases are chosen: a case that
does not tie proves nothing, and on the device the same assertions are made again on the device-fed record.

(The imaginary channel is not run here: the oracle's Kramers-Kronig quadrature takes milliseconds per grid point.  Those
GPU cases use shapes and seeds that tie here in the real channel; a particle in the corner has no imaginary line at all.)
"""
import numpy as np
import pytest

from tests import swarm_support, ties_support as ts


@pytest.mark.parametrize("Y", ts.LEVELS)
@pytest.mark.parametrize("S,N,P,seed,gens", ts.LONE_SHAPES)
def test_lone_corner_swarms_tie_in_all_three_rules(S, N, P, seed, gens, Y):
    # (the oracle's per-particle loop on the GPU case's grid for the small swarms; from 1000 particles on, rows of one
    # array -- held to the oracle below -- on 96 points: the swarm, its seed and its generations are the GPU case's)
    pr = ts.corner_problem(N if S < 1000 else 96, P, Y)
    evaluate = ts.oracle_evaluator(pr) if S < 1000 else ts.corner_evaluator_rows(pr)
    rec = ts.TieRecorder(evaluate, pr["lower"], pr["upper"], S, seed).run(gens)
    n = ts.assert_ties(rec, pr["level"], "corner S=%d N=%d P=%d Y=%g seed=%d" % (S, N, P, Y, seed))
    assert rec.host.iteration == gens and rec.host.fg == pr["level"]
    if S >= 100:    # (swarms of 9 reach the corner one particle at a time)
        assert n["d"] > 0, "no generation accepts a minimum that several particles hold"
    if S == 1024:   # the deferred fold of four-wave workgroups looks at four particles per lane: two holders must share one
        assert any(ts.last_of_each_lane(k["fp"], 4) != k["first"] for k in rec.notes if k["d"])
    print(ts.line("cpu corner S=%d N=%d P=%d Y=%g seed=%d" % (S, N, P, Y, seed), n))


@pytest.mark.parametrize("P,Y,N", [(1, 0.0, 96), (1, 0.25, 96), (2, 0.25, 64), (1, 0.25, 8), (2, 0.0, 700)])
def test_rows_evaluator_is_the_oracle_bit_for_bit(P, Y, N):
    """The corner problem's objective with the particles as rows of one array (what the large swarms here run on) against
    the oracle's loop over particles, on a swarm's positions after some generations (clipped particles included), and on
    the flat problem."""
    pr = ts.corner_problem(N, P, Y)
    rec = ts.TieRecorder(ts.corner_evaluator_rows(pr), pr["lower"], pr["upper"], 300, 5).run(6)
    X = rec.host.x
    assert np.any(X[:, 6] == 0.0) and np.any(X[:, 3] == Y)
    want = ts.oracle_evaluator(pr)(X)
    np.testing.assert_array_equal(ts.corner_evaluator_rows(pr)(X), want)
    assert np.count_nonzero(want == pr["level"]) >= 2
    flat = ts.flat_problem(N, P, Y)
    np.testing.assert_array_equal(ts.corner_evaluator_rows(flat)(X), ts.oracle_evaluator(flat)(X))


@pytest.mark.parametrize("Y", ts.LEVELS)
def test_strided_swarm_ties_at_the_argmin(Y):
    """262144 + 5 particles, 3 generations (a grid of 8 points here, 64 on the device): the minimum has several holders
    and the lowest is not particle 0 -- and is one of the five particles whose wave holds a second one, which ties with it."""
    S, _, P, seed, gens = ts.STRIDED
    pr = ts.corner_problem(ts.STRIDED_CPU_N, P, Y)
    rec = ts.TieRecorder(ts.corner_evaluator_rows(pr), pr["lower"], pr["upper"], S, seed, keep_fp=True).run(gens)
    n = ts.assert_ties(rec, pr["level"], "strided Y=%g" % Y, need="a")
    assert ts.wave_mates_tie(rec) > 0, "the first holder of the minimum never ties with the other particle of its wave"
    print(ts.line("cpu strided S=%d Y=%g" % (S, Y), n))


@pytest.mark.parametrize("S,N,seed", sorted(set((S, N, seed) for _, S, N, _, seed in ts.BATCH_FITS + ts.BATCH_FITS_EQUAL)))
def test_flat_swarms_tie_everywhere_and_particle_zero_holds_g(S, N, seed):
    """The flat problem: every objective +0.0; particle 0 wins generation 0, g and p never move again, nothing stops."""
    pr = ts.flat_problem(N)
    rec = ts.TieRecorder(ts.oracle_evaluator(pr), pr["lower"], pr["upper"], S, seed)
    rec.init()
    x0 = rec.host.x.copy()
    np.testing.assert_array_equal(rec.host.g, x0[0])
    for _ in range(10):
        rec.generation()
    h = rec.host
    np.testing.assert_array_equal(h.p, x0)
    np.testing.assert_array_equal(h.g, x0[0])
    assert h.fg == 0.0 and not np.signbit(h.fg) and (h.fp == 0.0).all() and (h.iteration, h.stop) == (10, 0)
    n = rec.counts()
    assert n["a"] == 0 and n["b"] == 10 and n["c"] == 0      # everybody ties with its own best; the candidate IS g


@pytest.mark.parametrize("fits", [ts.BATCH_FITS, ts.BATCH_FITS_EQUAL], ids=["ragged", "equal"])
def test_batch_fits_tie(fits):
    seen = set()
    for kind, S, N, Y, seed in fits:
        if kind != "corner" or (S, N, Y, seed) in seen:
            continue
        seen.add((S, N, Y, seed))
        pr = ts.corner_problem(N, 1, Y)
        rec = ts.TieRecorder(ts.oracle_evaluator(pr), pr["lower"], pr["upper"], S, seed).run(ts.GENERATIONS)
        n = ts.assert_ties(rec, pr["level"], "batch fit S=%d N=%d Y=%g seed=%d" % (S, N, Y, seed))
        print(ts.line("cpu batch fit S=%d N=%d Y=%g seed=%d" % (S, N, Y, seed), n))


@pytest.mark.parametrize("S,shards", [(9, (3, 3, 3)), (204, (70, 67, 67))])
@pytest.mark.parametrize("Y", ts.LEVELS)
def test_shards_tie_across_ranks_and_equal_the_whole_swarm(S, shards, Y):
    """Three shards folded by HostSwarm.apply_global over the gathered records against the unsharded mirror; in at least one
    generation two shards post the same value, and the lowest rank's row is the one taken."""
    assert sum(shards) == S
    offsets = np.concatenate(([0], np.cumsum(shards)))
    pr = ts.corner_problem(96, 1, Y)
    ev = ts.oracle_evaluator(pr)
    whole = ts.TieRecorder(ev, pr["lower"], pr["upper"], S, 1)
    parts = [swarm_support.HostSwarm(ev, pr["lower"], pr["upper"], S, offset=int(offsets[r]), S_local=n, seed=1)
             for r, n in enumerate(shards)]
    cross = 0
    for gen in range(ts.GENERATIONS + 1):
        if gen == 0:
            whole.init()
            for h in parts:
                h.init()
        else:
            whole.generation()
            for h in parts:
                h.step_local()
        cands = np.stack([h.candidate() for h in parts])
        cross += ts.cross_rank_tie(cands)
        for h in parts:
            h.apply_global(cands)
            np.testing.assert_array_equal(h.g, whole.host.g)
            assert (h.fg, h.iteration, h.stop) == (whole.host.fg, whole.host.iteration, whole.host.stop)
        for k in ("x", "v", "p", "fx", "fp"):
            np.testing.assert_array_equal(np.concatenate([getattr(h, k) for h in parts]), getattr(whole.host, k))
    ts.assert_ties(whole, pr["level"], "shards S=%d Y=%g" % (S, Y))
    assert cross > 0, "no generation in which two shards posted the same value with different rows"

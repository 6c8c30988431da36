"""
CPU tier: what the random walks over the device batch's interface (tests/test_gpu_batch_walk.py) contain.  A walk's
operation sequence depends on its seed alone (tests/batch_walk_support.py: ``sequence``), so what it exercises can be
held here, without a device: every reader directly after a generation (a fold is pending) and directly after another
reader (nothing is pending), one-part calls on both ends of the batch, the reconstruction, the normal equations and the
polish resumed after further generations, geometry flips in every position, both ways of polling a run -- and U4's
three stopping thresholds, against HostSwarm over the C oracle.
"""
import numpy as np
import pytest

from tests import batch_walk_support as walk
from tests import swarm_support


@pytest.mark.parametrize("name", sorted(walk.SHAPES))
def test_every_committed_walk_reaches_what_it_is_for(name):
    shape = walk.SHAPES[name]
    ops = walk.sequence(shape)
    assert ops == walk.sequence(shape), "the sequence is a pure function of the seed"
    assert 90 <= len(ops) <= 110
    assert walk.unmet(shape, ops) == []
    kinds = {op[0] for op in ops}
    assert {"step", "run", "status", "best", "state", "generate", "stats_best", "stats_x", "normal", "polish", "spectrum",
            "sync"} <= kinds
    assert ("flip" in kinds) == shape.flips
    assert {op[1] for op in ops if op[0] == "generate"} == {1.0, 1.5}
    assert {op[1] == 0 for op in ops if op[0] == "normal"} == {True, False}       # at the best rows, and at random points
    first = next(i for i, op in enumerate(ops) if op[0] in walk.GENERATIONS)
    if shape.regions:       # the opening: add_noise, what is legal before the first generation, the refusals
        assert ops[0] == ("add_noise",) and ops[1] == ("add_noise_again",)
        opening = ops[2:first]
        assert {op[0] for op in opening} == {"stats_x", "normal", "spectrum", "refused"}
        assert {op[1] for op in opening if op[0] == "refused"} == {"generate", "best", "status", "stats_best"}
    else:
        assert first == 0


def test_the_parts_of_the_shapes():
    assert walk.U4.first == [0, 3, 7] and walk.U8.first == [0, 3, 6] and walk.R.first == [0, 3, 7]
    assert walk.U4P3.first == [0, 2, 4, 7]
    assert walk.REFUSED_N == (2048, 2048, 2048, 512, 64, 1000, 2048) and walk.REFUSED_S == (40, 40, 40, 16, 8, 24, 40)


def test_u4_thresholds_stop_three_fits_inside_the_walk():
    """U4's per-fit minfunc: with the numpy mirror of the swarm over the C oracle, the three fits with a threshold stop
    between generations 10 and 40 -- well inside a walk of this many generations -- and the four without never do."""
    from oracle import c_oracle
    shape = walk.U4
    total = walk.coverage(shape, walk.sequence(shape))["generations"]
    assert total >= 60
    on = [k for k, m in enumerate(shape.minfunc) if m > 0]
    assert len(on) == 3 and walk.U4F.minfunc == walk.U4P3.minfunc == shape.minfunc
    for k, sp in enumerate(walk.make_problems(shape)):
        def evaluate(X, sp=sp):
            return c_oracle.objective_batch(X, sp["w"], sp["u"], sp["v"], sp["weights"], threads=4)
        host = swarm_support.HostSwarm(evaluate, sp["lower"], sp["upper"], shape.S[k], seed=5000 + 13 * k, minstep=-1.0,
                                       minfunc=shape.minfunc[k])
        host.init()
        host.apply_global(host.candidate()[None, :])
        for _ in range(45):
            host.step_local()
            host.apply_global(host.candidate()[None, :])
        if k in on:
            assert host.stop == 1 and 10 <= host.iteration <= 40, (k, host.stop, host.iteration)
        else:
            assert host.stop == 0 and host.iteration == 45, k

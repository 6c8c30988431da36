"""
GPU tier: every argmin, personal best and fold of the swarms in front of EXACT ties.

pyswarm's three rules are strict comparisons -- the personal best moves only where fx < fp, the candidate is
p[np.argmin(fp)] (the first index of the minimum), the global best moves and the stopping rule is looked at only where
fc < fg, and among ranks the lowest wins -- and on the device they are written out in many places, each with its own index
layout (argmin_block, pso_select_kernel / select_final, the deferred folds of csrc/swarm_prologue.h, apply_wave,
pbest_particle, the objective launch's personal_best and the pair form's).  With synthetic spectra two particles never share
an objective value, so a `<=` in any of them passes every other test.  Here the problems tie by themselves
(tests/ties_support.py: the corner problem, whose clipped particles all have the objective Y exactly, and the flat problem,
where every objective is +0.0), and every launch form is held to the numpy mirror (tests/swarm_support.HostSwarm, fed by the
same context's objective_batch) bit for bit: x, v, p, fx, fp, the candidate, best() and status().  No tolerance anywhere.

Each case asserts on its own device-fed record that the ties really happened -- (a) several holders of the minimum, the
lowest not particle 0; (b) fx == fp with x != p; (c) fc == fg with another row; where the fold is deferred also (d): an
ACCEPTED minimum with several holders, the one generation whose tie-break a deferred fold leaves in g -- at the exact
level, and, with pyswarm's default thresholds ARMED, that nothing stops: a fold that accepted fc == fg would stop the
search with code 1 at once.
Each case prints its counts (pytest -s); profiles/r14/swarm_ties.txt is the record of a run.  The seeds come from
tests/test_ties_cpu.py, which runs the same swarms under the numpy oracle.
"""
import numpy as np
import pytest

from nmrfit_amd import _cabi, pso
from nmrfit_amd.batch import FitBatch
from nmrfit_amd.equations import Evaluator
from tests import swarm_support
from tests import test_gpu_pair_waves as pw
from tests import ties_support as ts

pytestmark = pytest.mark.gpu

GENS = ts.GENERATIONS
SEED = {(S, N, P): seed for S, N, P, seed, _ in ts.LONE_SHAPES}
TAIL_MAX_ELEMS = 2560      # csrc/pso.hip, tail_max_elems(): up to here ONE workgroup runs everything after the objective


def _evaluate(ev, fit_im=False):
    return lambda X: ev.objective_batch(X, fit_im=fit_im)


def _mirror(ev, pr, S, seed, gens=GENS, fit_im=False, **kw):
    return ts.Mirror(_evaluate(ev, fit_im), pr, S, seed, gens, **kw)


def _swarm(ev, pr, S, seed, pbest=None, tail=None, handover=None, **kw):
    sw = pso.DeviceSwarm(ev, pr["lower"], pr["upper"], S, seed=seed, **kw)
    if pbest is not None:
        sw.set_fused_pbest(pbest)
    if tail is not None:
        sw.set_fused_tail(tail)
    if handover is not None:
        sw.set_handover(handover)
    return sw


def _hold(dev, snap, what):
    """Everything the device swarm shows equals the mirror's snapshot, bit for bit."""
    st = dev.state()
    for k in ts.STATE:
        assert ts.same_bits(st[k], snap[k]), "%s: %s differs at %r" % (what, k, np.argwhere(st[k] != snap[k])[:5].tolist())
    assert ts.same_bits(dev.candidate(), snap["cand"]), "%s: candidate %r, mirror %r" % (what, dev.candidate(), snap["cand"])
    xb, fb = dev.best()
    assert ts.same_bits(xb, snap["best_x"]) and ts.same_bits(fb, snap["best_f"]), "%s: best %r %r, mirror %r %r" % (
        what, xb, fb, snap["best_x"], snap["best_f"])
    assert dev.status() == snap["status"], "%s: status %r, mirror %r" % (what, dev.status(), snap["status"])


def _ties(m, pr, what, gens=GENS, need="abc"):
    """The device-fed record tied in every rule, at the exact level; the armed mirror ran all its generations."""
    n = ts.assert_ties(m.rec, pr["level"], what, need)
    assert m.last["status"]["stop"] == 0 and m.last["status"]["iteration"] == gens, (what, m.last["status"])
    if "c" in need:
        assert m.last["status"]["fg"] == pr["level"], (what, m.last["status"], pr["level"])
    print(ts.line(what, n))
    return n


def _drive_run(ev, pr, S, seed, m, what, launches=None, gens=GENS, polls=None, **knobs):
    """nmrfit_pso_run, polled once at the end and after every generation."""
    for ce in polls or (gens, 1):
        dev = _swarm(ev, pr, S, seed, **knobs)
        try:
            dev.run(gens, check_every=ce)
            if launches is not None:
                assert dev.last_launches() == launches, "%s: %d launches, built for %d" % (what, dev.last_launches(), launches)
            _hold(dev, m.last, "%s run(%d, %d)" % (what, gens, ce))
        finally:
            dev.close()


def _drive_protocol(ev, pr, S, seed, m, what, launches=None, gens=GENS, **knobs):
    """The rank protocol: init, candidate, apply_global, step_local -- the candidate compared in every generation."""
    dev = _swarm(ev, pr, S, seed, **knobs)
    try:
        dev.init()
        for gen in range(gens + 1):
            if gen:
                dev.step_local()
                if launches is not None:
                    assert dev.last_launches() == launches, "%s: %d launches, built for %d" % (what, dev.last_launches(), launches)
            c = dev.candidate()
            assert ts.same_bits(c, m.snaps[gen]["cand"]), "%s: candidate of generation %d %r, mirror %r" % (
                what, gen, c, m.snaps[gen]["cand"])
            dev.apply_global(c[None, :])
        _hold(dev, m.last, what + " protocol")
    finally:
        dev.close()


def _drive_readers(ev, pr, S, seed, m, what, launches=None, gens=GENS, **knobs):
    """One generation per call with another reader after each (test_gpu_pso.test_deferred_fold_is_invisible_from_outside):
    status, best, state, candidate, none at all -- against the mirror at every generation."""
    dev = _swarm(ev, pr, S, seed, **knobs)
    try:
        dev.init()
        dev.step()                                           # folds generation 0
        for gen in range(1, gens + 1):
            dev.step()
            if launches is not None:
                assert dev.last_launches() == launches, "%s: %d launches, built for %d" % (what, dev.last_launches(), launches)
            snap, reader = m.snaps[gen], gen % 5
            if reader == 0:
                assert dev.status() == snap["status"], (what, gen, dev.status(), snap["status"])
            elif reader == 1:
                xb, fb = dev.best()
                assert ts.same_bits(xb, snap["best_x"]) and ts.same_bits(fb, snap["best_f"]), (what, gen)
            elif reader == 2:
                st = dev.state()
                for k in ts.STATE:
                    assert ts.same_bits(st[k], snap[k]), "%s: %s at generation %d" % (what, k, gen)
            elif reader == 3:
                assert ts.same_bits(dev.candidate(), snap["cand"]), (what, gen)
        _hold(dev, m.last, what + " readers")
    finally:
        dev.close()


def _context(pr, variant="default", fit_im=False):
    ev = Evaluator(*ts.spectrum(pr))
    ev.set_variant(_cabi.variant_id(variant))
    ev.set_fit_im(fit_im)
    return ev


# ---- lone swarms, corner problem ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Y", ts.LEVELS)
@pytest.mark.parametrize("S", [9, 100])
def test_single_workgroup_tail(S, Y):
    """pso_tail_kernel (S * D <= 2560): pbest_particle, argmin_block and apply_wave in one workgroup -- and argmin_block
    alone behind an objective launch that wrote the personal bests itself."""
    N, P = 96, 1
    pr = ts.corner_problem(N, P, Y)
    assert S * len(pr["lower"]) <= TAIL_MAX_ELEMS
    with _context(pr) as ev:
        m = _mirror(ev, pr, S, SEED[S, N, P])
        what = "tail S=%d N=%d Y=%g" % (S, N, Y)
        _ties(m, pr, what)
        for pbest in (False, True):
            _drive_run(ev, pr, S, SEED[S, N, P], m, what, launches=2, pbest=pbest, tail=False)
            _drive_protocol(ev, pr, S, SEED[S, N, P], m, what, launches=2, pbest=pbest)
        _drive_run(ev, pr, S, SEED[S, N, P], m, what + " defaults")


@pytest.mark.parametrize("Y", ts.LEVELS)
@pytest.mark.parametrize("mode", ["fast", "fenced", "two_launch"])
@pytest.mark.parametrize("S,N,P", [(204, 4096, 3), (1000, 2048, 1), (204, 4096, 1)])
def test_select_kernel_in_every_handover_form(S, N, P, mode, Y):
    """Fused personal bests off: pso_select_kernel's `f < cur`, its lex_less over a wave's particles and the four waves of
    a workgroup, and select_final over the posts (51 workgroups; 250 with a ragged last one).  At P = 1 a swarm of 204 is
    1428 elements and takes the single-workgroup tail instead; three peaks (2652 elements) take it to the select kernel."""
    pr = ts.corner_problem(N, P, Y)
    select = S * len(pr["lower"]) > TAIL_MAX_ELEMS
    assert select == ((S, P) != (204, 1))
    with _context(pr) as ev:
        m = _mirror(ev, pr, S, SEED[S, N, P])
        what = "select %s S=%d N=%d P=%d Y=%g" % (mode, S, N, P, Y)
        _ties(m, pr, what)
        launches = 3 if (select and mode == "two_launch") else 2
        _drive_run(ev, pr, S, SEED[S, N, P], m, what, launches=launches, pbest=False, handover=mode)


@pytest.mark.parametrize("Y", ts.LEVELS)
@pytest.mark.parametrize("tail", [True, False])
@pytest.mark.parametrize("S,N,wpb", [(204, 4096, 8), (256, 2048, 4), (1024, 4096, 4), (1025, 4096, 4)])
def test_personal_bests_in_the_objective_launch_and_the_deferred_fold(S, N, wpb, tail, Y):
    """The objective launch's own personal_best (`f < fp_old`) and, with the one-launch form on and up to 1024 particles,
    the lone swarm's deferred fold in the next launch's prologue (per-lane `vv[k] < best`, wave shuffle, per-wave LDS
    slots, acceptance rule); above, or with the form off, argmin_block and apply_wave in a launch of their own."""
    P = 1
    pr = ts.corner_problem(N, P, Y)
    with _context(pr) as ev:
        seed = SEED[S, N, P]
        m = _mirror(ev, pr, S, seed)
        what = "objective-launch pbest S=%d N=%d tail=%d Y=%g" % (S, N, tail, Y)
        _ties(m, pr, what, need="abcd")
        if S == 1024:   # four particles per lane in the fold: a `<=` there would take another holder than np.argmin does
            seen = [n for n in m.rec.notes if n["d"]]
            assert any(ts.last_of_each_lane(n["fp"], wpb) != n["first"] for n in seen), what + ": no two holders share a lane"
        launches = 1 if (tail and S <= 1024) else 2
        _drive_readers(ev, pr, S, seed, m, what, launches=launches, tail=tail)
        g = ev.last_launch()
        print("swarm_ties: %s: waves_per_workgroup=%d segments=%d" % (what, g["waves_per_workgroup"], g["segments"]))
        assert g["waves_per_workgroup"] == wpb and g["segments"] == wpb, (what, g)
        _drive_run(ev, pr, S, seed, m, what, launches=launches, tail=tail, polls=(GENS, 7))


@pytest.mark.parametrize("Y", ts.LEVELS)
@pytest.mark.parametrize("S,pbest,tail,launches", [(9, True, False, 2), (9, True, True, 1), (9, False, True, 2),
                                                   (1025, True, True, 2), (1025, False, True, 3)])
def test_pair_form(S, pbest, tail, launches, Y):
    """Two particles per workgroup (forced as tests/test_gpu_pair_swarm_modes.py forces it): the pair form's own personal
    bests for A and B, a last workgroup without a B, and the personal best outside the launch.  The mirror's objective values
    come from the pair-off context."""
    N, P = 1700, 1
    pr = ts.corner_problem(N, P, Y)
    ev1, ev0 = pw._evaluator(ts.spectrum(pr), 1, 4 * S), pw._evaluator(ts.spectrum(pr), 0, 4 * S)
    try:
        seed = SEED[S, N, P]
        m = _mirror(ev0, pr, S, seed)
        what = "pair S=%d N=%d pbest=%d tail=%d Y=%g" % (S, N, pbest, tail, Y)
        _ties(m, pr, what)
        _drive_readers(ev1, pr, S, seed, m, what, launches=launches, pbest=pbest, tail=tail)
        pw._assert_pair(ev1, S)
        _drive_run(ev1, pr, S, seed, m, what, launches=launches, pbest=pbest, tail=tail)
        pw._assert_pair(ev1, S)
    finally:
        ev1.close()
        ev0.close()


@pytest.mark.parametrize("Y", ts.LEVELS)
@pytest.mark.parametrize("variant", ["farfield", "norec"])
def test_kernel_variants(variant, Y):
    S, N, P = 204, 4096, 1
    pr = ts.corner_problem(N, P, Y)
    with _context(pr, variant) as ev:
        m = _mirror(ev, pr, S, SEED[S, N, P])
        what = "variant %s S=%d N=%d Y=%g" % (variant, S, N, Y)
        _ties(m, pr, what)
        _drive_run(ev, pr, S, SEED[S, N, P], m, what, launches=1)
        _drive_run(ev, pr, S, SEED[S, N, P], m, what + " select", pbest=False, handover="fast", polls=(GENS,))


@pytest.mark.parametrize("Y", ts.LEVELS)
@pytest.mark.parametrize("fit_im", [True, "sum"])
@pytest.mark.parametrize("S,N", [(120, 4096), (1024, 4096)])
def test_imaginary_channel(S, N, fit_im, Y):
    """fit_im=True / "sum" (test_gpu_pso.test_handover_modes_match_numpy_mirror's shapes: the select path, and the rows of a
    workgroup with the imaginary channel's second sum).  A particle in the corner has no imaginary line: the level is
    (Y + 0) / 2."""
    P = 1
    seed = SEED.get((S, N, P), 1)
    pr = ts.corner_problem(N, P, Y, fit_im=fit_im)
    assert pr["level"] == Y / 2
    with _context(pr, fit_im=fit_im) as ev:
        m = _mirror(ev, pr, S, seed, fit_im=fit_im)
        what = "fit_im=%s S=%d N=%d Y=%g" % (fit_im, S, N, Y)
        _ties(m, pr, what)
        _drive_run(ev, pr, S, seed, m, what)
        for mode in ("fast", "two_launch"):
            _drive_run(ev, pr, S, seed, m, what + " " + mode, pbest=False, handover=mode, polls=(GENS,))


@pytest.mark.parametrize("Y", ts.LEVELS)
def test_two_peaks(Y):
    S, N, P = 204, 4096, 2
    pr = ts.corner_problem(N, P, Y)
    assert pr["level"] == 2 * Y
    with _context(pr) as ev:
        m = _mirror(ev, pr, S, SEED[S, N, P])
        what = "two peaks S=%d N=%d Y=%g" % (S, N, Y)
        _ties(m, pr, what)
        _drive_run(ev, pr, S, SEED[S, N, P], m, what, launches=1)
        _drive_run(ev, pr, S, SEED[S, N, P], m, what + " tail off", launches=2, tail=False, polls=(GENS,))
        _drive_run(ev, pr, S, SEED[S, N, P], m, what + " pbest off", launches=2, pbest=False, handover="fenced", polls=(GENS,))


# ---- lone swarms, flat problem --------------------------------------------------------------------------------------------
FLAT_FORMS = [
    pytest.param(100, 96, 1, None, dict(pbest=False), 2, id="tail"),
    pytest.param(1000, 2048, 1, None, dict(pbest=False, handover="fast"), 2, id="select-fast"),
    pytest.param(1000, 2048, 1, None, dict(pbest=False, handover="fenced"), 2, id="select-fenced"),
    pytest.param(1000, 2048, 1, None, dict(pbest=False, handover="two_launch"), 3, id="select-two-launch"),
    pytest.param(204, 4096, 3, None, dict(pbest=False, handover="fast"), 2, id="select-51-workgroups"),
    pytest.param(204, 4096, 1, None, dict(), 1, id="deferred-eight-waves"),
    pytest.param(1024, 4096, 1, None, dict(), 1, id="deferred-four-waves"),
    pytest.param(1024, 4096, 1, None, dict(tail=False), 2, id="objective-pbest-own-fold"),
    pytest.param(1025, 4096, 1, None, dict(), 2, id="objective-pbest-1025"),
    pytest.param(9, 1700, 1, 1, dict(tail=False), 2, id="pair-9"),
    pytest.param(9, 1700, 1, 1, dict(), 1, id="pair-9-deferred"),
    pytest.param(1025, 1700, 1, 1, dict(), 2, id="pair-1025"),
    pytest.param(1025, 1700, 1, 1, dict(pbest=False), 3, id="pair-1025-pbest-outside"),
]


@pytest.mark.parametrize("S,N,P,pair,knobs,launches", FLAT_FORMS)
def test_flat_problem_particle_zero_wins_and_holds(S, N, P, pair, knobs, launches):
    """Every objective is +0.0: after generation 0 g is particle 0's initial row; ten generations later p is still
    generation 0's x, fg == 0.0, the iteration counts and nothing stops -- in every launch form."""
    pr = ts.flat_problem(N, P)
    if pair is None:
        ev1, ev0 = _context(pr), None
    else:
        ev1, ev0 = pw._evaluator(ts.spectrum(pr), 1, 4 * S), pw._evaluator(ts.spectrum(pr), 0, 4 * S)
    dev = _swarm(ev1, pr, S, 1, **knobs)
    try:
        m = _mirror(ev0 or ev1, pr, S, 1, gens=10)
        what = "flat S=%d N=%d P=%d %r" % (S, N, P, knobs)
        dev.init()
        x0 = dev.state()["x"]
        assert ts.same_bits(x0, m.snaps[0]["x"])
        dev.step()                                           # folds generation 0
        xb, fb = dev.best()
        assert ts.same_bits(xb, x0[0]) and ts.same_bits(fb, 0.0), (what, xb, fb)
        assert dev.status() == dict(iteration=0, stop=0, fg=0.0)
        for _ in range(10):
            dev.step()
            assert dev.last_launches() == launches, (what, dev.last_launches())
        if pair is not None:
            pw._assert_pair(ev1, S)
        st = dev.state()
        assert ts.same_bits(st["p"], x0), what + ": a personal best moved on fx == fp"
        assert ts.same_bits(st["fp"], np.zeros(S)) and ts.same_bits(st["fx"], np.zeros(S)), what
        xb, fb = dev.best()
        assert ts.same_bits(xb, x0[0]) and ts.same_bits(fb, 0.0), what + ": g moved on fc == fg"
        assert ts.same_bits(dev.candidate(), np.concatenate(([0.0], x0[0]))), what
        assert dev.status() == dict(iteration=10, stop=0, fg=0.0), (what, dev.status())
        _hold(dev, m.last, what)
        n = m.rec.counts()
        assert (n["a"], n["b"], n["c"]) == (0, 10, 0), n     # everybody ties with its own best; the candidate IS g
        print(ts.line(what, n, " (flat: all %d particles hold the minimum in all 11 generations)" % S))
    finally:
        dev.close()
        ev1.close()
        if ev0 is not None:
            ev0.close()


# ---- ranks ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Y", ts.LEVELS)
@pytest.mark.parametrize("S,shards", [(9, (3, 3, 3)), (204, (70, 67, 67))])
def test_shards_fold_ties_to_the_lowest_rank(S, shards, Y):
    """Three device shards whose records are gathered on the host and folded on the device (apply_wave, nranks = 3), three
    mirror shards folded by HostSwarm.apply_global, the unsharded device swarm and the unsharded mirror: all the same, bit
    for bit, in every generation -- with generations in which two shards post the same value with different rows."""
    N, P, seed = 96, 1, 1
    pr = ts.corner_problem(N, P, Y)
    offsets = np.concatenate(([0], np.cumsum(shards)))
    assert offsets[-1] == S
    with _context(pr) as ev:
        m = _mirror(ev, pr, S, seed)
        what = "ranks S=%d shards=%r Y=%g" % (S, shards, Y)
        n = _ties(m, pr, what)
        one = _swarm(ev, pr, S, seed)
        devs = [_swarm(ev, pr, S, seed, offset=int(offsets[r]), S_local=k) for r, k in enumerate(shards)]
        hosts = [swarm_support.HostSwarm(_evaluate(ev), pr["lower"], pr["upper"], S, offset=int(offsets[r]), S_local=k, seed=seed)
                 for r, k in enumerate(shards)]
        try:
            cross = 0
            for gen in range(GENS + 1):
                for sw in [one] + devs + hosts:
                    sw.init() if gen == 0 else sw.step_local()
                cands = np.stack([s.candidate() for s in devs])
                assert ts.same_bits(cands, np.stack([h.candidate() for h in hosts])), (what, gen)
                cross += ts.cross_rank_tie(cands)
                for sw in devs + hosts:
                    sw.apply_global(cands)
                one.apply_global(one.candidate()[None, :])
                snap = m.snaps[gen]
                for sw in devs:
                    xb, fb = sw.best()
                    assert ts.same_bits(xb, snap["best_x"]) and ts.same_bits(fb, snap["best_f"]), (what, gen, xb, snap["best_x"])
                    assert sw.status() == snap["status"], (what, gen, sw.status(), snap["status"])
                for h in hosts:
                    assert ts.same_bits(h.g, snap["g"]) and h.status() == snap["status"], (what, gen)
            tiles = [s.state() for s in devs]
            for k in ts.STATE:
                assert ts.same_bits(np.concatenate([t[k] for t in tiles]), m.last[k]), (what, k)
                assert ts.same_bits(np.concatenate([getattr(h, k) for h in hosts]), m.last[k]), (what, k)
            _hold(one, m.last, what + " unsharded")
            assert cross > 0, what + ": no generation in which two shards posted the same value with different rows"
            print(ts.line(what, n, " cross-rank ties in %d generations" % cross))
        finally:
            for sw in [one] + devs:
                sw.close()


# ---- the strided select ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pbest", [False, True])
def test_select_kernel_striding_over_a_quarter_of_a_million_particles(pbest):
    """Above 4 * kSelectMaxPosts = 262144 particles the select kernel's 65536 workgroups stride over the swarm (fused personal
    bests off); with them on, one workgroup's argmin_block strides over all of fp."""
    S, N, P, seed, gens = ts.STRIDED
    Y = 0.25
    pr = ts.corner_problem(N, P, Y)
    with _context(pr) as ev:
        m = _mirror(ev, pr, S, seed, gens=gens, keep_fp=True)
        what = "strided S=%d N=%d pbest=%d Y=%g" % (S, N, pbest, Y)
        _ties(m, pr, what, gens=gens, need="a")
        assert m.last["status"]["fg"] == pr["level"]
        # the first holder is one of the five particles whose wave looks at a second one (i + 262144), which ties with it
        assert ts.wave_mates_tie(m.rec) > 0, what + ": no tie inside a striding wave"
        _drive_run(ev, pr, S, seed, m, what, launches=None if pbest else 3, gens=gens, polls=(gens,), pbest=pbest)


# ---- device batches -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fits,fit_im,geometry", [
    pytest.param(ts.BATCH_FITS, False, "wave", id="ragged-wave"),
    pytest.param(ts.BATCH_FITS, "sum", "wave", id="ragged-wave-sum"),
    pytest.param(ts.BATCH_FITS_EQUAL, False, "wave", id="equal-wave"),
    pytest.param(ts.BATCH_FITS_EQUAL, False, "workgroup", id="equal-workgroup"),
])
def test_device_batches(fits, fit_im, geometry):
    """Seven corner and flat fits as one FitBatch (two parts): batch_tail_kernel's pbest_particle / argmin_block /
    apply_wave and the batch's own deferred fold with its 32-bit index.  state(k), status() and best() equal each fit's lone
    DeviceSwarm AND the mirror; every corner fit ties in all three rules, every flat fit in all of its particles."""
    K = len(fits)
    assert K == 7
    problems = [ts.batch_problem(kind, N, Y, fit_im=fit_im) for kind, _, N, Y, _ in fits]
    sizes = [S for _, S, _, _, _ in fits]
    seeds = [seed for _, _, _, _, seed in fits]
    evs, sws = [], []
    try:
        for pr, S, seed in zip(problems, sizes, seeds):
            evs.append(_context(pr, fit_im=fit_im))
            sws.append(_swarm(evs[-1], pr, S, seed))
        mirrors = [_mirror(ev, pr, S, seed, fit_im=fit_im) for ev, pr, S, seed in zip(evs, problems, sizes, seeds)]
        for sw in sws:
            sw.run(GENS, 7)
        with FitBatch([ts.spectrum(pr) for pr in problems], [pr["lower"] for pr in problems], [pr["upper"] for pr in problems],
                      swarmsize=sizes, seeds=seeds, fit_im=fit_im) as fb:
            fb.set_geometry(geometry)
            assert fb.geometry()["mode"] == geometry
            fb.run(GENS, 7)
            status, best = fb.status(), fb.best()
            for k, (kind, S, N, Y, seed) in enumerate(fits):
                what = "batch %s fit_im=%s fit %d %s S=%d N=%d Y=%g seed=%d" % (geometry, fit_im, k, kind, S, N, Y, seed)
                m, pr = mirrors[k], problems[k]
                if kind == "corner":
                    _ties(m, pr, what)
                else:
                    n = m.rec.counts()
                    assert (n["a"], n["b"], n["c"]) == (0, GENS, 0) and m.last["status"] == dict(iteration=GENS, stop=0, fg=0.0), (what, n)
                    assert ts.same_bits(m.last["p"], m.snaps[0]["x"]) and ts.same_bits(m.last["best_x"], m.snaps[0]["x"][0])
                    print(ts.line(what, n, " (flat)"))
                _hold(sws[k], m.last, what + " lone")
                a = fb.state(k)
                for name in ts.STATE:
                    assert ts.same_bits(a[name], m.last[name]), "%s: %s differs" % (what, name)
                assert dict(iteration=status[k]["iteration"], stop=status[k]["stop"], fg=status[k]["fg"]) == m.last["status"], (
                    what, status[k], m.last["status"])
                assert ts.same_bits(best[k][0], m.last["best_x"]) and ts.same_bits(best[k][1], m.last["best_f"]), (what, best[k])
    finally:
        for sw in sws:
            sw.close()
        for ev in evs:
            ev.close()

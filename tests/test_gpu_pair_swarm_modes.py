"""
The pair form of the objective kernel (csrc/objective_pair.h) in the modes of a swarm generation it really runs in, against
the single form and the numpy mirror, bit for bit.  tests/test_gpu_pair_waves.py holds the objective values and the
deferred-fold generations of 5 and 8 particles; left alone the plan (csrc/objective_plan.h) takes the pair form from
S = 8 x compute units on, where the fold is no longer deferred, and that mode -- the headline launch's -- is held here:

  1. generations with the personal best in the launch and the fold in the select kernel (one row per particle, no pflip:
     S = 1025, 1026 through step(), S = 5, 8 with the one-launch form switched off), with the personal best outside the
     launch, through the rank protocol against tests/swarm_support.HostSwarm evaluated by the SINGLE form, and a swarm that
     the second generation stops -- on a grid of four one-chunk blocks and on one whose blocks have two chunks;
  2. shards whose pairs are not the whole swarm's (an odd offset: every particle changes sides);
  3. peak counts up to the LDS limit of a CU (plain launches, P = 739 / 740) and of the fused update (P = 132 / 133);
  4. the plan's own choice, without NMRFIT_PAIR_WAVES, on both sides of S = 8 x compute units;
  5. a waiting fold across a change of kernel: pair-form generations folded by a FARFIELD single-form launch and back.

Every comparison is np.array_equal on whole arrays.  Every case first asks the plan itself (tests/launch_plan/
plan_query.hip, compiled for the host, with the device's compute-unit count) which form and mode its shape takes, holds
that answer to the mode the case was built for, and holds what the library reports of the launch (Evaluator.last_launch,
DeviceSwarm.last_launches) to the plan's answer: a case that lands in another mode fails.  Each case prints one record
line (pytest -s); profiles/r13/pair_swarm_modes.txt is the record of a run.
"""
import os
import subprocess

import numpy as np
import pytest

from nmrfit_amd import _cabi
from tests import swarm_support
from tests import test_gpu_pair_waves as pw

pytestmark = pytest.mark.gpu

ROOT = pw.ROOT
HIPCC = "/opt/rocm/bin/hipcc"
GRIDS = (1700, 12000)     # four blocks of one chunk, ragged; twelve blocks of two chunks, three to a segment
P_SWARM = 8
FREE = dict(minfunc=-1.0, minstep=-1.0)       # the stopping rule disarmed
STATE = ("x", "v", "p", "fx", "fp")


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    """ask(S, N, P, pair, target, mode, variant=0) -> plan_objective's answer for this device, as a dict."""
    exe = str(tmp_path_factory.mktemp("plan_query") / "plan_query")
    cc = subprocess.run([HIPCC, "--offload-arch=gfx950", "--cuda-host-only", "-O1", "-std=c++17",
                         "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "nmrfit_amd", "csrc"),
                         os.path.join(ROOT, "tests", "launch_plan", "plan_query.hip"), "-o", exe],
                        capture_output=True, text=True, timeout=300)
    assert cc.returncode == 0, cc.stderr[-3000:]
    cus = _cabi.device_info(0)["compute_units"]
    assert cus > 0

    def ask(S, N, P, pair, target, mode, variant=0):
        args = [cus, S, N, P, -1 if pair is None else pair, target or 0, variant, mode]
        run = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=60)
        assert run.returncode == 0, run.stderr
        q = dict(kv.split("=") for kv in run.stdout.split())
        return {k: (v if k == "unit" else int(v)) for k, v in q.items()}
    ask.compute_units = cus
    return ask


def _reached(plan, case, ev, S, P, pair, target, mode, want, sw=None, launches=None, variant=0):
    """The launch `ev` made last is the one this case was built for: the plan's answer for the shape is `want`, and the
    library reports the plan's geometry (and the swarm `launches` launches for the generation)."""
    q = plan(S, ev.N, P, pair, target, mode, variant)
    assert q["code"] == 0 and q["flush"] == 0, (case, q)
    for k, v in want.items():
        assert q[k] == v, "%s: the plan gives %s = %r, the case was built for %r (%r)" % (case, k, q[k], v, q)
    g = ev.last_launch()
    assert (g["waves"], g["segments"], g["waves_per_workgroup"]) == (q["waves"], q["nseg"], q["wpb"]), (case, g, q)
    if q["pair"]:
        assert q["unit"] == "pair"
        pw._assert_pair(ev, S)
    else:
        assert q["unit"] != "pair" and g["waves"] == S * q["nseg"], (case, g, q)
        assert S == 1 or not (g["segments"] == 4 and g["waves"] == 4 * ((S + 1) // 2)), (case, g)
        if q["nseg"] == 4:
            pw._assert_single(ev, S)
    n = None
    if sw is not None:
        n = sw.last_launches()
        assert n == launches, "%s: %d launches in the generation, built for %d" % (case, n, launches)
    print("pair_swarm_modes: %-58s unit=%-8s pbest=%d tail=%d rows=%d waves=%d per_workgroup=%d segments=%d launches=%s"
          % (case, q["unit"], q["pbest"], q["tail"], q["rows"], g["waves"], g["waves_per_workgroup"], g["segments"],
             "-" if n is None else n))
    return q


def _snapshot(sw):
    out = dict(sw.state())
    out["best_x"], out["best_f"] = sw.best()
    st = sw.status()
    out["status"] = np.array([st["iteration"], st["stop"], st["fg"]])
    out["candidate"] = sw.candidate()
    return out


def _same(a, b, what):
    assert set(a) == set(b)
    for k in b:
        assert np.all(np.isfinite(b[k])), (what, k, b[k])
        assert np.array_equal(a[k], b[k]), "%s: %s differs\n%r\n%r" % (what, k, a[k], b[k])


def _swarm(ev, box, S, seed, tail=True, pbest=True, minfunc=0.0, minstep=0.0, **kw):
    from nmrfit_amd.pso import DeviceSwarm
    sw = DeviceSwarm(ev, box[0], box[1], swarmsize=S, seed=seed, minstep=minstep, minfunc=minfunc, **kw)
    sw.set_fused_tail(tail)
    sw.set_fused_pbest(pbest)
    return sw


def _generations(ev, box, S, seed, steps, after=None, watch=False, **kw):
    """Snapshot of a swarm after `steps` generations through step() (the first call only folds generation 0);
    after(sw): called after every generation's launch; watch: the swarm's best value after every step as well."""
    sw = _swarm(ev, box, S, seed, **kw)
    try:
        sw.init()
        sw.step()
        fg = [sw.status()["fg"]] if watch else []
        for _ in range(steps):
            sw.step()
            if after is not None:
                after(sw)
            if watch:
                fg.append(sw.status()["fg"])
        ev.synchronize()
        return _snapshot(sw), fg
    finally:
        sw.close()


def _contexts(N, target, pair=1):
    spec = pw._spectrum(N, "lin")
    return pw._evaluator(spec, pair, target), pw._evaluator(spec, 0, target)


# ---- 1. swarm generations in the modes the pair form really runs in ---------------------------------------------------
# (S, one-launch form, personal best in the launch, what the swarm asks of the launch, the pair launch's pbest, launches)
# launches: 2 = objective + the single-workgroup select; a personal best outside the launch goes through the select
# kernel, which for more than 2560 swarm elements is posts + final reduction (csrc/pso.hip): 3
GENERATION_MODES = [
    pytest.param(1025, True, True, "fused+pbest+tail", 1, 2, id="pbest-in-launch-1025"),     # odd: the last workgroup has no B
    pytest.param(1026, True, True, "fused+pbest+tail", 1, 2, id="pbest-in-launch-1026"),
    pytest.param(5, False, True, "fused+pbest", 1, 2, id="pbest-in-launch-5-no-tail"),
    pytest.param(8, False, True, "fused+pbest", 1, 2, id="pbest-in-launch-8-no-tail"),
    pytest.param(8, True, False, "fused", 0, 2, id="pbest-outside-8"),
    pytest.param(1025, True, False, "fused", 0, 3, id="pbest-outside-1025"),
]


@pytest.mark.parametrize("S,tail,pbest,mode,want_pbest,launches", GENERATION_MODES)
@pytest.mark.parametrize("N", GRIDS)
def test_generations_without_a_deferred_fold_are_the_single_forms(plan, N, S, tail, pbest, mode, want_pbest, launches):
    rec = pw._recorder()
    box = pw._swarm_box(rec, P_SWARM)
    ev1, ev0 = _contexts(N, 4 * S)
    try:
        case = "generations N=%d S=%d %s" % (N, S, mode)
        a, _ = _generations(ev1, box, S, 7, 3, tail=tail, pbest=pbest, after=lambda sw: _reached(
            plan, case, ev1, S, P_SWARM, 1, 4 * S, mode, dict(unit="pair", pbest=want_pbest, tail=0, rows=2), sw, launches))
        b, _ = _generations(ev0, box, S, 7, 3, tail=tail, pbest=pbest, after=lambda sw: _reached(
            plan, case + " (single)", ev0, S, P_SWARM, 0, 4 * S, mode, dict(unit="default", pbest=want_pbest, tail=0, rows=1),
            sw, launches))
        assert b["status"][0] == 3 and b["status"][1] == 0, b["status"]
        _same(a, b, case)
    finally:
        ev1.close()
        ev0.close()


@pytest.mark.parametrize("S", (9, 1025))
@pytest.mark.parametrize("N", GRIDS)
def test_rank_protocol_of_a_pair_swarm_matches_the_numpy_mirror_of_the_single_form(plan, N, S):
    """init, candidate, apply_global, step_local as in test_gpu_pso.test_device_swarm_matches_numpy_mirror_bitwise: the
    device swarm runs the pair form, the mirror's objective values come from the pair-off context."""
    rec = pw._recorder()
    box = pw._swarm_box(rec, P_SWARM)
    ev1, ev0 = _contexts(N, 4 * S)
    dev = _swarm(ev1, box, S, 77, **FREE)
    try:
        host = swarm_support.HostSwarm(ev0.objective_batch, box[0], box[1], S, seed=77, **FREE)
        case = "rank protocol N=%d S=%d" % (N, S)
        dev.init()
        _reached(plan, case + " init", ev1, S, P_SWARM, 1, 4 * S, "objective", dict(unit="pair"))
        host.init()
        _reached(plan, case + " mirror", ev0, S, P_SWARM, 0, 4 * S, "objective", dict(unit="default", nseg=4))
        st = dev.state()
        for k in ("x", "v", "fx"):
            assert np.array_equal(st[k], getattr(host, k)), (case, k)
        assert np.array_equal(dev.candidate(), host.candidate())
        dev.apply_global(dev.candidate()[None, :])
        host.apply_global(host.candidate()[None, :])
        for gen in range(1, 6):
            dev.step_local()
            _reached(plan, case, ev1, S, P_SWARM, 1, 4 * S, "fused+pbest", dict(unit="pair", pbest=1, tail=0, rows=2), dev, 2)
            host.step_local()
            assert np.array_equal(dev.candidate(), host.candidate()), (case, gen)
            dev.apply_global(dev.candidate()[None, :])
            host.apply_global(host.candidate()[None, :])
        st = dev.state()
        for k in STATE:
            assert np.all(np.isfinite(getattr(host, k))), (case, k)
            assert np.array_equal(st[k], getattr(host, k)), (case, k)
        xb, fb = dev.best()
        assert np.array_equal(xb, host.best_x) and fb == host.best_f
        assert dev.status() == dict(iteration=5, stop=0, fg=host.fg)
    finally:
        dev.close()
        ev1.close()
        ev0.close()


@pytest.mark.parametrize("S", (5, 8))
@pytest.mark.parametrize("N", GRIDS)
def test_a_stop_carries_every_row_of_a_pair_over(plan, N, S):
    """The second generation stops the swarm, the fold is the select kernel's (one-launch form off): the third launch's
    workgroups carry the rows of BOTH their particles over before they return.  Then the same swarm through
    run(maxiter, check_every), polled after every generation and after every fourth."""
    rec = pw._recorder()
    box = pw._swarm_box(rec, P_SWARM)
    ev1, ev0 = _contexts(N, 4 * S)
    try:
        # the first seed whose best value improves in generation 2, with minfunc between that improvement and
        # generation 1's (found with the single form, as in tests/test_gpu_pair_waves.py)
        found = None
        for seed in range(1, 40):
            _, fg = _generations(ev0, box, S, seed, 3, tail=False, watch=True)
            d1, d2 = fg[0] - fg[1], fg[1] - fg[2]
            if d2 > 0.0 and (d1 == 0.0 or d1 > d2):
                found = (seed, d2)
                break
        assert found, "no seed below 40 whose second generation can be made the stopping one"
        seed, minfunc = found
        case = "stop N=%d S=%d seed=%d" % (N, S, seed)
        want = dict(pbest=1, tail=0)
        a, _ = _generations(ev1, box, S, seed, 3, tail=False, minfunc=minfunc, after=lambda sw: _reached(
            plan, case, ev1, S, P_SWARM, 1, 4 * S, "fused+pbest", dict(want, unit="pair", rows=2), sw, 2))
        b, _ = _generations(ev0, box, S, seed, 3, tail=False, minfunc=minfunc, after=lambda sw: _reached(
            plan, case + " (single)", ev0, S, P_SWARM, 0, 4 * S, "fused+pbest", dict(want, unit="default", rows=1), sw, 2))
        assert b["status"][1] != 0 and b["status"][0] == 2, b["status"]     # two generations completed, the third launch carried the rows over
        _same(a, b, case)
        for check_every in (1, 4):
            res = []
            for ev, pair, unit, rows in ((ev1, 1, "pair", 2), (ev0, 0, "default", 1)):
                sw = _swarm(ev, box, S, seed, tail=False, minfunc=minfunc)
                try:
                    sw.run(6, check_every)
                    _reached(plan, "%s run(6, %d) %s" % (case, check_every, unit), ev, S, P_SWARM, pair, 4 * S, "fused+pbest",
                             dict(want, unit=unit, rows=rows), sw, 2)
                    res.append(_snapshot(sw))
                finally:
                    sw.close()
            assert res[1]["status"][1] != 0 and res[1]["status"][0] == 2, res[1]["status"]
            _same(res[0], res[1], "%s run(6, %d)" % (case, check_every))
            for k in ("status", "best_x", "best_f"):
                assert np.array_equal(res[0][k], b[k]), (case, check_every, k)
    finally:
        ev1.close()
        ev0.close()


# ---- 2. shards whose pairs are not the whole swarm's -------------------------------------------------------------------
@pytest.mark.parametrize("S,shards,gens", [(9, ((0, 3), (3, 3), (6, 3)), 5), (2051, ((0, 1025), (1025, 1026)), 5)])
def test_pair_form_shards_at_odd_offsets_tile_the_single_form_swarm(plan, S, shards, gens):
    """A shard that starts at an odd particle pairs (2k + 1, 2k + 2): every particle is on the other side of its
    workgroup than in the whole swarm.  The shards run the pair form, the whole swarm the single form."""
    rec = pw._recorder()
    N = 1700
    box = pw._swarm_box(rec, P_SWARM)
    t1, t0 = 4 * max(n for _, n in shards), 4 * S
    spec = pw._spectrum(N, "lin")
    ev1, ev0 = pw._evaluator(spec, 1, t1), pw._evaluator(spec, 0, t0)
    one = _swarm(ev0, box, S, 5, **FREE)
    parts = [_swarm(ev1, box, S, 5, offset=off, S_local=n, **FREE) for off, n in shards]
    try:
        assert any(off % 2 for off, _ in shards) and sum(n for _, n in shards) == S
        case = "shards S=%d" % S

        def exchange():
            cands = np.stack([s.candidate() for s in parts])
            for s in parts:
                s.apply_global(cands)
            one.apply_global(one.candidate()[None, :])
        one.init()
        for s in parts:
            s.init()
        exchange()
        for _ in range(gens):
            one.step_local()
            _reached(plan, case + " whole", ev0, S, P_SWARM, 0, t0, "fused+pbest", dict(unit="default", pbest=1, tail=0, rows=1), one, 2)
            for s, (off, n) in zip(parts, shards):
                s.step_local()
                _reached(plan, "%s shard (%d, %d)" % (case, off, n), ev1, n, P_SWARM, 1, t1, "fused+pbest",
                         dict(unit="pair", pbest=1, tail=0, rows=2), s, 2)
            exchange()
        whole = one.state()
        tiles = [s.state() for s in parts]
        for k in STATE:
            assert np.all(np.isfinite(whole[k])), (case, k)
            assert np.array_equal(np.concatenate([t[k] for t in tiles]), whole[k]), (case, k)
        xb, fb = one.best()
        st = one.status()
        assert st["iteration"] == gens and st["stop"] == 0, st
        for s in parts:
            x, f = s.best()
            assert np.array_equal(x, xb) and f == fb
            assert s.status() == st
    finally:
        for s in parts + [one]:
            s.close()
        ev1.close()
        ev0.close()


# ---- 3. peak counts up to the LDS limit --------------------------------------------------------------------------------
BIG_PEAKS = (66, 127, 128, 129, 132, 200, 739, 740)
PAIR_MAX_P = 739      # the records of two particles with more peaks no longer fit in a CU's 160 KiB
ORDERS3 = ((1, 2, 4), (2, 1, 3))      # (scaled, general) and (general, scaled) pairs, a last workgroup without a B


@pytest.mark.parametrize("P", BIG_PEAKS)
@pytest.mark.parametrize("spacing", ("lin", "pert"))
def test_objective_values_up_to_the_lds_limit_of_the_pair_form(plan, spacing, P):
    """From P = 128 on StagePeakConstants takes a second turn per wave; at P = 739 one workgroup fills the CU's LDS; at
    740 the plan takes the single form (asked of the plan for this device, held to the boundary the LDS layout gives)."""
    rec = pw._recorder()
    S, N, target = 3, 1700, 12
    spec = pw._spectrum(N, spacing)
    base = rec._make_rows(P, np.random.default_rng(1000 + P))
    ev1, ev0 = pw._evaluator(spec, 1, target), pw._evaluator(spec, 0, target)
    try:
        for order in ORDERS3:
            X = pw._rows(rec, base, order, spec[0], N)
            assert [rec.scaled_form_ok(x) for x in X] == [k in (0, 1, 4) for k in order]
            case = "objective %s P=%d order=%s" % (spacing, P, "".join(map(str, order)))
            f1 = ev1.objective_batch(X)
            _reached(plan, case, ev1, S, P, 1, target, "objective", dict(pair=int(P <= PAIR_MAX_P), nseg=4))
            f0 = ev0.objective_batch(X)
            _reached(plan, case + " (single)", ev0, S, P, 0, target, "objective", dict(pair=0, nseg=4))
            assert np.all(np.isfinite(f0)), (case, f0)
            assert np.array_equal(f1, f0), "%s: pair %r single %r" % (case, f1, f0)
    finally:
        ev1.close()
        ev0.close()


@pytest.mark.parametrize("tail", (True, False))
@pytest.mark.parametrize("P", (132, 133))
def test_generations_at_the_limit_of_the_fused_update(plan, P, tail):
    """D = 400 = kFusedMaxD at P = 132: the pair form still carries the update (six rows per workgroup in the one-launch
    form); at P = 133 the update is a kernel of its own and the pair form carries only the objective."""
    rec = pw._recorder()
    S, N = 6, 1700
    box = pw._swarm_box(rec, P)
    ev1, ev0 = _contexts(N, 4 * S)
    try:
        case = "fused limit P=%d %s" % (P, "one launch" if tail else "no tail")
        if P == 132:
            mode = "fused+pbest+tail" if tail else "fused+pbest"
            want, launches = dict(pbest=1, tail=int(tail)), (1 if tail else 2)
            rows = 3 if tail else 1
        else:   # personal bests, argmin and fold in the single-workgroup kernel after the objective launch
            mode, want, launches, rows = "objective", dict(pbest=0, tail=0), 2, 0
        seen = []

        def after1(sw):
            m = mode + ("+pending" if mode.endswith("+tail") and seen else "")
            seen.append(_reached(plan, case, ev1, S, P, 1, 4 * S, m, dict(want, unit="pair", rows=2 * rows), sw, launches))
        seen0 = []

        def after0(sw):
            m = mode + ("+pending" if mode.endswith("+tail") and seen0 else "")
            seen0.append(_reached(plan, case + " (single)", ev0, S, P, 0, 4 * S, m, dict(want, pair=0, nseg=4, rows=rows), sw, launches))
        a, _ = _generations(ev1, box, S, 7, 3, tail=tail, after=after1)
        b, _ = _generations(ev0, box, S, 7, 3, tail=tail, after=after0)
        assert len(seen) == len(seen0) == 3 and b["status"][0] == 3 and b["status"][1] == 0, b["status"]
        _same(a, b, case)
    finally:
        ev1.close()
        ev0.close()


# ---- 4. the plan's own choice ------------------------------------------------------------------------------------------
def test_the_plan_takes_the_pair_form_by_itself_where_its_pairs_fill_the_chip(plan):
    """No NMRFIT_PAIR_WAVES, no target: from S = 8 x compute units on, on a grid long enough for four segments, the plan
    takes the pair form -- objective values and swarm generations (personal best in the launch, fold in the select
    kernel: the headline mode) -- and one particle fewer, or a grid of half the length, keeps the single form."""
    rec = pw._recorder()
    P = 2
    S = 8 * plan.compute_units
    base = rec._make_rows(P, np.random.default_rng(1000 + P))
    box = pw._swarm_box(rec, P)
    for N, S_, pair in ((32768, S, 1), (32768, S - 1, 0), (16384, S, 0)):
        spec = pw._spectrum(N, "lin")
        ev1, ev0 = pw._evaluator(spec, None), pw._evaluator(spec, 0)
        try:
            X = pw._rows(rec, base, tuple((3 * i + i // 5) % 5 for i in range(S_)), spec[0], N)
            case = "own choice N=%d S=%d" % (N, S_)
            f1 = ev1.objective_batch(X)
            _reached(plan, case, ev1, S_, P, None, 0, "objective", dict(pair=pair, nseg=4 if N == 32768 else 2))
            f0 = ev0.objective_batch(X)
            _reached(plan, case + " (pair off)", ev0, S_, P, 0, 0, "objective", dict(pair=0))
            assert np.all(np.isfinite(f0)), case
            assert np.array_equal(f1, f0), "%s: %d values differ" % (case, np.count_nonzero(f1 != f0))
            if pair:
                a, _ = _generations(ev1, box, S_, 7, 2, after=lambda sw: _reached(
                    plan, case + " step()", ev1, S_, P, None, 0, "fused+pbest+tail", dict(unit="pair", pbest=1, tail=0, rows=2), sw, 2))
                b, _ = _generations(ev0, box, S_, 7, 2, after=lambda sw: _reached(
                    plan, case + " step() (pair off)", ev0, S_, P, 0, 0, "fused+pbest+tail", dict(unit="default", pbest=1, tail=0), sw, 2))
                assert b["status"][0] == 2 and b["status"][1] == 0, b["status"]
                _same(a, b, case)
        finally:
            ev1.close()
            ev0.close()


# ---- 5. a waiting fold across a change of kernel -----------------------------------------------------------------------
def test_a_waiting_fold_of_the_pair_form_survives_a_change_of_kernel(plan):
    """test_gpu_pso.test_deferred_fold_survives_a_change_of_kernel_between_generations on a pair-on context: the pair
    form's last generation (personal bests written through pflip) is folded by the first FARFIELD launch, a single-form
    one, and FARFIELD's last by the first launch back in the pair form.  Nothing reads the swarm between the last
    generation of one kernel and the first of the next (a reader would fold the waiting generation itself); the state
    is read after that first generation, and at the end."""
    rec = pw._recorder()
    S, N = 8, 1700
    box = pw._swarm_box(rec, P_SWARM)
    ev1, ev0 = _contexts(N, 4 * S)
    sws = [_swarm(ev, box, S, 7) for ev in (ev1, ev0)]
    try:
        for sw in sws:
            sw.init()
            sw.step()
        walk = (("default", "pair", 6), ("farfield", "farfield", 3), ("default", "pair", 6))
        pending = [False, False]
        for leg, (variant, unit1, rows1) in enumerate(walk):
            for gen in range(3):
                for i, (ev, sw) in enumerate(zip((ev1, ev0), sws)):
                    if gen == 0:
                        ev.set_variant(_cabi.variant_id(variant))
                    sw.step()
                    mode = "fused+pbest+tail" + ("+pending" if pending[i] else "")
                    want = dict(unit=unit1, rows=rows1) if i == 0 else dict(unit=variant, rows=3)
                    _reached(plan, "kernel change leg %d (%s) generation %d%s" % (leg, variant, gen, "" if i == 0 else " (pair off)"),
                             ev, S, P_SWARM, 1 - i, 4 * S, mode, dict(want, pbest=1, tail=1), sw, 1, _cabi.variant_id(variant))
                    pending[i] = True
                if gen == 0 or (leg == 2 and gen == 2):
                    a, b = _snapshot(sws[0]), _snapshot(sws[1])       # (reading folds the waiting generation)
                    pending = [False, False]
                    assert b["status"][0] == 3 * leg + gen + 1 and b["status"][1] == 0, b["status"]
                    _same(a, b, "kernel change leg %d (%s) generation %d" % (leg, variant, gen))
    finally:
        for sw in sws:
            sw.close()
        ev1.close()
        ev0.close()

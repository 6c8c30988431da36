"""
GPU tier: random walks over the device batch's interface (nmrfit_batch_*, nmrfit_amd.batch.FitBatch) against its lone
fits.  One FitBatch is the subject; every fit has a lone oracle -- an Evaluator with a pso.DeviceSwarm of the same seed,
constants, thresholds, variant and fit_im, itself pinned to the numpy mirror and the restated pyswarm in
tests/test_gpu_pso.py.  A walk draws generations (step, run), readers (status, best, state, generate, residual_stats,
normal_equations, polish, spectrum), geometry flips and synchronize in an order that depends on its seed alone
(tests/batch_walk_support.py; what every committed sequence contains is held in tests/test_batch_walk_cpu.py).
Generations are mirrored on the oracles, reads compare at once, and everything is compared at the end: BIT FOR BIT, no
tolerance anywhere -- each contract is stated as bit identity in the library's own docstrings.  The oracles are never
told about the reads, so a read that disturbs the swarms, a missing flush, a wrong buffer phase or a stale descriptor
table shows as a trajectory that has left its lone fit's.  The log of the last 12 operations is in every message.
"""
import numpy as np
import pytest

from nmrfit_amd import _cabi, synth
from nmrfit_amd.batch import FitBatch
from tests import batch_walk_support as walk

pytestmark = pytest.mark.gpu


def _walked(shape):
    w = walk.Walk(shape)
    try:
        return w, w.run()
    finally:
        w.close()


def test_walk_uniform_four_wave_workgroups():
    """U4: seven fits of 2048 points in two parts (3 + 4), 40 particles, one to six peaks, both launch geometries (the
    part starts in the four-wave workgroup form: flips go both ways), three fits with a stopping threshold: they stop
    on the way while the others go on, and the walk goes on over them for ten generations and more."""
    shape = walk.U4
    w = walk.Walk(shape)
    try:
        assert w.fb.geometry() == dict(mode="workgroup", waves_per_workgroup=4, segments=4, workgroups=7 * 40)
        status = w.run()
    finally:
        w.close()
    stopped = {k: st["iteration"] for k, st in enumerate(status) if st["stop"]}
    print("U4: %d generations; stopped at %r" % (w.generations, stopped))
    assert stopped and all(shape.minfunc[k] > 0 for k in stopped)
    assert min(stopped.values()) <= w.generations - 10, (stopped, w.generations)
    assert any(st["stop"] == 0 and st["iteration"] == w.generations for st in status)


def test_walk_uniform_eight_wave_workgroups():
    """U8: six fits of 4096 points (the grid cuts into eight segments: eight-wave workgroups), stopping rule off."""
    shape = walk.U8
    w = walk.Walk(shape)
    try:
        assert w.fb.geometry() == dict(mode="workgroup", waves_per_workgroup=8, segments=8, workgroups=6 * 40)
        status = w.run()
    finally:
        w.close()
    assert all(st == dict(iteration=w.generations, stop=0, fg=st["fg"]) for st in status)


@pytest.mark.parametrize("name", ["R", "RI-sum", "RI-true"])
def test_walk_ragged(name):
    """R: seven fits of seven lengths (64 to 2048), swarm sizes and peak counts, created from regions= (the weights are
    built on the device; the oracles use utils.compute_weights), add_noise first (the oracles fit noise.replicas of the
    same inputs), then the calls that are legal before the first generation and the refusals, which leave no trace.
    RI: the same with the imaginary channel ("sum" in the default variant, and True); normal_equations and polish on
    both channels."""
    shape = walk.SHAPES[name]
    w, status = _walked(shape)
    assert w.mode == "wave" and all(st["iteration"] == w.generations for st in status)


def test_walk_uniform_farfield():
    """U4F: U4 with the far-field kernel."""
    _walked(walk.U4F)


def test_walk_three_parts(monkeypatch):
    """U4P3: U4 in three parts (2 + 2 + 3 fits) on three streams."""
    monkeypatch.setenv("NMRFIT_BATCH_STREAMS", "3")
    w = walk.Walk(walk.U4P3)
    monkeypatch.delenv("NMRFIT_BATCH_STREAMS")
    try:
        w.run()
    finally:
        w.close()


def test_two_batches_alive_together():
    """U4 and R on one device, in one thread, their operations drawn alternately from their own walks (fit_many drives
    two batches at once: they share the stream pool, the staged-copy buffers and the device): neither shows in the
    other -- each still equals its lone fits after every read and at the end."""
    a, b = walk.Walk(walk.U4), walk.Walk(walk.R)
    try:
        for i in range(max(len(a.ops), len(b.ops))):
            if i < len(a.ops):
                a.apply(i)
            if i < len(b.ops):
                b.apply(i)
        a.finish()
        b.finish()
    finally:
        a.close()
        b.close()


def test_a_refused_set_geometry_changes_nothing():
    """Fits 0..2 uniform (the first part: both forms), fits 3..6 ragged (the second part: the wave form only).  After
    some generations in the wave form set_geometry("workgroup") is refused with E_UNSUPPORTED -- and, like every other
    refusal of the library, has changed nothing: geometry() and every fit's trajectory are an untouched twin's.  (The
    trajectories are bit-identical in both forms, so only geometry() can show a first part that switched before the
    second refused.)"""
    N, S, P = walk.REFUSED_N, walk.REFUSED_S, walk.REFUSED_P
    problems = [synth.make_spectrum(n, p, seed=460 + k) for k, (n, p) in enumerate(zip(N, P))]
    seeds = [91 + k for k in range(len(N))]

    def batch():
        return FitBatch([(sp["w"], sp["u"], sp["v"], sp["weights"]) for sp in problems], [sp["lower"] for sp in problems],
                        [sp["upper"] for sp in problems], swarmsize=list(S), seeds=seeds, minstep=-1.0, minfunc=-1.0)
    with batch() as fb, batch() as twin:
        assert fb.geometry()["mode"] == "workgroup"          # (of the first part)
        for b in (fb, twin):
            b.set_geometry("wave")                            # every part has this one
            b.run(5, 2)
            b.step()                                          # (a fold is pending)
        before = twin.geometry()
        assert before["mode"] == "wave" and fb.geometry() == before
        with pytest.raises(_cabi.NmrfitError) as ei:
            fb.set_geometry("workgroup")
        assert ei.value.code == _cabi.E_UNSUPPORTED
        assert fb.geometry() == before
        for b in (fb, twin):
            b.step()
            b.run(4, 5)
        assert fb.geometry() == before
        assert fb.status() == twin.status() and all(st["iteration"] == 11 for st in fb.status())
        for k, ((x, f), (xt, ft)) in enumerate(zip(fb.best(), twin.best())):
            np.testing.assert_array_equal(x, xt)
            assert f == ft
            a, t = fb.state(k), twin.state(k)
            for name in ("x", "v", "p", "fx", "fp"):
                np.testing.assert_array_equal(a[name], t[name], err_msg="fit %d %s" % (k, name))
        # a form no part has, and a form every part has, behave as before
        with pytest.raises(_cabi.NmrfitError):
            fb.set_geometry(2)
        fb.set_geometry("wave")
        assert fb.geometry() == before


def test_fit_many_shared_options_on_one_device_and_on_a_device_list(monkeypatch):
    """Four jobs with their own seed and shared options: fit_many(jobs) and fit_many(jobs, devices=[0]) are the same
    fits -- params and error bit-identical, six generations of sixteen particles each."""
    import nmrfit_amd
    seen = []
    status = FitBatch.status

    def spy(self):
        out = status(self)
        seen.append((list(self.Ss), out))
        return out
    monkeypatch.setattr(FitBatch, "status", spy)
    jobs = []
    for k in range(4):
        sp = synth.make_spectrum(512, 2, seed=610 + k)
        jobs.append(dict(data=synth.SynthData(sp["w"], sp["u"], sp["v"], sp["peaks"]), lower=list(sp["lower"]),
                         upper=list(sp["upper"]), options={"seed": 40 + k}))
    shared = {"maxiter": 6, "swarmsize": 16}
    local = nmrfit_amd.fit_many(jobs, options=shared)
    listed = nmrfit_amd.fit_many(jobs, devices=[0], options=shared)
    for a, b in zip(local, listed):
        np.testing.assert_array_equal(a.params, b.params)
        assert a.error == b.error
    assert len(seen) == 2
    for sizes, sts in seen:
        assert sizes == [16] * 4 and [st["iteration"] for st in sts] == [6] * 4, (sizes, sts)

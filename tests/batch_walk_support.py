"""
Test infrastructure for the random walks over the device batch's interface (tests/test_gpu_batch_walk.py, conditions on
the sequences in tests/test_batch_walk_cpu.py; NOT part of the nmrfit_amd package).

A walk is a pure function of its seed: ``sequence(shape)`` draws the operations (no device needed), ``Walk`` executes
them on one ``FitBatch`` and, fit by fit, on a lone oracle -- an ``Evaluator`` with a ``pso.DeviceSwarm`` of the same
seed, constants, thresholds, variant and ``fit_im`` (itself pinned to the numpy mirror and the restated pyswarm in
tests/test_gpu_pso.py).  Writes (step, run) are mirrored on the oracles, reads compare at once and bit for bit, and the
oracles are never told about the reads: a read that changed what a later read returns shows as a difference.

Also here: ``lone_result`` / ``same_result``, the lone reconstruction and its comparison (tests/test_gpu_generate.py).
"""
import types
from typing import NamedTuple

import numpy as np

from nmrfit_amd import synth, utils

_ATTRS = ("u", "v", "V", "I", "w")


def lone_result(sp, x, scale):
    data = synth.SynthData(sp["w"], sp["u"], sp["v"], sp["peaks"])
    fu = utils.FitUtility(data, sp["lower"], sp["upper"], summary=False)
    fu.params = x
    fu.generate_result(scale)
    return fu, data


def same_result(a, b, data_a, data_b, tag):
    for name in _ATTRS:
        np.testing.assert_array_equal(getattr(a, name), getattr(b, name), err_msg="%s %s" % (tag, name))
    assert len(a.real_contribs) == len(b.real_contribs) == len(a.imag_contribs)
    for k in range(len(a.real_contribs)):
        np.testing.assert_array_equal(a.real_contribs[k], b.real_contribs[k], err_msg="%s real %d" % (tag, k))
        np.testing.assert_array_equal(a.imag_contribs[k], b.imag_contribs[k], err_msg="%s imag %d" % (tag, k))
    np.testing.assert_array_equal(data_a.V, data_b.V, err_msg=tag)
    np.testing.assert_array_equal(data_a.I, data_b.I, err_msg=tag)
    assert data_a.p0 == data_b.p0 and data_a.p1 == data_b.p1


# ---- the shapes ----------------------------------------------------------------------------------------------------

class Shape(NamedTuple):
    name: str
    N: tuple                 # grid length per fit
    S: tuple                 # swarm size per fit
    P: tuple                 # peaks per fit
    seed: int                # the walk's seed: the operation sequence depends on it (and on K, parts, flips) alone
    n_ops: int = 100
    fit_im: object = False
    variant: str = "default"
    regions: bool = False    # created from regions= (weights built on the device), add_noise first, the opening calls
    flips: bool = False      # both launch geometries exist: set_geometry is one of the operations
    minfunc: tuple = None    # per fit (None: the stopping rule is off everywhere)
    parts: int = 2           # (NMRFIT_BATCH_STREAMS when it is not the library's own choice)
    spectrum_seed: int = 400

    @property
    def K(self):
        return len(self.N)

    @property
    def first(self):         # the parts' first fits, as nmrfit_batch_create cuts them
        return [self.K * p // self.parts for p in range(self.parts + 1)]

    @property
    def channels(self):
        return "both" if self.fit_im else "real"


_U4_P = (1, 2, 3, 6, 2, 1, 4)
# U4's thresholds (fits 1, 3, 4; the rule is off for the others): chosen on the CPU, with HostSwarm over the C oracle, so
# that these three stop between generations 10 and 40 (tests/test_batch_walk_cpu.py holds them to that)
U4_MINFUNC = (-1.0, 1e-5, -1.0, 5e-5, 3e-5, -1.0, -1.0)
_R_N = (300, 513, 1025, 512, 64, 1000, 2048)
_R_S = (16, 24, 40, 16, 8, 24, 40)
_R_P = (1, 2, 3, 1, 1, 2, 1)

U4 = Shape("U4", (2048,) * 7, (40,) * 7, _U4_P, seed=747, n_ops=110, flips=True, minfunc=U4_MINFUNC)
U8 = Shape("U8", (4096,) * 6, (40,) * 6, (2, 3, 1, 4, 2, 3), seed=1032, n_ops=110, flips=True)
R = Shape("R", _R_N, _R_S, _R_P, seed=2609, regions=True)
RI_SUM = Shape("RI-sum", _R_N, _R_S, _R_P, seed=2568, regions=True, fit_im="sum")
RI_TRUE = Shape("RI-true", _R_N, _R_S, _R_P, seed=3008, regions=True, fit_im=True)
U4F = U4._replace(name="U4F", variant="farfield", seed=123)
U4P3 = U4._replace(name="U4P3", parts=3, seed=3259)
SHAPES = {s.name: s for s in (U4, U8, R, RI_SUM, RI_TRUE, U4F, U4P3)}

# the batch of the refused set_geometry: fits 0..2 uniform (the first part: both forms), fits 3..6 as in R (wave form only)
REFUSED_N, REFUSED_S, REFUSED_P = (2048,) * 3 + _R_N[3:], (40,) * 3 + _R_S[3:], (2, 1, 3) + _R_P[3:]

GENERATIONS = ("step", "run")
READERS = ("status", "best", "state", "generate", "stats_best", "polish")     # each folds a waiting generation first
# How often each operation is drawn, directly after a generation (a fold is pending: the readers' turn) and otherwise
_KINDS = ("step", "run", "status", "best", "state", "generate", "stats_best", "polish", "stats_x", "normal", "spectrum", "flip", "sync")
_AFTER_GENERATION = (8, 6, 9, 9, 12, 9, 9, 9, 2, 6, 5, 9, 2)
_OTHERWISE = (30, 18, 3, 3, 8, 4, 3, 4, 2, 6, 6, 5, 2)
_FLIP_AFTER_FLIP = 25


def _draw(rng, shape, prev):
    w = np.array(_AFTER_GENERATION if prev in GENERATIONS else _OTHERWISE, dtype=float)
    if prev == "flip":
        w[_KINDS.index("flip")] = _FLIP_AFTER_FLIP
    if not shape.flips:
        w[_KINDS.index("flip")] = 0.0
    return str(rng.choice(_KINDS, p=w / w.sum()))


def sequence(shape):
    """The walk's operations, ``(kind, argument...)`` tuples: a pure function of ``shape.seed`` (and of the shape's K,
    parts and whether it has both geometries).  Shapes made from regions open with add_noise, the calls that are legal
    before the first generation and the refusals; every walk's first drawn operation is a generation."""
    rng = np.random.default_rng(shape.seed)
    K = shape.K
    ops = []
    if shape.regions:
        ops += [("add_noise",), ("add_noise_again",), ("stats_x", 11), ("normal", 12), ("spectrum", 0), ("spectrum", K - 1),
                ("refused", "generate"), ("refused", "best"), ("refused", "status"), ("refused", "stats_best"),
                ("stats_x", 13)]
    polishes = 0
    while len(ops) < shape.n_ops:
        started = any(o[0] in GENERATIONS for o in ops)
        kind = _draw(rng, shape, ops[-1][0]) if started else str(rng.choice(GENERATIONS))
        if kind == "run":
            ops.append(("run", int(rng.integers(1, 9)), int(rng.choice([1, 2, 5]))))
        elif kind in ("state", "spectrum"):
            ops.append((kind, int(rng.integers(0, K))))
        elif kind == "generate":
            ops.append((kind, float(rng.choice([1.0, 1.5]))))
        elif kind == "stats_x":
            ops.append((kind, int(rng.integers(1, 1 << 30))))
        elif kind == "normal":      # 0: at the best rows; else the seed of random points in the boxes
            ops.append((kind, 0 if rng.integers(0, 2) else int(rng.integers(1, 1 << 30))))
        elif kind == "polish":
            subset = tuple(int(k) for k in np.flatnonzero(rng.integers(0, 2, K)))
            if not subset:
                subset = (int(rng.integers(0, K)),)
            ops.append((kind, () if polishes == 1 else subset))     # (once: nothing to refine)
            polishes += 1
        else:
            ops.append((kind,))
    return ops


def generations_of(op):
    return 1 if op[0] == "step" else op[1] if op[0] == "run" else 0


def drawn(ops):
    """The operations from the first generation on: what the seed drew (before it: a regions shape's fixed opening)."""
    return ops[next(i for i, op in enumerate(ops) if op[0] in GENERATIONS):]


def coverage(shape, ops):
    """What tests/test_batch_walk_cpu.py asserts of a sequence, as a dict of counts -- of the drawn operations: the
    fixed opening counts for nothing."""
    ops = drawn(ops)
    first = shape.first
    lo, hi = range(first[0], first[1]), range(first[-2], first[-1])
    c = dict(after_generation={k: 0 for k in READERS}, after_reader={k: 0 for k in READERS},
             state_first=0, state_last=0, spectrum_first=0, spectrum_last=0,
             resumed=dict(generate=0, normal=0, polish=0), flips_after_generation=0, flips_after_reader=0, flips_in_a_row=0,
             run_polled_at_end_only=0, run_polled_every=0, generations=sum(generations_of(o) for o in ops))
    since = {}                        # kind -> generations since its last call
    for i, op in enumerate(ops):
        kind, prev = op[0], ops[i - 1][0] if i else None
        if kind in READERS:
            c["after_generation"][kind] += prev in GENERATIONS
            c["after_reader"][kind] += prev in READERS
        if kind in ("state", "spectrum"):
            c[kind + "_first"] += op[1] in lo
            c[kind + "_last"] += op[1] in hi
        if kind in c["resumed"]:
            c["resumed"][kind] += since.get(kind, 0) >= 3
            since[kind] = 0
        if kind == "flip":
            c["flips_after_generation"] += prev in GENERATIONS
            c["flips_after_reader"] += prev in READERS
            c["flips_in_a_row"] += prev == "flip"
        if kind == "run":
            c["run_polled_at_end_only"] += op[2] > op[1]
            c["run_polled_every"] += op[2] == 1
        for k in since:
            since[k] += generations_of(op)
    return c


def unmet(shape, ops):
    """The conditions that keep a walk from being vacuous and that ``ops`` does not meet (none: [])."""
    c, out, ops = coverage(shape, ops), [], drawn(ops)

    def need(what, got, least):
        if got < least:
            out.append("%s: %d < %d" % (what, got, least))
    for kind in READERS:
        need("%s directly after a generation" % kind, c["after_generation"][kind], 3)
        need("%s directly after another reader" % kind, c["after_reader"][kind], 1)
    for part in ("first", "last"):
        need("state(k), k in the %s part" % part, c["state_" + part], 4)
        need("spectrum(k), k in the %s part" % part, c["spectrum_" + part], 2)
    for kind, n in c["resumed"].items():
        need("%s, three or more generations, %s again" % (kind, kind), n, 2)
    if shape.flips:
        need("flips directly after a generation", c["flips_after_generation"], 3)
        need("flips directly after a reader", c["flips_after_reader"], 1)
        need("two flips in a row", c["flips_in_a_row"], 1)
    need("run with check_every > n", c["run_polled_at_end_only"], 1)
    need("run with check_every = 1", c["run_polled_every"], 1)
    for kind in ("stats_x", "sync"):
        need(kind, sum(1 for o in ops if o[0] == kind), 1)
    need("normal_equations at the best rows", sum(1 for o in ops if o == ("normal", 0)), 1)
    need("normal_equations at random points", sum(1 for o in ops if o[0] == "normal" and o[1] != 0), 1)
    need("generate on the fits' own grids", sum(1 for o in ops if o == ("generate", 1.0)), 1)
    need("generate on upsampled grids", sum(1 for o in ops if o == ("generate", 1.5)), 1)
    need("polish(which=[])", sum(1 for o in ops if o[0] == "polish" and not o[1]), 1)
    return out


def make_problems(s):
    """The spectra of a shape: ``synth.make_spectrum`` per fit, with ``compute_weights`` of its peaks as the weights
    where the batch builds them from regions."""
    out = [synth.make_spectrum(n, p, seed=s.spectrum_seed + k, physical=bool(s.fit_im)) for k, (n, p) in enumerate(zip(s.N, s.P))]
    if s.regions:
        out = [dict(sp, weights=utils.compute_weights(sp["w"], sp["peaks"])) for sp in out]
    return out


def stats_regions(sp):
    """Two regions of a fit's residual statistics, in units of w: one across points 255 / 256 where the grid has them
    (the boundary of the statistics kernel's tiles), one further down."""
    w, n = sp["w"], len(sp["w"])
    a, b = min(250, n // 2), min(261, n - 1)
    c, d = n // 8, n // 4
    return [tuple(sorted((w[a], w[b]))), tuple(sorted((w[c], w[d])))]


def box_points(problems, seed):
    rng = np.random.default_rng(seed)
    return [sp["lower"] + rng.random(len(sp["lower"])) * (sp["upper"] - sp["lower"]) for sp in problems]


# ---- the walk on the device ------------------------------------------------------------------------------------------

class Lone:
    """One fit's oracle: the lone swarm on a context of its own, and a second, untouched context for the lone
    least-squares calls (``lsq.ResidualModel(Evaluator(spectrum), ...)``)."""

    def __init__(self, sp, S, seed, variant, fit_im, minfunc):
        from nmrfit_amd import _cabi, lsq, pso
        from nmrfit_amd.equations import Evaluator
        self.sp = sp
        self.ev = Evaluator(sp["w"], sp["u"], sp["v"], sp["weights"])
        self.ev.set_variant(_cabi.variant_id(variant))
        self.ev.set_fit_im(fit_im)
        self.sw = pso.DeviceSwarm(self.ev, sp["lower"], sp["upper"], S, seed=seed, minstep=-1.0, minfunc=minfunc)
        self.plain = Evaluator(sp["w"], sp["u"], sp["v"], sp["weights"])
        self.model = lsq.ResidualModel(self.plain, sp["lower"], sp["upper"], **(dict(fit_im=fit_im) if fit_im else {}))
        self.started = False

    def generations(self, n, check_every=None):
        """What ``FitBatch.step`` (n None) / ``FitBatch.run(n, check_every)`` do to this fit."""
        if not self.started:
            self.sw.init()
            self.sw.step()               # (folds generation 0)
            self.started = True
            if n is None:
                return
        if n is None:
            self.sw.step()
        else:
            self.sw.run(n, check_every)

    def close(self):
        self.sw.close()
        self.ev.close()
        self.plain.close()


class Walk:
    """One batch, its oracles and its operations; ``apply(i)`` executes operation i (so that two walks can alternate)."""

    def __init__(self, shape, ops=None):
        from nmrfit_amd.batch import FitBatch
        self.shape, self.ops = shape, sequence(shape) if ops is None else ops
        self.problems = make_problems(shape)
        K = shape.K
        self.seeds = [5000 + 13 * k for k in range(K)]
        self.minfunc = list(shape.minfunc) if shape.minfunc else [-1.0] * K
        sps = self.problems
        kw = dict(swarmsize=list(shape.S), seeds=self.seeds, minstep=-1.0, minfunc=self.minfunc, variant=shape.variant,
                  fit_im=shape.fit_im)
        if shape.regions:
            self.fb = FitBatch([(sp["w"], sp["u"], sp["v"]) for sp in sps], [sp["lower"] for sp in sps],
                               [sp["upper"] for sp in sps], regions=[utils.weight_regions(sp["w"], sp["peaks"]) for sp in sps], **kw)
        else:
            self.fb = FitBatch([(sp["w"], sp["u"], sp["v"], sp["weights"]) for sp in sps], [sp["lower"] for sp in sps],
                               [sp["upper"] for sp in sps], **kw)
        self.lone = []
        self.regions = [stats_regions(sp) for sp in sps]
        self.log = []
        self.mode = self.fb.geometry()["mode"]
        self.generations = 0
        if not shape.regions:
            self._make_oracles()

    def _make_oracles(self):
        s = self.shape
        self.lone = [Lone(sp, s.S[k], self.seeds[k], s.variant, s.fit_im, self.minfunc[k]) for k, sp in enumerate(self.problems)]

    def close(self):
        for o in self.lone:
            o.close()
        self.fb.close()

    # -- comparisons (each takes the tag that carries the log) --
    def _status(self, tag):
        got = self.fb.status()
        for k, o in enumerate(self.lone):
            assert got[k] == o.sw.status(), "status of fit %d: %r != %r, %s" % (k, got[k], o.sw.status(), tag)
        return got

    def _best(self, tag):
        for k, ((x, f), o) in enumerate(zip(self.fb.best(), self.lone)):
            xb, fbest = o.sw.best()
            np.testing.assert_array_equal(x, xb, err_msg="best row of fit %d, %s" % (k, tag))
            assert f == fbest, "best value of fit %d: %r != %r, %s" % (k, f, fbest, tag)

    def _state(self, k, tag):
        a, b = self.fb.state(k), self.lone[k].sw.state()
        for name in ("x", "v", "p", "fx", "fp"):
            np.testing.assert_array_equal(a[name], b[name], err_msg="%s of fit %d, %s" % (name, k, tag))

    def _generate(self, scale, tag):
        for k, (r, o) in enumerate(zip(self.fb.generate(scale), self.lone)):
            x = o.sw.best()[0]
            fu, data = lone_result(o.sp, x, scale)
            got = types.SimpleNamespace(w=o.sp["w"] if r["w"] is None else r["w"], real_contribs=list(r["real"]),
                                        imag_contribs=list(r["imag"]), **{n: r[n] for n in ("u", "v", "V", "I")})
            got_data = types.SimpleNamespace(V=r["data_V"], I=r["data_I"], p0=x[0], p1=x[1])
            assert (r["w"] is None) == (scale == 1)
            same_result(got, fu, got_data, data, "generate(%r) of fit %d, %s" % (scale, k, tag))

    def _stats(self, X, tag):
        from nmrfit_amd import quality
        got = self.fb.residual_stats(X, self.regions)
        for k, sp in enumerate(self.problems):
            x = self.lone[k].sw.best()[0] if X is None else X[k]
            want = quality.residual_stats(sp["w"], sp["u"], sp["v"], x, self.regions[k])
            assert np.array_equal(got[k].rows, want.rows, equal_nan=True), "residual_stats of fit %d, %s" % (k, tag)

    def _normal(self, X, tag):
        got = self.fb.normal_equations(X, channels=self.shape.channels)
        for k, o in enumerate(self.lone):
            A, g, f = o.model.normal_equations(X[k])
            np.testing.assert_array_equal(got[k][0], A, err_msg="A of fit %d, %s" % (k, tag))
            np.testing.assert_array_equal(got[k][1], g, err_msg="g of fit %d, %s" % (k, tag))
            assert got[k][2] == f, "f of fit %d: %r != %r, %s" % (k, got[k][2], f, tag)

    def _polish(self, which, tag):
        from nmrfit_amd import lsq
        got = self.fb.polish(which=list(which), channels=self.shape.channels, max_launches=3)
        want = [o.sw.best() for o in self.lone]
        if which:
            def provider(trial):
                return [None if x is None else self.lone[k].model.normal_equations(x) for k, x in zip(which, trial)]
            Xw, fw, _ = lsq.lm_polish(provider, [want[k][0] for k in which], [self.problems[k]["lower"] for k in which],
                                      [self.problems[k]["upper"] for k in which], max_launches=3)
            for k, x, f in zip(which, Xw, fw):
                want[k] = (x, float(f))
        for k, ((x, f), (xw, fw_)) in enumerate(zip(got, want)):
            np.testing.assert_array_equal(x, xw, err_msg="polished x of fit %d, %s" % (k, tag))
            assert f == fw_, "polished f of fit %d: %r != %r, %s" % (k, f, fw_, tag)

    def _spectrum(self, k, tag):
        u, v = self.fb.spectrum(k)
        np.testing.assert_array_equal(u, self.problems[k]["u"], err_msg="u of fit %d, %s" % (k, tag))
        np.testing.assert_array_equal(v, self.problems[k]["v"], err_msg="v of fit %d, %s" % (k, tag))

    def _add_noise(self):
        from nmrfit_amd import noise
        sps = self.problems
        su = [0.0 if k == 4 else 0.5 * sp["sigma"] for k, sp in enumerate(sps)]       # (fit 4: both sigmas 0, not touched)
        sv = [0.0 if k == 4 else 0.25 * sp["sigma"] for k, sp in enumerate(sps)]
        self.noise = (su, sv, [7000 + k for k in range(len(sps))])
        self.fb.add_noise(*self.noise)
        noisy = noise.replicas([sp["u"] for sp in sps], [sp["v"] for sp in sps], *self.noise)
        self.problems = [dict(sp, u=u, v=v) for sp, (u, v) in zip(sps, noisy)]
        assert not np.array_equal(self.problems[0]["u"], sps[0]["u"]) and np.array_equal(self.problems[4]["u"], sps[4]["u"])
        self._make_oracles()      # the oracles fit the replicas

    def _refused(self, what, tag):
        import pytest
        from nmrfit_amd import _cabi
        call = dict(generate=self.fb.generate, best=self.fb.best, status=self.fb.status,
                    stats_best=lambda: self.fb.residual_stats(None, self.regions),
                    add_noise_again=lambda: self.fb.add_noise(*self.noise))[what]
        with pytest.raises(_cabi.NmrfitError) as ei:
            call()
        assert ei.value.code == _cabi.E_STATE, "%s: code %r, %s" % (what, ei.value.code, tag)

    def apply(self, i):
        op = self.ops[i]
        kind = op[0]
        self.log.append(op)
        tag = "walk %s seed %d, operation #%d of %s" % (self.shape.name, self.shape.seed, i, self.log[-12:])
        fb = self.fb
        if kind == "step":
            fb.step()
            self.generations += int(any(o.started for o in self.lone))
            for o in self.lone:
                o.generations(None)
        elif kind == "run":
            fb.run(op[1], op[2])
            self.generations += op[1]
            for o in self.lone:
                o.generations(op[1], op[2])
            self._status(tag)
        elif kind == "status":
            self._status(tag)
        elif kind == "best":
            self._best(tag)
        elif kind == "state":
            self._state(op[1], tag)
        elif kind == "generate":
            self._generate(op[1], tag)
        elif kind == "stats_best":
            self._stats(None, tag)
        elif kind == "stats_x":
            self._stats(box_points(self.problems, op[1]), tag)
        elif kind == "normal":
            started = self.lone and self.lone[0].started
            self._normal([o.sw.best()[0] for o in self.lone] if op[1] == 0 and started else box_points(self.problems, op[1] or 1), tag)
        elif kind == "polish":
            self._polish(op[1], tag)
        elif kind == "spectrum":
            self._spectrum(op[1], tag)
        elif kind == "flip":
            self.mode = "wave" if self.mode == "workgroup" else "workgroup"
            fb.set_geometry(self.mode)
            assert fb.geometry()["mode"] == self.mode, tag
        elif kind == "sync":
            fb.synchronize()
        elif kind == "add_noise":
            self._add_noise()
        elif kind == "add_noise_again":
            self._refused("add_noise_again", tag)
        elif kind == "refused":
            self._refused(op[1], tag)
        else:
            raise AssertionError("unknown operation %r" % (op,))

    def finish(self):
        """After the last operation: everything, for every fit."""
        tag = "walk %s seed %d, at the end (%s)" % (self.shape.name, self.shape.seed, self.log[-12:])
        for k in range(self.shape.K):
            self._state(k, tag)
            self._spectrum(k, tag)
        st = self._status(tag)
        self._best(tag)
        self._generate(1.0, tag)
        self._stats(None, tag)
        assert self.fb.geometry()["mode"] == self.mode, tag
        return st

    def run(self):
        for i in range(len(self.ops)):
            self.apply(i)
        return self.finish()

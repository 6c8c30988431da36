"""
Test infrastructure for exact ties in the swarm (NOT part of the nmrfit_amd package): problems whose particles share an
objective value bit for bit, and a recorder round ``swarm_support.HostSwarm`` that notes, generation by generation, whether
the three strict comparisons of pyswarm were really put in front of equal values:

  (a) the minimum of ``fp`` is held by at least two particles and the lowest of them is not particle 0 -- the candidate is
      ``p[np.argmin(fp)]``, the FIRST index of the minimum;
  (b) some particle has ``fx == fp`` with ``x != p`` -- the personal best moves only where ``fx < fp``;
  (c) the candidate's value equals ``fg`` while its row differs from ``g`` -- the global best moves, and the stopping rule is
      looked at, only where ``fc < fg``;
  (d) (noted as well) the fold ACCEPTS a value that several particles hold: there the argmin's tie-break shows in g itself.

Nobody can place particles (there is no set-state call, and a box needs ``ub > lb``), so the ties come from the dynamics:

``corner_problem``  a grid ``linspace(3, 4, N)`` with ``u = v = 0`` and unit weights; x = [p0, p1, r, yoff, (width, loc, a) x P]
                    in a box whose ``yoff`` ends at Y and whose amplitudes end at 0.  Every residual is
                    ``sum_k (yoff + a_k shape_k)``: a particle clipped to ``a = 0`` and ``yoff = Y`` has an objective of
                    exactly ``P * Y`` whatever its other coordinates are (for Y = 0.25: N squares of 0.0625 or 0.25, their
                    sum, the division and the root are all exact), and nothing lies below that level.  Particles reach the
                    corner through pyswarm's clipping at different generations and with different rows, which makes the
                    winner's index visible in g, p and the candidate record.  With the imaginary channel the level is
                    ``(P * Y + 0) / 2``: its residual has no offset.
``flat_problem``    the same with every weight 0: every objective is +0.0 in every generation, the whole swarm ties, and
                    particle 0 must win generation 0 and hold g for good.

The recorder is additive: HostSwarm's own arithmetic is left alone.
"""
import numpy as np

from tests import swarm_support

LEVELS = (0.0, 0.25)


def corner_problem(N, P=1, Y=0.0, fit_im=False):
    """dict(w, u, v, weights, lower, upper, level): the corner problem on N points with P peaks and its tied level."""
    w = np.linspace(3.0, 4.0, N)
    lower = np.array([-1.0, -1.0, 0.0, Y] + [0.02, 3.2, 0.0] * P)
    upper = np.array([1.0, 1.0, 1.0, 1.0] + [0.2, 3.8, 1.0] * P)
    level = P * Y if fit_im is False else (P * Y + 0.0) / 2.0
    return dict(w=w, u=np.zeros(N), v=np.zeros(N), weights=np.ones(N), lower=lower, upper=upper, level=level, N=N, P=P, Y=Y)


def flat_problem(N, P=1, Y=0.0):
    """The corner problem with every weight 0: all objectives are +0.0."""
    pr = corner_problem(N, P, Y)
    pr["weights"] = np.zeros(N)
    pr["level"] = 0.0
    return pr


def spectrum(pr):
    return pr["w"], pr["u"], pr["v"], pr["weights"]


def oracle_evaluator(pr):
    """evaluate(X) -> f through the numpy oracle (the CPU tier's evaluator)."""
    from oracle import nmrfit_oracle as onp
    return lambda X: onp.objective_batch(X, pr["w"], pr["u"], pr["v"], pr["weights"])


def corner_evaluator_rows(pr):
    """The oracle's objective for the corner / flat problem (u = v = 0: the phased data are zero whatever p0, p1) with the
    particles as rows of one array instead of a Python loop over them -- the same elementwise operations in the same order
    and numpy's same pairwise sum over each row, so the same bits (tests/test_ties_cpu.py holds it to the oracle): what makes
    a swarm of a quarter of a million particles affordable on the CPU."""
    w, weights = pr["w"][None, :], pr["weights"][None, :]
    assert not pr["u"].any() and not pr["v"].any()

    def evaluate(X):
        X = np.asarray(X, dtype=np.float64)
        r, yoff = X[:, 2:3], X[:, 3:4]
        V_data = np.zeros((X.shape[0], w.shape[1]))
        V_fit = np.zeros_like(V_data)
        for i in range(4, X.shape[1], 3):
            width, loc, a = X[:, i:i + 1], X[:, i + 1:i + 2], X[:, i + 2:i + 3]
            L = (2 / (np.pi * width)) * 1 / (1 + ((w - loc) / (0.5 * width)) ** 2)
            G = (2 / width) * np.sqrt(np.log(2) / np.pi) * np.exp(-((w - loc) / (width / (2 * np.sqrt(np.log(2))))) ** 2)
            V_fit = V_fit + (yoff + a * (r * L + (1 - r) * G))
        return np.sqrt(np.square(np.multiply(weights, (V_data - V_fit))).mean(axis=1))
    return evaluate


class TieRecorder:
    """A HostSwarm stepped one generation at a time, with a note per generation of the conditions (a), (b), (c) above and
    of the tied level (the minimum of fp), taken after the personal bests and the candidate, before the fold.

    ``exchange(cand) -> rows`` gathers the candidate records of all shards (default: this swarm alone)."""

    def __init__(self, evaluate, lower, upper, swarmsize, seed, exchange=None, keep_fp=False, **kw):
        self.host = swarm_support.HostSwarm(evaluate, lower, upper, swarmsize, seed=seed, **kw)
        self.exchange = exchange
        self.keep_fp = keep_fp   # a copy of fp in every note (otherwise only in those of (d))
        self.notes = []          # one dict(a, b, c, level, holders) per generation, generation 0 first

    def note(self):
        h = self.host
        level = h.fp.min()
        holders = np.flatnonzero(h.fp == level)
        a = holders.size >= 2 and holders[0] != 0
        b = bool(np.any((h.fx == h.fp) & np.any(h.x != h.p, axis=1)))
        c = bool(h._seeded and h.cand[0] == h.fg and np.any(h.cand[1:] != h.g))
        # (d) the fold is about to ACCEPT (fc < fg) a value that several particles hold: the one generation in which the
        # argmin's tie-break shows in g itself, which is all a deferred fold leaves behind (the candidate record a reader
        # sees is written again by the launch that folds for it)
        d = bool(h._seeded and h.cand[0] < h.fg and holders.size >= 2)
        self.notes.append(dict(a=bool(a), b=b, c=c, d=d, level=float(level), holders=int(holders.size), first=int(holders[0]),
                               fp=h.fp.copy() if (d or self.keep_fp) else None))

    def fold(self):
        h = self.host
        h.apply_global(h.candidate()[None, :] if self.exchange is None else self.exchange(h.candidate()))

    def init(self, fold=True):
        self.host.init()
        self.note()
        if fold:
            self.fold()

    def generation(self, fold=True):
        self.host.step_local()
        self.note()
        if fold:
            self.fold()

    def run(self, generations):
        self.init()
        for _ in range(generations):
            self.generation()
        return self

    def counts(self):
        """Generations in which (a), (b) and (c) held."""
        return {k: sum(n[k] for n in self.notes) for k in "abcd"}

    def tied_levels(self):
        """The minimum of fp in every generation where at least two particles held it."""
        return [n["level"] for n in self.notes if n["holders"] >= 2]


def assert_ties(rec, level, what, need="abc"):
    """Each of the conditions in `need` held in at least one generation, every tie at the minimum was at `level` exactly,
    and the mirror did not stop.  Returns the counts (printed by the callers: the record of a run)."""
    n = rec.counts()
    for k in need:
        assert n[k] > 0, "%s: condition (%s) never held: %r -- the case does not tie and proves nothing" % (what, k, n)
    tied = rec.tied_levels()
    assert tied and all(v == level for v in tied), "%s: tied levels %r, expected exactly %r" % (what, sorted(set(tied)), level)
    assert rec.host.stop == 0, "%s: the mirror stopped with code %d at iteration %d" % (what, rec.host.stop, rec.host.iteration)
    return n


STATE = ("x", "v", "p", "fx", "fp")


def snapshot(h):
    """What a swarm shows to the outside after a generation's fold, as copies."""
    out = {k: getattr(h, k).copy() for k in STATE}
    out.update(cand=h.candidate().copy(), best_x=h.best_x.copy(), best_f=float(h.best_f), g=h.g.copy(), status=h.status())
    return out


class Mirror:
    """The mirror of one swarm, run for `generations` with the recorder: snaps[k] is its state after generation k's fold."""

    def __init__(self, evaluate, pr, S, seed, generations, **kw):
        self.rec = TieRecorder(evaluate, pr["lower"], pr["upper"], S, seed, **kw)
        self.rec.init()
        self.snaps = [snapshot(self.rec.host)]
        for _ in range(generations):
            self.rec.generation()
            self.snaps.append(snapshot(self.rec.host))
        self.host, self.last = self.rec.host, self.snaps[-1]


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(np.all(a.view(np.uint64) == b.view(np.uint64)))


def last_of_each_lane(fp, waves, lanes=64):
    """What the lone swarm's deferred fold would take if its per-lane test were `<=`: wave w, lane l looks at the particles
    w * kper * 64 + l + 64 k in ascending order and keeps the LAST of its minima; across lanes and waves the lowest index of
    the minimum wins.  Equal to np.argmin(fp) unless two holders of the minimum share a lane."""
    S = len(fp)
    kper = -(-S // (waves * lanes))
    picks = []
    for w in range(waves):
        for l in range(lanes):
            idx = w * kper * lanes + l + lanes * np.arange(kper)
            idx = idx[idx < S]
            if idx.size:
                picks.append(int(idx[np.flatnonzero(fp[idx] == fp[idx].min())[-1]]))
    picks = np.array(sorted(picks))
    return int(picks[np.argmin(fp[picks])])


def wave_mates_tie(rec, stride=4 * 65536):
    """Generations of a recorder (keep_fp=True) in which the first holder of the minimum shares its wave of the strided
    select kernel (4 waves x kSelectMaxPosts = 65536 workgroups) with another holder (particle i and i + stride): where that wave's own tie-break shows."""
    out = 0
    for n in rec.notes:
        i, fp = n["first"], n["fp"]
        out += bool(i + stride < len(fp) and fp[i + stride] == n["level"])
    return out


def cross_rank_tie(cands):
    """The gathered records' minimum is posted by at least two ranks, with different rows (the fold must take the lowest
    rank's)."""
    cands = np.asarray(cands)
    holders = np.flatnonzero(cands[:, 0] == cands[:, 0].min())
    return bool(holders.size >= 2 and any(np.any(cands[k, 1:] != cands[holders[0], 1:]) for k in holders[1:]))


def line(what, n, extra=""):
    return "swarm_ties: %-78s (a)=%-3d (b)=%-3d (c)=%-3d (d)=%-2d%s" % (what, n["a"], n["b"], n["c"], n["d"], extra)


# ---- the cases of tests/test_gpu_swarm_ties.py, run by tests/test_ties_cpu.py with the numpy oracle first ----------------
# (S, N, P, seed, generations): the lone swarms, whatever launch form they are run in; both levels each
GENERATIONS = 30
LONE_SHAPES = [
    (9, 96, 1, 1, GENERATIONS),          # the single-workgroup tail
    (100, 96, 1, 1, GENERATIONS),
    (204, 4096, 1, 1, GENERATIONS),      # 51 select workgroups; the eight-wave form
    (1000, 2048, 1, 1, GENERATIONS),     # ragged last select workgroup
    (256, 2048, 1, 1, GENERATIONS),      # the four-wave form
    (1024, 4096, 1, 5, GENERATIONS),     # (seed 5: the accepted generation's minimum is held twice within a lane's share)
    (1025, 4096, 1, 1, GENERATIONS),     # the fold is its own launch
    (9, 1700, 1, 1, GENERATIONS),        # the pair form: the last workgroup has no B
    (1025, 1700, 1, 1, GENERATIONS),
    (120, 4096, 1, 1, GENERATIONS),      # the imaginary channel's shapes
    (204, 4096, 2, 1, GENERATIONS),      # two peaks
    (204, 4096, 3, 2, GENERATIONS),      # three: S * D = 2652 is past the single-workgroup tail, 51 select workgroups
]
STRIDED = (262144 + 5, 64, 1, 5, 3)      # the select kernel's workgroups stride over the swarm (seed 5: see below)
STRIDED_CPU_N = 8                        # (a shorter grid for the oracle's sake; the GPU case runs N = 64)
# the fits of the device batches: (kind, S, N, Y, seed)
BATCH_FITS = [
    ("corner", 8, 96, 0.0, 1), ("corner", 9, 700, 0.25, 2), ("flat", 100, 2048, 0.0, 1), ("corner", 204, 4096, 0.25, 1),
    ("corner", 100, 96, 0.0, 2), ("flat", 9, 4096, 0.25, 1), ("corner", 204, 700, 0.0, 2),
]
BATCH_FITS_EQUAL = [      # one grid length and one swarm size: the batch allows the workgroup geometry
    ("corner", 204, 4096, 0.0, 1), ("corner", 204, 4096, 0.25, 2), ("flat", 204, 4096, 0.0, 1), ("corner", 204, 4096, 0.25, 1),
    ("corner", 204, 4096, 0.0, 2), ("flat", 204, 4096, 0.25, 2), ("corner", 204, 4096, 0.25, 3),
]


def batch_problem(kind, N, Y, fit_im=False):
    if kind == "flat":
        return flat_problem(N, 1, Y)
    return corner_problem(N, 1, Y, fit_im=fit_im)

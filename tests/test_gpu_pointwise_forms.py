"""
GPU tier: the objective kernel's two per-particle form switches, held to the high-precision truth one grid point at a
time (tests/hp_truth.py; the one-hot probe of tests/test_gpu_pointwise.py).

The prologue (objective_prologue.h StagePeakConstants) decides once per particle whether every Lorentzian group takes the
two-operation pair form with batch inversion (fast_all) and whether every Gaussian that touches a full chunk of a
uniform grid is evaluated by recurrence from the lane's first row (rec_all).  One peak decides for the whole particle.
hp_truth.kernel_forms mirrors the two predicates in Python; every particle here is ASSERTED to be in its intended
class, with margin, before anything is launched, so a probe that passes is known to have read the form it was built for.

    classes        pair form + recurrence, pair form alone, general form + recurrence, general form alone, and the pair
                   form refused by the exponent budget alone (one amplitude of 2^-320, or eight of 2^44) with the recurrence on
    rows           all eight rows of a lane (a point is row * 64 + lane) at lanes 0, 31, 63, in a full chunk that is
                   first in its block, one that is second, and the ragged tail chunk
    peak counts    0 to 9, 12, 15, 16, 17, 33 at every probe; 64, 65, 130 at one probe per row
    Gaussians      centred in row 0, in row 7 (t0 furthest from the centre), mid-chunk, three widths outside the chunk
                   and with a window that misses the chunk by 1e-6 relative
    tolerance      the plain bound everywhere, except where the recurrence runs -- the mirror says so, the variant has
                   it, the launch is an objective launch and the chunk is full: there hp_truth's recurrence term is added

The launch forms (one wave per particle, the four- and eight-wave workgroups, per-block sums with finalize_kernel) are
tied to the probed one per class by bit-identity; the swarm step and the device batch are read through their fx in
boxes ("fine", "fine_neg") whose particles take the recurrence.

Each test prints its worst err/tol ratio (recorded in profiles/r07/pointwise_forms.txt).
"""
import math

import numpy as np
import pytest

from nmrfit_amd import _cabi
from nmrfit_amd.equations import Evaluator
from tests import hp_truth as hp
from tests.test_gpu_pointwise import (KGW, MODES, PHASES, REC_VARIANTS, check_objective, check_state, hostile_box,
                                      make_grid, variants_modes)

pytestmark = pytest.mark.gpu

# class -> (pair form, recurrence) on a uniform grid; on a non-uniform grid the recurrence is off in every class
CLASSES = {"pair_rec": (True, True), "pair": (True, False), "general_rec": (False, True), "general": (False, False),
           "budget_rec": (False, True)}
GRIDS = {"uniform1101": ("uniform", 1101), "descending1101": ("descending", 1101), "uniform8781": ("uniform", 8781),
         "nonuniform1101": ("nonuniform", 1101)}
P_ALL = tuple(range(10)) + (12, 15, 16, 17, 33)        # every probe of the chunk
P_ROW = (64, 65, 130)                                  # one probe per row
LANES = (0, 31, 63)
D_REC, D_NOREC = 1.5, 3.0                              # margins of the recurrence's |d| <= 2
E_IN, E_OUT = 200, 300                                 # margins of the exponent budget's 250


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    assert _cabi.device_count() >= 1


def chunk_kinds(N):
    """{kind: chunk index}: a full chunk that is first in its phase block, one that is second (where blocks have two
    chunks), and the ragged tail chunk."""
    bl = hp.block_len(N) // hp.CHUNK
    n_full = N // hp.CHUNK
    mid = (n_full // 2) // bl * bl
    kinds = {"first": mid}
    if bl > 1:
        assert mid + 1 < n_full
        kinds["second"] = mid + 1
    if N % hp.CHUNK:
        kinds["tail"] = n_full
    return kinds


def cases():
    for g, (_, N) in GRIDS.items():
        for kind in chunk_kinds(N):
            for cls in CLASSES:
                yield g, kind, cls


def probes_of(N, c):
    """[(row, j)] of chunk c: every row at lanes 0, 31, 63 (the tail chunk: the points it has)."""
    out = []
    for q in range(hp.ROWS):
        for lane in LANES:
            j = c * hp.CHUNK + q * hp.WAVE + lane
            if j < N:
                out.append((q, j))
    if N - c * hp.CHUNK < hp.CHUNK:
        out.append(((N - 1 - c * hp.CHUNK) // hp.WAVE, N - 1))
    return out


def one_per_row(probes):
    """One probe of every row, the lane varying with the row."""
    rows = {}
    for q, j in probes:
        rows.setdefault(q, []).append(j)
    return {js[q % len(js)] for q, js in rows.items()}


def centre(w, c, place, width, side):
    """Where a Gaussian of the given width sits relative to chunk c (see the module docstring)."""
    N = w.size
    j0 = c * hp.CHUNK
    h = float(w[-1] - w[0]) / (N - 1)
    seg = w[j0:j0 + hp.CHUNK]
    lo, hi = float(seg.min()), float(seg.max())
    if place < 3:               # in the chunk's first row, in its last row (row 7 of a full chunk), in its middle
        n = seg.size
        return float(w[j0]) + (32.3, n - 31.7, 0.5 * n + 0.3)[place] * h
    dist = 3.0 * width if place == 3 else KGW * width * (1 + 1e-6)
    return hi + dist if side else lo - dist


def deciding_peak(P, s):
    """Index of the one peak that decides for the particle: first group, last group (of the last pass), and the second
    pass of 64 where there is one (else a group in between)."""
    return (0, P - 1, 64 + (P - 64) // 2 if P > 64 else P // 2)[(P + s) % 3]


def particles_per_count(P):
    """Small P: enough particles for every placement of the centre; P >= 16: two, so that the deciding peak moves."""
    return 1 if P == 0 else 2 if P >= 16 else max(1, -(-5 // P))


def class_particles(w, c, cls, P, seed=0, with_places=False):
    """X[n, 4 + 3P]: particles of one class built around chunk c (and, on request, every peak's placement: centre())."""
    rng = np.random.default_rng(1000 * P + c + seed)
    N = w.size
    hs = abs(float(w[-1] - w[0])) / (N - 1)
    pair, rec = CLASSES[cls]
    X, places = [], []
    for s in range(particles_per_count(P)):
        special = deciding_peak(P, s) if P else -1
        r = rng.uniform(0.2, 0.9)
        peaks, pl = [], []
        for k in range(P):
            steps = math.exp(rng.uniform(math.log(86.0), math.log(400.0)))
            place = (k + s) % 5
            if not rec and k == special:
                steps, place = rng.uniform(8.0, 20.0), (k + s) % 3
            width = steps * hs
            jitter = rng.uniform(-3.0, 3.0) * hs                # (drawn for every peak; the window's edge takes none)
            loc = centre(w, c, place, width, (k + s) % 2) + (jitter if place != 4 else 0.0)
            peaks.append([width, loc, rng.uniform(0.5, 1.5)])
            pl.append(place)
        if cls == "budget_rec" and P >= 8 and (P + s) % 2:
            # the budget's lower side: eight amplitudes of 2^44 take a group's sum of ilogb(1/al) below -300
            # (fewer peaks would need 2^50 to 2^350 each, outside the mixed-precision kernel's fp32 domain: DESIGN.md)
            for pk in peaks:
                pk[2] *= 2.0 ** 43.75
        elif cls == "budget_rec":
            # the upper side: ONE positive amplitude of 2^-320 -- that peak's 1/al alone takes its group's sum past +300,
            # and the whole particle, every other line of it as usual, leaves the pair form
            peaks[special][2] *= 2.0 ** -320
        if not pair and cls != "budget_rec":
            if (P + s) % 2 == 0:
                peaks[special][2] = -peaks[special][2]
            else:
                r = 0.0
        p0, p1 = PHASES[(P + s) % len(PHASES)]
        X.append(np.concatenate([[p0, p1, r, rng.uniform(-1e-3, 1e-3)], np.ravel(peaks)]))
        places.append(pl)
    return (np.stack(X), places) if with_places else np.stack(X)


def assert_placements(x, places, w, c):
    """Every Gaussian sits where the module docstring says: the windows (3.97 widths) of placements 0 to 3 cross the
    chunk's [lo, hi]; placement 4 misses it by between 0 and 2e-6 of the window's half-length."""
    seg = w[c * hp.CHUNK:(c + 1) * hp.CHUNK]
    lo, hi = float(seg.min()), float(seg.max())
    for k, place in enumerate(places):
        width, loc = abs(float(x[4 + 3 * k])), float(x[5 + 3 * k])
        half = KGW * width
        gap = max(lo - (loc + half), (loc - half) - hi)          # > 0: the window misses the chunk
        if place == 4:
            assert 0.0 < gap <= 2e-6 * half, (k, place, gap / half)
        else:
            assert gap < 0.0, (k, place, gap / half)
            if place < 3:
                assert lo <= loc <= hi, (k, place)


def assert_class(x, w, cls, frame):
    """The mirror puts particle x in class cls, with margin (the conditions of the probes that follow)."""
    pair, rec = CLASSES[cls]
    kf = hp.kernel_forms(x, w, frame)
    P = (x.size - 4) // 3
    uniform = frame[2] != 0.0
    assert not kf["edge"], kf
    assert kf["rec"] == (rec and uniform or P == 0), (cls, kf)
    if P and uniform:
        assert kf["d"] <= D_REC if rec else kf["d"] >= D_NOREC, (cls, kf)
    assert kf["fast"] == pair, (cls, kf)
    if pair:
        assert P == 0 or (kf["ehi"] <= E_IN and kf["elo"] >= -E_IN), (cls, kf)
    elif cls == "budget_rec":
        assert kf["sign_ok"] and (kf["ehi"] >= E_OUT or kf["elo"] <= -E_OUT), (cls, kf)
    else:
        assert not kf["sign_ok"], (cls, kf)
    return kf


def counts_of(cls):
    """Peak counts of a class: without a peak nothing can refuse a form."""
    return [P for P in P_ALL + P_ROW if P > 0 or cls == "pair_rec"]


@pytest.mark.parametrize("grid,kind,cls", list(cases()))
def test_form_classes_pointwise(grid, kind, cls):
    w, u, v = make_grid(*GRIDS[grid])
    N = w.size
    frame = hp.grid_analysis(w)
    w0, _, lane_step, grid_dev = frame
    assert (lane_step != 0.0) == (GRIDS[grid][0] != "nonuniform")
    c = chunk_kinds(N)[kind]
    full = (c + 1) * hp.CHUNK <= N
    assert full == (kind != "tail")
    probes = probes_of(N, c)
    assert {q for q, _ in probes} == set(range(hp.ROWS if full else (N - 1 - c * hp.CHUNK) // hp.WAVE + 1))
    # the conditions first: every particle in its class with margin, every row probed at every peak count
    swarms, masks, seen_places, deciders = {}, {}, set(), set()
    for P in counts_of(cls):
        X, places = class_particles(w, c, cls, P, with_places=True)
        kfs = [assert_class(x, w, cls, frame) for x in X]
        for x, pl in zip(X, places):
            assert_placements(x, pl, w, c)
        seen_places.update(p_ for pl in places for p_ in pl)
        deciders.update((P, deciding_peak(P, s_)) for s_ in range(len(X)))
        swarms[P] = X
        masks[P] = [kf["rec"] for kf in kfs]
    assert seen_places == set(range(5))
    # the deciding peak: in the first group, in the last group of the first pass, in the second pass, in the third
    assert {(33, 0), (33, 32), (64, 63), (65, 64), (130, 97), (130, 129)} <= deciders
    seg = w[c * hp.CHUNK:(c + 1) * hp.CHUNK]
    lohi = (float(seg.min()) - w0, float(seg.max()) - w0)
    worst = hp.Worst("forms/%s/%s/%s" % (grid, kind, cls))
    sparse = one_per_row(probes)
    with Evaluator(w, u, v, np.ones(N)) as ev:
        for q, j in probes:
            wt = np.zeros(N)
            wt[j] = 1.0
            ev.set_weights(wt)
            for P, X in swarms.items():
                if P in P_ROW and j not in sparse:
                    continue
                rec = (lane_step, grid_dev, masks[P]) if full and lane_step != 0.0 else None
                check_objective(ev, X, w, u, v, j, worst, lohi, rec=rec)
    fails = worst.report()
    assert not fails, fails[:5]


def threshold_particles(w, c):
    """Particles AT the two predicates' thresholds: either form is legal, both must be right."""
    frame = hp.grid_analysis(w)
    lane_step = abs(frame[2])
    hs = lane_step / hp.WAVE
    out = []
    for f in (1 - 1e-9, 1 + 1e-9):                                  # |d| = 2 (1 -+ 1e-9)
        for r in (0.5, 0.0):
            x = np.array([0.5, 900.0, r, 1e-4, 150 * hs, centre(w, c, 2, 150 * hs, 0), 1.0,
                          lane_step / f, centre(w, c, 0, lane_step, 0), 1.2])
            d = hp.kernel_forms(x, w, frame)["d"]
            assert abs(d - 2.0) < 1e-8 and (d > 2.0) == (f > 1), d
            out.append(x)
    for last in (-32, -33):                                         # the exponent sum at the limit: -249 and -250
        peaks = []
        for k in range(8):
            pk = [100 * hs * (1 + 0.1 * k), centre(w, c, k % 3, 100 * hs, 0), 1.0]
            e0 = hp.kernel_forms(np.array([0.0, 0.0, 0.5, 0.0] + pk), w, frame)["elo"]
            pk[2] = 2.0 ** (e0 - (last if k == 7 else -31))
            peaks.append(pk)
        x = np.concatenate([[0.0, 7.0, 0.5, -1e-4], np.ravel(peaks)])
        kf = hp.kernel_forms(x, w, frame)
        assert kf["sign_ok"] and kf["elo"] == -217 + last and kf["fast"] == (last == -32), kf
        out.append(x)
    # al = the smallest positive double (a r (2/width) / pi rounds to it), beside an ordinary line
    x = np.array([3.0, -640.0, 1.0, 1e-4, 150 * hs, centre(w, c, 2, 150 * hs, 0), 1.0, 2.0 / 3.0, 3.5, 5e-324])
    assert 5e-324 * 1.0 * 3.0 * hp.INV_PI == 5e-324 and hp.kernel_forms(x, w, frame)["edge"]
    out.append(x)
    return out


def test_particles_at_the_thresholds_pointwise():
    w, u, v = make_grid("uniform", 1101)
    N = w.size
    w0, _, lane_step, grid_dev = hp.grid_analysis(w)
    c = chunk_kinds(N)["first"]
    seg = w[c * hp.CHUNK:(c + 1) * hp.CHUNK]
    lohi = (float(seg.min()) - w0, float(seg.max()) - w0)
    worst = hp.Worst("forms/thresholds")
    with Evaluator(w, u, v, np.ones(N)) as ev:
        for q, j in probes_of(N, c):
            wt = np.zeros(N)
            wt[j] = 1.0
            ev.set_weights(wt)
            for x in threshold_particles(w, c):
                check_objective(ev, x[None, :], w, u, v, j, worst, lohi, rec=(lane_step, grid_dev, [True]))
    fails = worst.report()
    assert not fails, fails[:5]


# ---- the launch forms, per class ------------------------------------------------------------------------------------

def launch_form(g, mode):
    if g["segments"] == 1:
        return "direct"
    if g["segments"] == g["waves_per_workgroup"]:
        return {4: "four_wave", 8: "eight_wave"}[g["segments"]]
    return "finalize"


def test_launch_forms_agree_bit_for_bit_per_class():
    """f of every class's particles is bit-identical whether a wave, a four-wave workgroup, an eight-wave workgroup
    (fit_im off) or eight waves and finalize_kernel sum it: the pointwise truth of the small launches holds for all."""
    w, u, v = make_grid("uniform", 4096)
    N = w.size
    frame = hp.grid_analysis(w)
    c = chunk_kinds(N)["first"]
    rows = []
    for cls in CLASSES:
        X = class_particles(w, c, cls, 12, seed=7)
        for x in X:
            assert_class(x, w, cls, frame)
        rows.append(X)
    X = np.concatenate(rows)
    n = X.shape[0]
    sizes = (12, 60, 250, 600, 1200, 1700, 2500, 3500, 5000, 9000, 20000)   # (which form each takes: asked below)
    rng = np.random.default_rng(5)
    wt = rng.uniform(0.5, 1.5, N)
    reached = []
    with Evaluator(w, u, v, wt) as ev:
        for var, mode in variants_modes():
            if var == _cabi.VARIANT_FARFIELD32 and mode is not False:
                continue
            ev.set_variant(var)
            seen = {}
            for S in sizes:
                f = ev.objective_batch(np.resize(X, (S, X.shape[1])), fit_im=mode)
                form = launch_form(ev.last_launch(), mode)
                assert np.isfinite(f[:n]).all()
                seen.setdefault(form, []).append((S, f[:n].copy()))
            want = {"direct", "four_wave", "finalize"}
            if mode is False and var != _cabi.VARIANT_FARFIELD32:
                want.add("eight_wave")
            assert want <= set(seen), (var, mode, sorted(seen))
            for form, fs in seen.items():
                for S, f in fs:
                    np.testing.assert_array_equal(f, seen["direct"][0][1], err_msg=str((var, mode, form, S)))
            reached.append("%s/%s: %s" % (var, mode, ", ".join("%s at S = %s" % (k, "/".join(str(S) for S, _ in fs))
                                                               for k, fs in sorted(seen.items()))))
    print("forms/launch forms: f of %d class particles bit-identical over " % n + "; ".join(reached))


# ---- the swarm step and the device batch ------------------------------------------------------------------------------

def probe_near(w, loc, row):
    """A point of row `row` of the full chunk nearest to loc."""
    N = w.size
    c = min(int(np.argmin(np.abs(w - loc))) // hp.CHUNK, N // hp.CHUNK - 1)
    return c * hp.CHUNK + row * hp.WAVE + int(np.argmin(np.abs(w - loc))) % hp.WAVE


@pytest.mark.parametrize("size", ["S204", "one_wave_per_particle"])
def test_swarm_step_pointwise_fine_lines(size):
    from nmrfit_amd.pso import DeviceSwarm
    w, u, v = make_grid("uniform")
    N = w.size
    rec = hp.grid_analysis(w)[2:]
    worst = hp.Worst("forms/swarm %s" % size)
    for i, (kind, P, mode, var) in enumerate((("fine", 9, False, _cabi.VARIANT_DEFAULT),
                                              ("fine_neg", 12, "sum", _cabi.VARIANT_FARFIELD),
                                              ("fine", 3, True, _cabi.VARIANT_DEFAULT),
                                              ("fine_neg", 5, False, _cabi.VARIANT_FARFIELD),
                                              ("fine", 17, False, _cabi.VARIANT_NOREC))):
        lo, up = hostile_box(w, P, kind, seed=70 + i)
        j = probe_near(w, 0.5 * (lo[5] + up[5]), (3, 5)[i % 2])
        assert (j // hp.CHUNK + 1) * hp.CHUNK <= N and (j % hp.CHUNK) // hp.WAVE in (3, 5)
        wt = np.zeros(N)
        wt[j] = 1.0
        for S in ((204,) if size == "S204" else (4099, 16411, 65537)):
            with Evaluator(w, u, v, wt) as ev:
                ev.set_variant(var)
                ev.set_fit_im(mode)
                sw = DeviceSwarm(ev, lo, up, swarmsize=S, seed=17 + i)
                sw.run(maxiter=2, check_every=1)
                st = sw.state()
                segments = ev.last_launch()["segments"]
                sw.close()
            if size == "S204" or segments == 1:
                break
        assert (segments == 1) == (size != "S204"), (S, segments)
        check_state(st["x"], st["fx"], w, u, v, j, mode, worst, (kind, P, str(mode), var),
                    rec=rec if var in REC_VARIANTS else None, forms=(kind == "fine", True))
    fails = worst.report()
    assert not fails, fails[:5]


@pytest.mark.parametrize("ragged", [False, True])
@pytest.mark.parametrize("mode", MODES)
def test_device_batch_pointwise_fine_lines(ragged, mode):
    from nmrfit_amd.batch import FitBatch
    worst = hp.Worst("forms/batch ragged=%s fit_im=%s" % (ragged, mode))
    specs, lows, ups, probes, kinds = [], [], [], [], []
    for k, (kind, P) in enumerate((("fine", 3), ("fine_neg", 7), ("fine", 12), ("fine_neg", 5))):
        w, u, v = make_grid("uniform", N=(1500 + 613 * k) if ragged else 3600, seed=k)
        lo, up = hostile_box(w, P, kind, seed=80 + k)
        j = probe_near(w, 0.5 * (lo[5] + up[5]), (3, 5)[k % 2])
        assert (j // hp.CHUNK + 1) * hp.CHUNK <= w.size and (j % hp.CHUNK) // hp.WAVE in (3, 5)
        wt = np.zeros(w.size)
        wt[j] = 1.0
        specs.append((w, u, v, wt))
        lows.append(lo)
        ups.append(up)
        probes.append(j)
        kinds.append(kind)
    for variant in ("default", "farfield"):
        # (the workgroup form exists for fits of one length, cut into four or eight segments, without the imaginary channel)
        for geometry in (("workgroup", "wave") if not ragged and mode is False else ("wave",)):
            with FitBatch(specs, lows, ups, swarmsize=96, seeds=[1, 2, 3, 4], variant=variant, fit_im=mode) as b:
                b.set_geometry(geometry)
                assert b.geometry()["mode"] == geometry
                b.run(2, 1)
                states = [b.state(k) for k in range(len(specs))]
            for k, st in enumerate(states):
                w, u, v, _ = specs[k]
                check_state(st["x"], st["fx"], w, u, v, probes[k], mode, worst, (variant, geometry, k), n=12,
                            rec=hp.grid_analysis(w)[2:], forms=(kinds[k] == "fine", True))
    fails = worst.report()
    assert not fails, fails[:5]

"""
GPU tier of the error weights built on the device (utils.compute_weights_many, FitBatch(regions=...),
fit_many(device_weights=True); csrc/weights.hip).  The contract is bit identity: every spectrum's weights equal the host
routine utils.compute_weights (pinned to the reference by tests/golden/weights.npz) and the reference's per-peak loop
(oracle.nmrfit_oracle.compute_weights) under np.array_equal, alone or in any batch, and every region's (first, last)
index pair equals numpy's argmin pair.
"""
import ctypes

import numpy as np
import pytest

from nmrfit_amd import _cabi, synth, utils
from oracle import nmrfit_oracle as onp

pytestmark = pytest.mark.gpu

T = utils.WEIGHTS_TILE


class Pk:
    def __init__(self, b0, b1, height=1.0):
        self.bounds = [b0, b1]
        self.height = height


def host_pairs(w, peaks):
    """numpy's index pairs, region by region (the reference's lIdx / rIdx, utils.py:205-211)."""
    grid = np.asarray(w, dtype=float)
    out = np.empty((len(peaks), 2), dtype=np.int64)
    for r, pk in enumerate(peaks):
        i0, i1 = (int(np.argmin(np.abs(grid - b))) for b in pk.bounds)
        out[r] = (min(i0, i1), max(i0, i1))
    return out


def truths(w, peaks, expon):
    """(host, per-peak loop): the two truths; the loop needs a peak (np.amax of nothing raises), none is all ones."""
    with np.errstate(divide="ignore", invalid="ignore"):
        host = utils.compute_weights(w, peaks, expon)
        loop = onp.compute_weights(np.asarray(w), peaks, expon) if len(peaks) else np.ones(len(w))
    return host, loop


def edge_cases():
    """name -> (w, peaks, expon).  Grids of halves keep every midpoint and difference exact."""
    g = np.arange(40) / 2.0                      # 0, 0.5, ..., 19.5
    rng = np.random.default_rng(5)
    nan_w = g.copy()
    nan_w[7] = np.nan
    cases = {
        "overlap_nested_last": (g, [Pk(2, 10, 1), Pk(6, 14, 2), Pk(7, 9, 4)], 0.5),
        "overlap_nested_first": (g, [Pk(7, 9, 4), Pk(2, 10, 1), Pk(6, 14, 2)], 0.5),
        "reversed_bounds": (g, [Pk(12, 3, 1), Pk(15, 14.5, 3)], 0.5),
        "left_right_of_grid": (g, [Pk(-5, -2, 2), Pk(30, 40, 3), Pk(4, 6, 1)], 0.5),
        "covers_everything": (g, [Pk(4, 6, 3), Pk(-1, 100, 2), Pk(9, 11, 1)], 0.5),
        "midway_first_on_ties": (g, [Pk(3.25, 8.75, 2), Pk(12.25, 12.25, 1)], 0.5),
        "b0_equals_b1": (g, [Pk(5.0, 5.0, 2), Pk(10, 12, 1)], 0.5),
        "descending": (g[::-1], [Pk(2, 10, 1), Pk(6.25, 14, 2)], 0.5),
        "permuted": (rng.permutation(g), [Pk(2, 10, 1), Pk(6.25, 14, 2), Pk(0, 19.5, 3)], 0.5),
        "duplicates": (np.repeat(np.arange(14) / 2.0, 3), [Pk(1, 3, 1), Pk(2.25, 5, 2), Pk(6.5, 6.5, 4)], 0.5),
        "duplicates_descending": (np.repeat(np.arange(14) / 2.0, 3)[::-1], [Pk(1, 3, 1), Pk(2.25, 5, 2)], 0.5),
        "zero_height": (g, [Pk(2, 6, 1), Pk(10, 12, 0.0), Pk(15, 16, 2)], 0.5),
        "negative_height": (g, [Pk(2, 6, -3), Pk(10, 12, 1), Pk(11, 16, -0.5)], 0.5),
        "expon_0": (g, [Pk(2, 10, 1), Pk(6, 14, 2)], 0.0),
        "expon_2": (g, [Pk(2, 10, 1), Pk(6, 14, 2), Pk(16, 18, 5)], 2.0),
        "no_regions": (g, [], 0.5),
        "nan_in_w": (nan_w, [Pk(2, 10, 1), Pk(12, 14, 2)], 0.5),
        "nan_bound": (g, [Pk(np.nan, 10, 1), Pk(12, 14, 2)], 0.5),
        "inf_bounds": (g, [Pk(-np.inf, 5, 2), Pk(12, np.inf, 3), Pk(-np.inf, np.inf, 1), Pk(8, 9, 4)], 0.5),
        "float32_w": (g.astype(np.float32), [Pk(3.25, 8.75, 2), Pk(12, 15, 1)], 0.5),
    }
    for n in (1, 2, 3, 4):
        cases["N_%d" % n] = (np.arange(n) / 2.0, [Pk(-1, 0.5, 2), Pk(0.25, 9, 1)], 0.5)
    return cases


@pytest.fixture(scope="module")
def edge_table():
    """The cases with their truths, and the device's answer for all of them as ONE ragged call."""
    cases = edge_cases()
    names = list(cases)
    with np.errstate(divide="ignore"):          # (the zero height's level)
        got, pairs = utils.compute_weights_many([cases[n][0] for n in names], [cases[n][1] for n in names],
                                                expon=[cases[n][2] for n in names], return_pairs=True)
    return {n: dict(w=cases[n][0], peaks=cases[n][1], expon=cases[n][2], truth=truths(*cases[n]),
                    pairs=host_pairs(cases[n][0], cases[n][1]), got=got[k], got_pairs=pairs[k])
            for k, n in enumerate(names)}


@pytest.mark.parametrize("name", list(edge_cases()))
def test_edge_table_in_a_ragged_batch_and_alone(edge_table, name):
    c = edge_table[name]
    host, loop = c["truth"]
    nan = name == "zero_height"          # (its level is inf; the only case compared with equal_nan)
    assert np.array_equal(host, loop, equal_nan=nan), "the two truths differ"
    assert c["got"].dtype == np.float64 and c["got"].shape == host.shape
    assert np.array_equal(c["got"], host, equal_nan=nan)
    assert np.array_equal(c["got"], loop, equal_nan=nan)
    assert np.array_equal(c["got_pairs"], c["pairs"])
    with np.errstate(divide="ignore"):
        alone, alone_pairs = utils.compute_weights_many([c["w"]], [c["peaks"]], expon=c["expon"], return_pairs=True)
    assert np.array_equal(alone[0], c["got"], equal_nan=nan)
    assert np.array_equal(alone_pairs[0], c["pairs"])


def tile_case(N):
    """Integer grid of N points; a step between two levels at every offset -11 ... +11 around every tile boundary, around
    both ends, and one region that spans two boundaries (first in the list: the others lie on top of it)."""
    w = np.arange(N, dtype=float)
    peaks = [Pk(T - 5, 2 * T + 5, 3.0)]
    marks = [0, N - 1] + list(range(T, N + 12, T))
    for m, B in enumerate(marks):
        for off in range(-11, 12):
            peaks.append(Pk(B + off - 3, B + off, 1.0 + ((off + 11 + 5 * m) % 7)))
    return w, peaks


TILE_LENGTHS = [21, 22, T - 1, T, T + 1, T + 9, T + 10, T + 11, 2 * T + 1, 3 * T + 5]


@pytest.fixture(scope="module")
def tile_table():
    cases = [tile_case(N) for N in TILE_LENGTHS]
    got, pairs = utils.compute_weights_many([c[0] for c in cases], [c[1] for c in cases], return_pairs=True)
    return {N: dict(w=c[0], peaks=c[1], truth=truths(c[0], c[1], 0.5), pairs=host_pairs(c[0], c[1]), got=got[k],
                    got_pairs=pairs[k]) for k, (N, c) in enumerate(zip(TILE_LENGTHS, cases))}


@pytest.mark.parametrize("N", TILE_LENGTHS)
def test_tile_edges(tile_table, N):
    c = tile_table[N]
    host, loop = c["truth"]
    assert np.array_equal(host, loop)
    assert len(np.unique(host)) > 20          # (the steps are there to be smoothed)
    assert np.array_equal(c["got"], host) and np.array_equal(c["got"], loop)
    assert np.array_equal(c["got_pairs"], c["pairs"])
    alone = utils.compute_weights_many([c["w"]], [c["peaks"]])
    assert np.array_equal(alone[0], host)


def batch_jobs():
    jobs = []
    for k, (N, P) in enumerate([(512, 2), (700, 3), (1024, 2)]):
        sp = synth.make_spectrum(N, P, seed=70 + k)
        jobs.append(dict(data=synth.SynthData(sp["w"], sp["u"], sp["v"], sp["peaks"]), lower=list(sp["lower"]),
                         upper=list(sp["upper"]), options={"seed": 400 + k, "swarmsize": 32, "maxiter": 5}))
    jobs[1]["dynamic_weighting"] = False
    return jobs


def test_fitbatch_from_regions_equals_fitbatch_from_host_weights():
    from nmrfit_amd.batch import FitBatch
    jobs = batch_jobs()
    datas = [j["data"] for j in jobs]
    weights = [utils.compute_weights(d.w, d.peaks) for d in datas]
    weights[1] = np.ones_like(weights[1])
    regions = [utils.weight_regions(d.w, d.peaks) for d in datas]
    regions[1] = None
    kw = dict(swarmsize=32, seeds=[400, 401, 402])
    lowers, uppers = [j["lower"] for j in jobs], [j["upper"] for j in jobs]
    with FitBatch([(d.w, d.u, d.v, wt) for d, wt in zip(datas, weights)], lowers, uppers, **kw) as a:
        a.run(5, 5)
        best_a, status_a = a.best(), a.status()
    with FitBatch([(d.w, d.u, d.v) for d in datas[:2]] + [(datas[2].w, datas[2].u, datas[2].v, None)], lowers, uppers,
                  regions=regions, **kw) as b:
        b.run(5, 5)
        best_b, status_b = b.best(), b.status()
    assert status_a == status_b
    for (xa, fa), (xb, fb) in zip(best_a, best_b):
        assert np.array_equal(xa, xb) and fa == fb
    with pytest.raises(ValueError):          # all or nothing: a weights array next to regions
        FitBatch([(d.w, d.u, d.v, wt) for d, wt in zip(datas, weights)], lowers, uppers, regions=regions, **kw)


def test_regions_are_offset_per_part_of_a_batch():
    """Seven fits: the batch runs as two parts on two streams (three and four fits), each with its own share of the region
    tables; peak counts 1 ... 3 and one fit without regions, so a wrong offset lands on another fit's bounds."""
    from nmrfit_amd.batch import FitBatch
    sps = [synth.make_spectrum(256 + 64 * k, 1 + k % 3, seed=90 + k) for k in range(7)]
    weights = [utils.compute_weights(sp["w"], sp["peaks"]) for sp in sps]
    weights[4] = np.ones_like(weights[4])
    regions = [utils.weight_regions(sp["w"], sp["peaks"]) for sp in sps]
    regions[4] = None
    kw = dict(swarmsize=16, seeds=list(range(7)))
    lowers, uppers = [sp["lower"] for sp in sps], [sp["upper"] for sp in sps]
    with FitBatch([(sp["w"], sp["u"], sp["v"], wt) for sp, wt in zip(sps, weights)], lowers, uppers, **kw) as a:
        a.run(3, 3)
        best_a = a.best()
    with FitBatch([(sp["w"], sp["u"], sp["v"]) for sp in sps], lowers, uppers, regions=regions, **kw) as b:
        b.run(3, 3)
        best_b = b.best()
    for (xa, fa), (xb, fb) in zip(best_a, best_b):
        assert np.array_equal(xa, xb) and fa == fb


def test_fit_many_with_device_weights_equals_fit_many():
    import nmrfit_amd
    plain = nmrfit_amd.fit_many(batch_jobs(), generate=True)
    flagged = nmrfit_amd.fit_many(batch_jobs(), device_weights=True, generate=True)
    for k, (a, b) in enumerate(zip(flagged, plain)):
        assert np.array_equal(a.params, b.params) and a.error == b.error, k
        assert "weights" not in a.__dict__          # (not computed for the batch ...)
        assert np.array_equal(a.weights, b.weights)      # (... made by the host routine on first access)
        assert "weights" in a.__dict__
        assert len(a.real_contribs) == len(a.data.peaks) and a.V.shape == a.data.w.shape      # generate=True
        assert np.array_equal(a.V, b.V) and np.array_equal(a.real_contribs, b.real_contribs)
    assert np.array_equal(flagged[1].weights, np.ones(700))          # dynamic_weighting=False


def test_invalid_arguments_are_refused_before_any_device_work():
    L = _cabi.lib()
    p = _cabi.ptr
    sp = synth.make_spectrum(64, 1, seed=3)
    w, u, v = sp["w"], sp["u"], sp["v"]
    N, R, P = np.array([64], dtype=np.int64), np.array([1], dtype=np.int32), np.array([1], dtype=np.int32)
    edges, level = np.array([3.2, 3.6]), np.array([1.0])
    lower, upper = _cabi.f64(sp["lower"]), _cabi.f64(sp["upper"])
    swarm = np.array([8], dtype=np.int64)
    prm = (_cabi.PsoParams * 1)(_cabi.PsoParams(0.5, 0.5, 0.5, 1e-8, 1e-8, 1))
    out = np.empty(64)
    zero_N, bad_R = np.array([0], dtype=np.int64), np.array([-1], dtype=np.int32)

    def build(S=1, N=N, w=w, R=R, edges=edges, level=level, out=out):
        return L.nmrfit_weights_build(0, S, p(N), p(w), p(R), p(edges), p(level), p(out), None)

    h = ctypes.c_void_p()

    def create(K=1, N=N, w=w, u=u, v=v, R=R, edges=edges, level=level, P=P, lower=lower, upper=upper, swarm=swarm,
               prm=prm, ref=ctypes.byref(h)):
        return L.nmrfit_batch_create_regions(0, K, p(N), p(w), p(u), p(v), p(R), p(edges), p(level), p(P), p(lower),
                                             p(upper), p(swarm), prm, 0, 0, ref)

    bad = [build(S=0), build(S=-1), build(N=None), build(w=None), build(R=None), build(edges=None), build(level=None),
           build(out=None), build(N=zero_N), build(R=bad_R),
           create(K=0), create(N=None), create(w=None), create(u=None), create(v=None), create(R=None), create(edges=None),
           create(level=None), create(P=None), create(lower=None), create(upper=None), create(swarm=None), create(prm=None),
           create(ref=None), create(N=zero_N), create(R=bad_R)]
    assert bad == [_cabi.E_INVALID] * len(bad)
    assert not h.value
    # the limits of a call: NMRFIT_E_UNSUPPORTED (nothing is read past the lengths)
    long_N = np.array([_cabi.WEIGHTS_MAX_POINTS + 1], dtype=np.int64)
    assert build(N=long_N, R=np.zeros(1, dtype=np.int32)) == _cabi.E_UNSUPPORTED
    many = 65536
    assert L.nmrfit_weights_build(0, many, p(np.ones(many, dtype=np.int64)), p(np.zeros(many)), p(np.zeros(many, dtype=np.int32)),
                                  None, None, p(np.zeros(many)), None) == _cabi.E_UNSUPPORTED
    # ... and a normal call afterwards succeeds
    assert build() == _cabi.OK
    assert np.array_equal(out, utils.compute_weights(w, [Pk(3.2, 3.6)]))
    assert create() == _cabi.OK and h.value
    assert L.nmrfit_batch_destroy(h) == _cabi.OK

"""
CPU tier of the device-built error weights: the preparation header (include/nmrfit_amd_prep.h) against its ctypes table
and the built library, the host half of the weights (utils.weight_regions, utils.pack_regions), the lazy
FitUtility.weights, and what fit_many(device_weights=True) hands to a device batch -- all without a GPU.
"""
import ctypes
import os
import re

import numpy as np
import pytest

from nmrfit_amd import _cabi, core, synth, utils

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared(header):
    text = open(os.path.join(ROOT, "include", header)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return set(re.findall(r"\b(nmrfit_[a-z0-9_]+)\s*\(", text))


def test_prep_header_has_its_own_ctypes_table():
    names = declared("nmrfit_amd_prep.h")
    assert names == set(_cabi.PREP_SIGNATURES) == {"nmrfit_weights_build", "nmrfit_batch_create_regions"}
    for table in (_cabi.ALL_SIGNATURES, _cabi.SIGNATURES, _cabi.DIAG_SIGNATURES):
        assert not names & set(table)
    assert not names & (declared("nmrfit_amd.h") | declared("nmrfit_amd_diag.h"))
    if not os.path.exists(_cabi.LIB_PATH):
        _cabi.build()
    L = ctypes.CDLL(_cabi.LIB_PATH)
    for n in names:
        assert hasattr(L, n), "libnmrfit_amd.so does not export " + n
    for n in names:          # ... and lib() has applied the table
        assert getattr(_cabi.lib(), n).argtypes == _cabi.PREP_SIGNATURES[n]
    assert _cabi.lib().nmrfit_abi_version() == _cabi.ABI_VERSION == 6


def test_the_tile_length_is_the_headers():
    text = open(os.path.join(ROOT, "include", "nmrfit_amd_prep.h")).read()
    assert int(re.search(r"#define NMRFIT_WEIGHTS_TILE (\d+)", text).group(1)) == utils.WEIGHTS_TILE


def test_weight_regions_levels_are_the_scalar_powers():
    sp = synth.make_spectrum(512, 5, seed=4)
    peaks = sp["peaks"]
    peaks[2].height = -peaks[2].height
    heights = [abs(pk.height) for pk in peaks]
    for expon in (0.0, 0.5, 0.37, 2.0):
        edges, level = utils.weight_regions(sp["w"], peaks, expon)
        assert edges.shape == (5, 2) and edges.dtype == np.float64 and level.shape == (5,)
        assert np.array_equal(edges, [pk.bounds for pk in peaks])
        want = [np.power(np.amax(heights) / h, expon) for h in heights]
        assert [x.hex() for x in level] == [float(x).hex() for x in want]
    edges, level = utils.weight_regions(sp["w"], [])
    assert edges.shape == (0, 2) and level.shape == (0,)


def test_pack_regions_offsets():
    a = (np.array([[1.0, 2.0], [3.0, 4.0]]), np.array([1.5, 2.5]))
    b = (np.empty((0, 2)), np.empty(0))
    c = ([[9.0, 8.0]], [7.0])
    R, edges, level = utils.pack_regions([a, None, b, c])
    assert R.dtype == np.int32 and R.tolist() == [2, 0, 0, 1]
    assert edges.dtype == np.float64 and edges.tolist() == [1.0, 2.0, 3.0, 4.0, 9.0, 8.0]
    assert level.tolist() == [1.5, 2.5, 7.0]
    with pytest.raises(ValueError):
        utils.pack_regions([(np.zeros((2, 2)), np.zeros(3))])


def jobs_of(shapes, **extra):
    jobs = []
    for k, (N, P) in enumerate(shapes):
        sp = synth.make_spectrum(N, P, seed=20 + k)
        jobs.append(dict(data=synth.SynthData(sp["w"], sp["u"], sp["v"], sp["peaks"]), lower=list(sp["lower"]),
                         upper=list(sp["upper"]), options={"seed": k + 1, "swarmsize": 16, "maxiter": 3}, **extra))
    return jobs


def test_weights_are_lazy_only_when_never_set():
    job = jobs_of([(256, 2)])[0]
    f = utils.FitUtility(job["data"], job["lower"], job["upper"], summary=False, options=job["options"])
    assert "weights" not in f.__dict__
    plan = f._plan(device_weights=True)
    assert "weights" not in f.__dict__ and len(plan["regions"][1]) == 2
    want = utils.compute_weights(f.data.w, f.data.peaks, f.expon)
    assert np.array_equal(f.weights, want) and f.__dict__["weights"] is f.weights          # made once, then kept
    f.weights = np.full(256, 2.0)                      # a value that was set is never replaced
    assert np.array_equal(f.weights, np.full(256, 2.0))
    f._plan()                                          # the host plan computes them as before
    assert np.array_equal(f.__dict__["weights"], want)
    f._plan(device_weights=True)                       # ... and a device plan leaves them to the first access again
    assert "weights" not in f.__dict__
    g = utils.FitUtility(job["data"], job["lower"], job["upper"], dynamic_weighting=False, summary=False)
    assert g._plan(device_weights=True)["regions"][1].size == 0
    assert np.array_equal(g.weights, np.ones(256))
    with pytest.raises(AttributeError):                # any other missing attribute is still missing
        g.params
    assert not hasattr(g, "error")


def test_device_weights_is_fit_manys_own_argument(monkeypatch):
    """The keyword never reaches FitUtility.__init__, and a span's batch is created from the plans' regions: offsets per
    fit, R = 0 for dynamic_weighting=False, (w, u, v) spectra."""
    import nmrfit_amd.batch as batch_module
    seen = {}
    init = utils.FitUtility.__init__

    def spy_init(self, *args, **kwargs):
        assert "device_weights" not in kwargs
        seen["inits"] = seen.get("inits", 0) + 1
        init(self, *args, **kwargs)

    class Refused(_cabi.NmrfitError):
        pass

    def spy_batch(spectra, lowers, uppers, regions=None, **kw):
        seen["spectra"], seen["regions"] = spectra, regions
        raise Refused(_cabi.E_NO_DEVICE, "no device in this test")

    monkeypatch.setattr(utils.FitUtility, "__init__", spy_init)
    monkeypatch.setattr(batch_module, "FitBatch", spy_batch)
    lone = []
    monkeypatch.setattr(utils.FitUtility, "fit", lambda self, plan=None: lone.append((self, plan)))
    jobs = jobs_of([(256, 2), (300, 3), (256, 1)])
    jobs[1]["dynamic_weighting"] = False
    fits = core.fit_many(jobs, device_weights=True)
    assert seen["inits"] == 3 and len(fits) == 3
    assert all(len(sp) == 3 for sp in seen["spectra"])
    R, edges, level = utils.pack_regions(seen["regions"])
    assert R.tolist() == [2, 0, 1]
    off = np.concatenate(([0], np.cumsum(R)))
    for k, job in enumerate(jobs):
        want = utils.weight_regions(job["data"].w, job["data"].peaks if k != 1 else [])
        assert np.array_equal(edges[2 * off[k]:2 * off[k + 1]], want[0].ravel())
        assert np.array_equal(level[off[k]:off[k + 1]], want[1])
    # the refused batch's fits took today's host path, each with its plan, and their weights are the host's
    assert len(lone) == 3 and all("regions" in plan for _, plan in lone)
    for k, job in enumerate(jobs):
        want = utils.compute_weights(job["data"].w, job["data"].peaks) if k != 1 else np.ones(300)
        assert np.array_equal(fits[k].weights, want)
    # without the flag the plans carry no regions and the spectra their weights
    core.fit_many(jobs_of([(256, 2), (256, 2)]))
    assert seen["regions"] is None and all(len(sp) == 4 for sp in seen["spectra"])


def test_entry_points_refuse_invalid_arguments_without_a_gpu():
    L = _cabi.lib()
    p = _cabi.ptr
    N, R = np.array([8], dtype=np.int64), np.array([1], dtype=np.int32)
    w, out, edges, level = np.arange(8.0), np.empty(8), np.array([1.0, 2.0]), np.array([1.0])
    assert L.nmrfit_weights_build(0, 0, p(N), p(w), p(R), p(edges), p(level), p(out), None) == _cabi.E_INVALID
    assert L.nmrfit_weights_build(0, 1, p(N), None, p(R), p(edges), p(level), p(out), None) == _cabi.E_INVALID
    assert L.nmrfit_weights_build(0, 1, p(np.array([0], dtype=np.int64)), p(w), p(R), p(edges), p(level), p(out), None) == _cabi.E_INVALID
    assert L.nmrfit_weights_build(0, 1, p(N), p(w), p(np.array([-1], dtype=np.int32)), p(edges), p(level), p(out), None) == _cabi.E_INVALID
    assert b"R >= 0" in L.nmrfit_last_error()
    h = ctypes.c_void_p()
    assert L.nmrfit_batch_create_regions(0, 1, p(N), p(w), p(w), p(w), None, p(edges), p(level), None, None, None, None,
                                         None, 0, 0, ctypes.byref(h)) == _cabi.E_INVALID
    assert not h.value
    if _cabi.device_count() == 0:          # valid arguments: no fall-back, the missing device is an error
        assert L.nmrfit_weights_build(0, 1, p(N), p(w), p(R), p(edges), p(level), p(out), None) == _cabi.E_NO_DEVICE
        with pytest.raises(_cabi.NmrfitError):
            utils.compute_weights_many([w], [[]])

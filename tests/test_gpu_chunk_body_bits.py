"""
The objective kernels' chunk body, bit for bit against the commit before its register moves were taken out.

tests/golden/chunk_body_parent_bits.npz holds the inputs and what that commit's library returned for them on an MI355X
(tools/record_chunk_body_bits.py wrote it; the commit's hash is in the file): f of objective launches, residual rows, the
state of a swarm after three fused generations and of three fits run as one device batch.  The cases are the smallest
shapes on which each path of the chunk body runs -- grids of one full chunk, full + ragged, three full + ragged and one
whose blocks are two chunks; 0, 1, 2, 7, 8, 9, 16, 24 and 65 peaks; a uniformly spaced grid (Gaussian recurrence on) and
the same grid perturbed by 1e-3 of its spacing (off); per case five particles: no chunk hit by a Gaussian window, every
chunk hit, one negative amplitude (general Lorentzian form), a group that fails the scaled form's exponent budget, a
peak centred on a chunk boundary; the DEFAULT, NOREC and FARFIELD kernels; fit_im off, True and "sum".

Everything is compared with np.array_equal: the chunk body may lose instructions, never a bit.
"""
import importlib.util
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "chunk_body_parent_bits.npz")


def _recorder():
    spec = importlib.util.spec_from_file_location("record_chunk_body_bits",
                                                  os.path.join(ROOT, "tools", "record_chunk_body_bits.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def computed(golden):
    """Every case once, by the library under test; shared by the tests below and left unchanged."""
    return _recorder().run_cases(golden)


def _keys(golden, prefix):
    keys = sorted(k[len("out/"):] for k in golden if k.startswith("out/" + prefix))
    assert keys, prefix
    return keys


def _compare(golden, computed, prefix):
    bad = []
    for k in _keys(golden, prefix):
        assert k in computed, k
        if not np.array_equal(golden["out/" + k], computed[k]):
            d = np.abs(golden["out/" + k] - computed[k])
            bad.append("%s: %d of %d values differ, by up to %.3g" % (k, int(np.count_nonzero(d)), d.size, float(d.max())))
    assert not bad, "\n".join(bad)


def test_fixture_is_recorded_data_of_the_parent_commit(golden):
    """CPU: the file names the commit it was recorded from, every recorded value is finite, the cases are all there, and
    the oracle's f is finite for every case (an all-NaN case would compare nothing)."""
    rec = _recorder()
    commit = str(golden["parent_commit"])
    assert len(commit) == 40 and set(commit) <= set("0123456789abcdef"), commit
    n_f = len(rec.GRID_N) * len(rec.SPACINGS) * len(rec.VARIANTS) * len(rec.PEAKS)
    assert len(_keys(golden, "f/")) == n_f
    assert len(_keys(golden, "f_im/")) == len(rec.FIT_IM) * len(rec.VARIANTS)
    assert len(_keys(golden, "rows/")) == len(rec.ROWS) and len(_keys(golden, "rows_im/")) == len(rec.ROWS_IM)
    assert len(_keys(golden, "swarm/")) == 5 and len(_keys(golden, "batch/")) == 2 * 3 * 5
    for k, a in golden.items():
        if k.startswith("out/"):
            assert np.all(np.isfinite(a)), k
    for k in _keys(golden, "f/"):
        assert golden["out/" + k].shape == (rec.S,), k
    rec.check_inputs(golden)
    assert os.path.getsize(GOLDEN) < 512 * 1024


@pytest.mark.gpu
def test_objective_values_are_the_parents_bits(golden, computed):
    _compare(golden, computed, "f/")


@pytest.mark.gpu
def test_objective_values_with_the_imaginary_channel_are_the_parents_bits(golden, computed):
    _compare(golden, computed, "f_im/")


@pytest.mark.gpu
def test_residual_rows_are_the_parents_bits(golden, computed):
    _compare(golden, computed, "rows/")
    _compare(golden, computed, "rows_f/")
    _compare(golden, computed, "rows_im/")
    _compare(golden, computed, "rows_im_f/")


@pytest.mark.gpu
def test_swarm_state_after_three_fused_generations_is_the_parents(golden, computed):
    _compare(golden, computed, "swarm/")


@pytest.mark.gpu
def test_batched_fits_state_is_the_parents_in_both_geometries(golden, computed):
    _compare(golden, computed, "batch/")

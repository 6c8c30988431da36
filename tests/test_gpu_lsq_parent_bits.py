"""
The least-squares sums of the device, bit for bit against the commit before their kernels were composed of shared stages.

tests/golden/lsq_parent_bits.npz holds what that commit's library returned on an MI355X (tools/record_lsq_bits.py wrote it;
the commit's hash is in the file): J, r, A, g and f of nmrfit_jacobian, the records of nmrfit_sandwich and, in both modes,
of nmrfit_sandwich_im -- each with sigma_v = 2 sigma_u and with sigma_v = sigma_u -- on the smallest shapes on which each
path of the kernels runs: one ragged tile; two segments, the second of one point; 65 tiles, two per segment with a last
segment of one (the only both-channel case anywhere with more than one tile per segment); the smallest D; D = 76 with
every accumulator in use and cross bands of 39 and 38 rows; the smallest grid of the both-channel tests.  Then a ragged
batch through nmrfit_batch_sandwich and nmrfit_batch_sandwich_im, and one whose groups divide under
NMRFIT_LSQ_WORKSPACE_MB=1.  The other tests of these paths compare the library with itself and with numpy to a bound: they
cannot see a change that moves both sides together.  The inputs are regenerated from the seeds the recorder names; arrays
above 32 KiB are compared by the SHA-256 of their bytes.

Everything is compared with np.array_equal: the kernels may change their text, never a bit.
"""
import importlib.util
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "lsq_parent_bits.npz")


def _recorder():
    spec = importlib.util.spec_from_file_location("record_lsq_bits", os.path.join(ROOT, "tools", "record_lsq_bits.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def computed():
    """Every case once, by the library under test; shared by the tests below and left unchanged."""
    rec = _recorder()
    return {k: rec.stored(v) for k, v in rec.run_cases().items()}


def _keys(golden, prefix):
    keys = sorted(k[len("out/"):] for k in golden if k.startswith("out/" + prefix))
    assert keys, prefix
    return keys


def _compare(golden, computed, prefix):
    bad = []
    for k in _keys(golden, prefix):
        assert k in computed, k
        want, got = golden["out/" + k], computed[k]
        assert want.dtype == got.dtype and want.shape == got.shape, k
        if not np.array_equal(want, got):
            if want.dtype.kind == "f":
                d = np.abs(want - got)
                bad.append("%s: %d of %d values differ, by up to %.3g" % (k, int(np.count_nonzero(d)), d.size, float(d.max())))
            else:
                bad.append("%s: the SHA-256 of the array's bytes differs" % k)
    assert not bad, "\n".join(bad)


def test_fixture_is_recorded_data_of_the_parent_commit(golden):
    """CPU: the file names the commit it was recorded from, the cases are all there, every recorded value is finite, a
    large array is kept as its digest, and the inputs this machine regenerates are the ones the record was made from."""
    rec = _recorder()
    commit = str(golden["parent_commit"])
    assert len(commit) == 40 and set(commit) <= set("0123456789abcdef"), commit
    per_shape = 5 + len(rec.RATIOS) * (4 + 4 * len(rec.MODES))
    assert len(_keys(golden, "ctx/")) == len(rec.SHAPES) * per_shape
    per_batch = 4 * (1 + len(rec.MODES)) * len(rec.BUDGETS)
    assert len(_keys(golden, "batch/")) == len(rec.RAGGED) * per_batch
    assert len(_keys(golden, "split/")) == len(rec.SPLIT) * per_batch
    hashed = 0
    for k, a in golden.items():
        if k.startswith("out/"):
            if a.dtype.kind == "f":
                assert np.all(np.isfinite(a)) and a.nbytes <= rec.HASH_ABOVE, k
            else:
                assert len(str(a)) == 64, k
                hashed += 1
    assert hashed and str(golden["out/ctx/4160/2/jacobian/J"]) != str(golden["out/ctx/256/24/jacobian/J"])
    for k, want in rec.input_digests().items():
        assert str(golden[k]) == str(want), k
    assert os.path.getsize(GOLDEN) < 477 * 1024
    # the shapes are what the docstrings say of them
    from nmrfit_amd import _cabi
    assert 4 + 3 * 24 == _cabi.LSQ_MAX_D and -(-4160 // 64) == 65
    for shapes, both in ((rec.RAGGED, 95020), (rec.SPLIT, 2 * (3 * 45760 + 1430))):
        assert 2 * sum((4 + 3 * P + 1) * N for N, P in shapes) == both
    assert 2 * 45760 + 1430 <= (1 << 17) < 3 * 45760 + 1430 and 2 * (45760 + 1430) <= (1 << 17) < 2 * (2 * 45760 + 1430)


@pytest.mark.gpu
def test_jacobian_and_normal_equations_are_the_parents_bits(golden, computed):
    for N, P in _recorder().SHAPES:
        _compare(golden, computed, "ctx/%d/%d/jacobian/" % (N, P))


@pytest.mark.gpu
def test_sandwich_is_the_parents_bits(golden, computed):
    for N, P in _recorder().SHAPES:
        _compare(golden, computed, "ctx/%d/%d/sandwich/" % (N, P))


@pytest.mark.gpu
def test_sandwich_im_is_the_parents_bits_in_both_modes(golden, computed):
    for N, P in _recorder().SHAPES:
        _compare(golden, computed, "ctx/%d/%d/sandwich_im/" % (N, P))


@pytest.mark.gpu
def test_batches_are_the_parents_bits_under_both_workspace_budgets(golden, computed):
    _compare(golden, computed, "batch/")
    _compare(golden, computed, "split/")

"""
GPU tier of the device-side least-squares pieces (csrc/lsq.hip, include/nmrfit_amd_lsq.h): nmrfit_jacobian's J and r bit
for bit against the host construction, A and g within the derived bound of exactly summed truth, the ragged batch against
lone contexts, FitBatch.polish against the per-fit scipy path, fit_many(batch_polish=True), argument validation.
Shapes: N = 512 (one chunk), 700 (ragged tail, no multiple of 64), 4096; P = 1, 2, 24 (D = 76, the kernel's largest).
"""

import numpy as np
import pytest

from nmrfit_amd import _cabi, lsq, synth
from tests import lsq_support as S

pytestmark = pytest.mark.gpu

SHAPES = [(N, P) for N in (512, 700, 4096) for P in (1, 2, 24)]


def _spectrum(N, P):
    return synth.make_spectrum(N, P, seed=100 + N % 97 + P)


def _interior(sp, seed=7):
    return synth.make_swarm(sp["lower"], sp["upper"], 2, seed=seed)[1]


@pytest.mark.parametrize("N, P", SHAPES)
def test_jacobian_bits_and_normal_equations(N, P):
    from nmrfit_amd.equations import Evaluator
    sp = _spectrum(N, P)
    D = 4 + 3 * P
    s = 1.0 / np.sqrt(N)
    with Evaluator(*S.spectrum_tuple(sp)) as ev:
        m = lsq.ResidualModel(ev, sp["lower"], sp["upper"])
        for where, x in (("interior", _interior(sp)), ("upper bound", np.array(sp["upper"], dtype=float))):
            rows, h = m.rows(x)
            c = s / h
            if where == "upper bound":
                assert np.all(c < 0)                       # every step flipped
            R, f = ev.residual_batch(rows, return_f=True)
            J_host = np.ascontiguousarray(((R[1:] - R[0]) * (s / h[:, None])).T)
            r_host = R[0] * s
            out = ev.jacobian(rows, c, s, J=True, r=True, normal=True)
            assert out["J"].shape == (N, D)
            np.testing.assert_array_equal(out["J"], J_host, err_msg=where)
            np.testing.assert_array_equal(out["r"], r_host, err_msg=where)
            assert out["f"] == f[0]
            np.testing.assert_array_equal(m.jac(x), J_host)           # what scipy receives
            A, g = out["A"], out["g"]
            np.testing.assert_array_equal(A, A.T)                      # symmetric as returned
            again = ev.jacobian(rows, c, s, J=True, r=True, normal=True)
            for key in ("J", "r", "A", "g"):
                np.testing.assert_array_equal(again[key], out[key], err_msg="second call: " + key)
            assert again["f"] == out["f"]
            A2, g2, f2 = m.normal_equations(x)                         # sums alone: the same bits
            np.testing.assert_array_equal(A2, A)
            np.testing.assert_array_equal(g2, g)
            assert f2 == out["f"]
            if where == "interior" or D < 76:
                Ax, gx, absA, absg = S.exact_normal_equations(J_host, r_host)
                print("N %d P %d %s: max |A - exact| / bound %.3g, g %.3g" % (
                    N, P, where, np.max(np.abs(A - Ax) / S.sum_bound(N, absA)), np.max(np.abs(g - gx) / S.sum_bound(N, absg))))
                assert np.all(np.abs(A - Ax) <= S.sum_bound(N, absA))
                assert np.all(np.abs(g - gx) <= S.sum_bound(N, absg))
            else:                                                      # (the exact sums of 76 x 77 / 2 entries once per shape)
                np.testing.assert_allclose(A, J_host.T @ J_host, rtol=0, atol=2 * np.max(S.sum_bound(N, np.abs(J_host).T @ np.abs(J_host))))


def test_jacobian_beyond_the_normal_equations_limit():
    """J and r have no limit on D (the existing least-squares path takes any P); A and g are refused beyond D = 76."""
    from nmrfit_amd.equations import Evaluator, NmrfitError
    sp = _spectrum(700, 25)
    s = 1.0 / np.sqrt(700)
    with Evaluator(*S.spectrum_tuple(sp)) as ev:
        m = lsq.ResidualModel(ev, sp["lower"], sp["upper"])
        x = _interior(sp)
        rows, h = m.rows(x)
        R = ev.residual_batch(rows)
        out = ev.jacobian(rows, s / h, s, J=True, r=True)
        np.testing.assert_array_equal(out["J"], np.ascontiguousarray(((R[1:] - R[0]) * (s / h[:, None])).T))
        np.testing.assert_array_equal(out["r"], R[0] * s)
        with pytest.raises(NmrfitError) as ei:
            m.normal_equations(x)
        assert ei.value.code == _cabi.E_UNSUPPORTED
        np.testing.assert_array_equal(m.jac(x), out["J"])             # the context is usable after the refusal


def test_jacobian_through_three_staging_chunks():
    """N = 16384, P = 24: J is 9.96 MB per channel, three 4 MiB chunks of the staged copy to host memory -- the smallest
    size at which a pinned buffer is used a second time -- and the second channel's J lands behind the first's."""
    from nmrfit_amd.equations import Evaluator
    N = 16384
    sp = _spectrum(N, 24)
    s = 1.0 / np.sqrt(N)
    with Evaluator(*S.spectrum_tuple(sp)) as ev:
        rows, h = lsq.ResidualModel(ev, sp["lower"], sp["upper"]).rows(_interior(sp))
        c = s / h
        assert N * len(c) * 8 > 2 * (4 << 20)
        R = ev.residual_batch(rows)
        J = ev.jacobian(rows, c, s, J=True)["J"]
        np.testing.assert_array_equal(J, ((R[1:] - R[0]) * c[:, None]).T)
        R_re, R_im, _ = ev.residual_batch_im(rows, True)
        J2 = ev.jacobian_im(rows, c, s, True, J=True)["J"]
        assert J2.shape == (2, N, len(c))
        np.testing.assert_array_equal(J2[0], ((R_re[1:] - R_re[0]) * c[:, None]).T)
        np.testing.assert_array_equal(J2[1], ((R_im[1:] - R_im[0]) * c[:, None]).T)
        np.testing.assert_array_equal(J2[0], J)


RAGGED = [(512, 1), (700, 2), (4096, 24)]


@pytest.fixture(scope="module")
def ragged():
    """Three fits of different N and P, their points, and each fit's normal equations on a lone context."""
    from nmrfit_amd.equations import Evaluator
    specs = [_spectrum(N, P) for N, P in RAGGED]
    X = [_interior(sp, seed=11 + k) for k, sp in enumerate(specs)]
    X[1] = np.array(specs[1]["upper"], dtype=float)                    # one fit on its upper bound: flipped steps
    lone = []
    for sp, x in zip(specs, X):
        with Evaluator(*S.spectrum_tuple(sp)) as ev:
            lone.append(lsq.ResidualModel(ev, sp["lower"], sp["upper"]).normal_equations(x))
    return specs, X, lone


def _batch(specs, order, **kw):
    from nmrfit_amd.batch import FitBatch
    return FitBatch([S.spectrum_tuple(specs[k]) for k in order], [specs[k]["lower"] for k in order],
                    [specs[k]["upper"] for k in order], swarmsize=8, seeds=list(range(1, len(order) + 1)), **kw)


@pytest.mark.parametrize("order", [(0, 1, 2), (2, 0, 1), (0, 1, 2, 0, 1, 2, 1)])
def test_ragged_batch_equals_lone_contexts_bit_for_bit(ragged, order, monkeypatch):
    """Seven fits are two parts of 3 + 4 (a batch splits from K = 6): the call walks per-part offsets into every array, the
    part boundary lies between fits that differ in N and P, and the fits recur, so that a wrong offset lands on another
    fit's block of another size."""
    specs, X, lone = ragged
    with _batch(specs, order) as fb:
        got = fb.normal_equations([X[k] for k in order])
        for (A, g, f), k in zip(got, order):
            np.testing.assert_array_equal(A, lone[k][0], err_msg="A of fit %d" % k)
            np.testing.assert_array_equal(g, lone[k][1], err_msg="g of fit %d" % k)
            assert f == lone[k][2]
        # a workspace budget of 1 MiB: every fit a group of its own -- not a bit changes
        monkeypatch.setenv("NMRFIT_LSQ_WORKSPACE_MB", "1")
        for (A, g, f), k in zip(fb.normal_equations([X[k] for k in order]), order):
            np.testing.assert_array_equal(A, lone[k][0])
            np.testing.assert_array_equal(g, lone[k][1])
            assert f == lone[k][2]


@pytest.fixture(scope="module")
def five():
    return [synth.make_spectrum(2048, 2 + k % 2, seed=30 + k, physical=True) for k in range(5)]


def test_batch_polish_against_the_per_fit_path(five):
    from nmrfit_amd.batch import FitBatch
    from nmrfit_amd.equations import Evaluator
    from oracle import c_oracle
    specs = five
    with FitBatch([S.spectrum_tuple(sp) for sp in specs], [sp["lower"] for sp in specs], [sp["upper"] for sp in specs],
                  swarmsize=64, seeds=[3 + k for k in range(5)]) as fb:
        fb.run(100, 10)
        start = fb.best()
        # (the budget of the CPU comparison: scipy's own default of 100 D evaluations)
        res = fb.polish(max_launches=100 * max(fb.D))
        info = fb.last_polish
        assert fb.polish(which=[])[0][1] == start[0][1]               # nothing asked for: the swarm's answers
    for k, (sp, (xs, fs), (x, f)) in enumerate(zip(specs, start, res)):
        assert f <= fs, (k, f, fs)
        assert np.all(x >= sp["lower"]) and np.all(x <= sp["upper"])
        ref = c_oracle.objective_batch(x, *S.spectrum_tuple(sp))[0]
        assert f == pytest.approx(ref, rel=1e-9)
        with Evaluator(*S.spectrum_tuple(sp)) as ev:
            xp, fp, _ = lsq.polish(ev, xs, sp["lower"], sp["upper"], **S.TRF_TOL)
        gap = abs(f - fp) / fp
        print("fit %d: swarm %.9g  batch polish %.17g (%s, %d accepted)  per-fit %.17g  relative gap %.3g"
              % (k, fs, f, info["stop"][k], info["accepted"][k], fp, gap))
        assert gap <= S.FINAL_F_BAR, (k, gap, S.FINAL_F_BAR)


def test_fit_many_batch_polish(five):
    import nmrfit_amd
    specs = five + [synth.make_spectrum(2048, 2, seed=36, physical=True)]

    def jobs():
        out = []
        for k, sp in enumerate(specs):
            job = dict(data=synth.SynthData(sp["w"], sp["u"], sp["v"], sp["peaks"]), lower=list(sp["lower"]), upper=list(sp["upper"]),
                       options={"swarmsize": 64, "maxiter": 100, "seed": 3 + k, "polish": k not in (1, 4)})
            out.append(job)
        return out

    def im_jobs():
        return [dict(j, fit_im=True) for j in jobs()[:2]]
    plain = nmrfit_amd.fit_many([dict(j, options=dict(j["options"], polish=False)) for j in jobs()], generate=True)
    base = nmrfit_amd.fit_many(jobs(), generate=True, threads=2)
    many = nmrfit_amd.fit_many(jobs(), generate=True, threads=2, batch_polish=True)
    for k, (a, b, c) in enumerate(zip(plain, base, many)):
        if k in (1, 4):                        # no options['polish']: the keyword changes nothing
            np.testing.assert_array_equal(c.params, b.params)
            assert c.error == b.error
            np.testing.assert_array_equal(c.V, b.V)
            np.testing.assert_array_equal(c.real_contribs, b.real_contribs)
            continue
        assert c.error <= a.error, (k, c.error, a.error)
        assert np.all(c.params >= c.lower) and np.all(c.params <= c.upper)
        lone = nmrfit_amd.utils.FitUtility(jobs()[k]["data"], jobs()[k]["lower"], jobs()[k]["upper"], summary=False)
        lone.params = np.array(c.params)
        lone.generate_result()
        np.testing.assert_array_equal(c.V, lone.V)
        np.testing.assert_array_equal(c.u, lone.u)
        np.testing.assert_array_equal(c.real_contribs, lone.real_contribs)
    # fit_im jobs keep the per-fit path, polish or not
    im_base = nmrfit_amd.fit_many(im_jobs(), generate=True)
    im_many = nmrfit_amd.fit_many(im_jobs(), generate=True, batch_polish=True)
    for b, c in zip(im_base, im_many):
        np.testing.assert_array_equal(c.params, b.params)
        assert c.error == b.error
        np.testing.assert_array_equal(c.V, b.V)


def test_argument_validation(ragged):
    from nmrfit_amd.equations import Evaluator
    specs, X, lone = ragged
    L = _cabi.lib()
    sp, x = specs[0], X[0]
    D = len(x)
    s = 1.0 / np.sqrt(len(sp["w"]))
    with Evaluator(*S.spectrum_tuple(sp)) as ev:
        m = lsq.ResidualModel(ev, sp["lower"], sp["upper"])
        rows, h = m.rows(x)
        c = s / h
        A = np.empty((D, D))
        for args, text in (((ev.handle, 1, None, _cabi.ptr(c)), b"null rows or c"), ((ev.handle, 1, _cabi.ptr(rows), None), b"null rows or c"),
                           ((ev.handle, -1, _cabi.ptr(rows), _cabi.ptr(c)), b"negative"),
                           ((ev.handle, 1 << 20, _cabi.ptr(rows), _cabi.ptr(c)), b"exceeds the supported maximum")):
            assert L.nmrfit_jacobian(*args, s, None, None, _cabi.ptr(A), None, None) == _cabi.E_INVALID
            assert text in L.nmrfit_last_error()
        A2, g2, f2 = m.normal_equations(x)                             # after the refused calls a normal one succeeds
        np.testing.assert_array_equal(A2, lone[0][0])
        # nmrfit_residual_batch: the refusals nmrfit_residual_batch_im is held to (test_gpu_lsq_im.py)
        R0 = ev.residual_batch(rows)
        pr, pR = _cabi.ptr(rows), _cabi.ptr(np.empty_like(R0))
        for args, text in (((ev.handle, D + 1, 1, None, pR), b"null parameter/output pointer"),
                           ((ev.handle, D + 1, 1, pr, None), b"null parameter/output pointer"),
                           ((ev.handle, D + 1, -1, pr, pR), b"negative"), ((ev.handle, -1, 1, pr, pR), b"negative")):
            assert L.nmrfit_residual_batch(*args, None) == _cabi.E_INVALID, args
            assert text in L.nmrfit_last_error()
        np.testing.assert_array_equal(ev.residual_batch(rows), R0)
        # the two copies: a negative size, a null pointer with a positive size, each under its own name
        host = np.arange(8.0)
        dptr = ev.dev_alloc(host.nbytes)
        for fn, name in ((L.nmrfit_memcpy_h2d, b"nmrfit_memcpy_h2d"), (L.nmrfit_memcpy_d2h, b"nmrfit_memcpy_d2h")):
            dst, src = (dptr, _cabi.ptr(host)) if fn is L.nmrfit_memcpy_h2d else (_cabi.ptr(host), dptr)
            for args in ((dst, src, -1), (None, src, 8), (dst, None, 8)):
                assert fn(ev.handle, *args) == _cabi.E_INVALID, (name, args)
                assert L.nmrfit_last_error() == b"bad arguments to " + name
        ev.upload(dptr, host)
        np.testing.assert_array_equal(ev.download(dptr, host.shape), host)
        ev.dev_free(dptr)
        # a variant the library does not hold, and one that does not exist
        if not _cabi.has_ab_variants():
            assert L.nmrfit_ctx_set_variant(ev.handle, _cabi.VARIANT_NOSKIP) == _cabi.E_UNSUPPORTED
            assert b"A/B form" in L.nmrfit_last_error()
            np.testing.assert_array_equal(ev.residual_batch(rows), R0)
        for gone in (-1, 3, 4, 5):            # (3, 4, 5: the numbers of retired A/B forms, in every library)
            assert L.nmrfit_ctx_set_variant(ev.handle, gone) == _cabi.E_INVALID, gone
            assert b"bad context or variant" in L.nmrfit_last_error()
        np.testing.assert_array_equal(ev.residual_batch(rows), R0)
    with _batch(specs, (0, 1, 2)) as fb:
        good = fb.normal_equations(X)
        rows = np.concatenate([lsq.forward_rows(x, q["lower"], q["upper"])[0].ravel() for x, q in zip(X, specs)])
        cs = np.ones(int(fb.offsets[-1]))
        ss = np.ones(3)
        f = np.empty(3)
        for args in ((None, _cabi.ptr(cs), _cabi.ptr(ss)), (_cabi.ptr(rows), None, _cabi.ptr(ss)), (_cabi.ptr(rows), _cabi.ptr(cs), None)):
            assert L.nmrfit_batch_normal_equations(fb._h, *args, None, None, _cabi.ptr(f)) == _cabi.E_INVALID
            assert b"null rows, c or s" in L.nmrfit_last_error()
        with pytest.raises(ValueError):
            fb.normal_equations(X[:2])
        with pytest.raises(ValueError):
            fb.normal_equations([X[0], X[0], X[2]])                    # a vector whose P does not match the fit's
        for (A, g, fk), (A0, g0, f0) in zip(fb.normal_equations(X), good):
            np.testing.assert_array_equal(A, A0)
            assert fk == f0
    # one fit beyond D = 76 in the batch: refused, and the batch goes on fitting
    big = [specs[0], _spectrum(700, 25)]
    with _batch(big, (0, 1)) as fb:
        with pytest.raises(_cabi.NmrfitError) as ei:
            fb.normal_equations([X[0], _interior(big[1])])
        assert ei.value.code == _cabi.E_UNSUPPORTED
        fb.run(3, 1)
        assert len(fb.best()) == 2

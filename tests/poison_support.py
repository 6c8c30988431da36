"""
The case driver of tests/test_gpu_poison.py (NOT part of the nmrfit_amd package): one AREA of the library's device
allocations -- ctx, swarm, batch, prep -- exercised in ONE process,

    python -m tests.poison_support AREA OUT.npz

Every case makes the calls of its rows of the audit table (which piece of which device allocation is
written by whom before whom reads it), asserts each result against the oracle the existing test of that call uses, at
that test's tolerance, and records every output array; the arrays and the list of the cases that ran go to OUT.npz.
tests/test_gpu_poison.py runs the driver three times -- NMRFIT_POISON_ALLOC unset, 255 (every fresh double a NaN) and 63
(every fresh double 4.8e-4, every fresh index 0x3f3f...) -- and holds the three files byte-identical: no result may depend
on what a fresh device block holds.

No case is ever skipped: a case runs or raises.  Host arrays that the library writes into are made by the package's
wrappers with np.empty; in this process np.empty fills with NaN (integers: the type's minimum), so that a copy that came
up short shows in the result.

The oracles: the C oracle and the numpy oracle (oracle/), tests/swarm_support.HostSwarm, noise.replicas_host,
utils.compute_weights, quality.residual_stats_host, the host peak picking and phase paths, and the lone-context twins
of the batch calls.  Where the launch form matters a case asks the plan (tests/launch_plan/plan_query.hip, compiled for
the host) and holds Evaluator.last_launch / DeviceSwarm.last_launches to its answer.
"""
import contextlib
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
AREAS = ("ctx", "swarm", "batch", "prep")
CASES = {area: [] for area in AREAS}          # area -> [(name, function)], in the order they run
FREE = dict(minfunc=-1.0, minstep=-1.0)        # the stopping rule disarmed
STATE = ("x", "v", "p", "fx", "fp")
RTOL_F, F_FLOOR = 1e-9, 1e-6                   # tests/test_gpu_parity.py


def case(area, name):
    def register(fn):
        CASES[area].append((name, fn))
        return fn
    return register


def case_names(area):
    return [name for name, _ in CASES[area]]


def case_ids():
    """Every case as ``area/name``: what the audit table's case column names."""
    return ["%s/%s" % (area, name) for area in AREAS for name in case_names(area)]


class Record:
    """The arrays of one run: ``save`` keeps a copy under ``<case>:<key>``."""

    def __init__(self):
        self.arrays = {}
        self.ran = []
        self._case = None

    def begin(self, name):
        self._case = name
        self.ran.append(name)

    def save(self, key, value):
        full = "%s:%s" % (self._case, key)
        assert full not in self.arrays, full
        self.arrays[full] = np.array(value, copy=True)

    def save_dict(self, key, d):
        for k in sorted(d):
            self.save("%s.%s" % (key, k), d[k])


# ---- np.empty that shows a short copy ----------------------------------------------------------------------------------
_EMPTY, _EMPTY_LIKE = np.empty, np.empty_like


def _fill(a):
    if a.dtype.kind == "f":
        a.fill(np.nan)
    elif a.dtype.kind == "c":
        a.fill(complex(np.nan, np.nan))
    elif a.dtype.kind == "i":
        a.fill(np.iinfo(a.dtype).min)
    elif a.dtype.kind == "u":
        a.fill(np.iinfo(a.dtype).max)
    return a


@contextlib.contextmanager
def nan_outputs():
    np.empty = lambda *a, **k: _fill(_EMPTY(*a, **k))
    np.empty_like = lambda *a, **k: _fill(_EMPTY_LIKE(*a, **k))
    try:
        yield
    finally:
        np.empty, np.empty_like = _EMPTY, _EMPTY_LIKE


@contextlib.contextmanager
def env(**kv):
    old = {k: os.environ.get(k) for k in kv}
    try:
        for k, v in kv.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = str(v)
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


# ---- the plan ----------------------------------------------------------------------------------------------------------
_PLAN = {}


def build_plan_query(exe):
    cc = subprocess.run([HIPCC, "--offload-arch=gfx950", "--cuda-host-only", "-O1", "-std=c++17",
                         "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "nmrfit_amd", "csrc"),
                         os.path.join(ROOT, "tests", "launch_plan", "plan_query.hip"), "-o", exe],
                        capture_output=True, text=True, timeout=300)
    assert cc.returncode == 0, cc.stderr[-3000:]
    return exe


def ask(S, N, P, pair, target, mode, variant=0):
    """plan_objective's answer for this device (NMRFIT_POISON_PLAN_QUERY: a plan_query the caller has built already)."""
    from nmrfit_amd import _cabi
    if "exe" not in _PLAN:
        exe = os.environ.get("NMRFIT_POISON_PLAN_QUERY")
        if not exe:
            _PLAN["dir"] = tempfile.TemporaryDirectory()
            exe = build_plan_query(os.path.join(_PLAN["dir"].name, "plan_query"))
        _PLAN["exe"] = exe
        _PLAN["cus"] = _cabi.device_info(0)["compute_units"]
    args = (_PLAN["cus"], S, N, P, -1 if pair is None else pair, target or 0, variant, mode)
    if args not in _PLAN:
        run = subprocess.run([_PLAN["exe"]] + [str(a) for a in args], capture_output=True, text=True, timeout=60)
        assert run.returncode == 0, run.stderr
        q = dict(kv.split("=") for kv in run.stdout.split())
        q = {k: (v if k == "unit" else int(v)) for k, v in q.items()}
        assert q["code"] == 0 and q["flush"] == 0, q
        _PLAN[args] = q
    return dict(_PLAN[args])


def reached(what, ev, q, **want):
    """The launch ``ev`` made last is the plan's, and the plan's answer is the form the case was built for."""
    for k, v in want.items():
        assert q[k] == v, "%s: the plan gives %s = %r, the case was built for %r (%r)" % (what, k, q[k], v, q)
    g = ev.last_launch()
    assert (g["waves"], g["segments"], g["waves_per_workgroup"]) == (q["waves"], q["nseg"], q["wpb"]), (what, g, q)


# ---- shared pieces -----------------------------------------------------------------------------------------------------
def close_f(f, ref, rtol=RTOL_F, what=""):
    f, ref = np.asarray(f), np.asarray(ref)
    tol = rtol * np.maximum(np.abs(ref), F_FLOOR)
    bad = ~(np.abs(f - ref) <= tol)
    assert not bad.any(), "%s: max rel err %.3g at %s" % (what, np.nanmax(np.abs(f - ref) / np.maximum(np.abs(ref), F_FLOOR)),
                                                         np.nonzero(bad)[0][:5])


def spectrum_tuple(sp):
    return sp["w"], sp["u"], sp["v"], sp["weights"]


def closed_form_fit_im(X, w, u, v, wt):
    """(fit_im=True, fit_im="sum") objective values by numpy + scipy.special.dawsn: tests/test_gpu_kk.py's closed form."""
    from nmrfit_amd import proc_autophase, synth
    from oracle import nmrfit_oracle as onp
    want_ref, want_sum = np.zeros(len(X)), np.zeros(len(X))
    for s, x in enumerate(X):
        P = (len(x) - 4) // 3
        V, I = proc_autophase.ps2(u, v, x[0], x[1])
        Vf = sum(onp.voigt(w, x[2], x[3], *x[4 + 3 * k:7 + 3 * k]) for k in range(P))
        Ik = [synth._dispersion(w, x[2], *x[4 + 3 * k:7 + 3 * k]) for k in range(P)]
        rr = np.sqrt(np.mean((wt * (V - Vf)) ** 2))
        want_ref[s] = 0.5 * (rr + np.sqrt(np.mean((wt * (I - Ik[-1])) ** 2)))
        want_sum[s] = 0.5 * (rr + np.sqrt(np.mean((wt * (I - sum(Ik))) ** 2)))
    return want_ref, want_sum


def snapshot(sw):
    out = dict(sw.state())
    out["best_x"], out["best_f"] = sw.best()
    st = sw.status()
    out["status"] = np.array([st["iteration"], st["stop"], st["fg"]])
    out["candidate"] = sw.candidate()
    return out


def assert_mirror(dev, host, what):
    """state, best, candidate and status of a device swarm against the numpy mirror, bit for bit; returns the snapshot."""
    snap = snapshot(dev)
    for k in STATE:
        assert np.all(np.isfinite(getattr(host, k))), (what, k)
        assert np.array_equal(snap[k], getattr(host, k)), "%s: %s differs" % (what, k)
    assert np.array_equal(snap["best_x"], host.best_x) and snap["best_f"] == host.best_f, what
    assert np.array_equal(snap["candidate"], host.candidate()), what
    assert np.array_equal(snap["status"], [host.iteration, host.stop, host.fg]), (what, snap["status"], host.status())
    return snap


def host_generations(host, n):
    for _ in range(n):
        host.step_local()
        host.apply_global(host.candidate()[None, :])


# =========================================================================================================================
# ctx: a context's block, the ensure()-grown workspaces, nmrfit_dev_alloc, the scratch of generate_one
# =========================================================================================================================
CTX_N = (700, 513, 1024)          # two chunks with padding, two chunks with 511 padded points, two whole chunks
CTX_P = 3
CTX_S = (3, 300, 5)               # grow, grow, reuse with a smaller need
VARIANTS = ("default", "farfield", "norec", "farfield32")


def _ctx_spectrum(N, P=CTX_P):
    from nmrfit_amd import synth
    return synth.make_spectrum(N, P, seed=300 + N % 97 + P, physical=True)


def _ctx_rows(sp, S):
    from nmrfit_amd import synth
    return synth.make_swarm(sp["lower"], sp["upper"], S, seed=17 + S, x_true=sp["x_true"])


def _contexts(sp):
    """(form, target_waves, context): one segment per particle -- the wave writes f -- and the plan's own choice, which
    on a grid of two blocks and these swarms is two segments: per-block sums and the finalize kernel."""
    from nmrfit_amd.equations import Evaluator
    out = []
    for form, target in (("direct", 1), ("partial", None)):
        with env(NMRFIT_TARGET_WAVES=target):
            out.append((form, target, Evaluator(*spectrum_tuple(sp))))
    return out


@case("ctx", "objective_forms")
def ctx_objective_forms(rec):
    """nmrfit_objective_batch in every product variant and imaginary mode, f written by the wave and through the partial
    sums, S = 3, 300, 5 on ONE context (d_X, d_f, d_partial grow twice and are then reused), set_weights in between."""
    from nmrfit_amd import _cabi
    from oracle import c_oracle
    for N in CTX_N:
        sp = _ctx_spectrum(N)
        w, u, v, wt = spectrum_tuple(sp)
        wt2 = 0.5 + 0.25 * np.cos(np.arange(N))          # the weights set between the calls
        truth = {}
        for S in CTX_S:
            X = _ctx_rows(sp, S)
            for tag, weights in (("wt", wt), ("wt2", wt2)):
                truth[(S, tag, 0)] = c_oracle.objective_batch(X, w, u, v, weights, threads=4)
                truth[(S, tag, 1)], truth[(S, tag, 2)] = closed_form_fit_im(X, w, u, v, weights)
        for form, target, ev in _contexts(sp):
            try:
                for variant in VARIANTS:
                    vid = _cabi.variant_id(variant)
                    ev.set_variant(vid)
                    for S in CTX_S:
                        X = _ctx_rows(sp, S)
                        for tag, weights in (("wt", wt), ("wt2", wt2)):
                            ev.set_weights(weights)
                            for mode, fit_im in ((0, False), (1, True), (2, "sum")):
                                what = "objective N=%d %s %s S=%d %s fit_im=%d" % (N, form, variant, S, tag, mode)
                                f = ev.objective_batch(X, fit_im=fit_im)
                                q = ask(S, N, CTX_P, None, target, "objective", vid)
                                reached(what, ev, q, nseg=1 if form == "direct" else 2)
                                assert form == "direct" or q["wpb"] == 4, q       # (two segments in a four-wave workgroup: no direct f)
                                if mode == 0:
                                    close_f(f, truth[(S, tag, 0)], what=what)
                                else:
                                    np.testing.assert_allclose(f, truth[(S, tag, mode)], rtol=1e-11, err_msg=what)
                                rec.save("f.%d.%s.%s.%d.%s.%d" % (N, form, variant, S, tag, mode), f)
            finally:
                ev.close()


@case("ctx", "residual_rows")
def ctx_residual_rows(rec):
    """nmrfit_residual_batch and nmrfit_residual_batch_im (d_R, d_f, d_partial): B = 5 then 2 rows in both launch forms."""
    from oracle import c_oracle
    from tests import lsq_support
    for N in CTX_N:
        sp = _ctx_spectrum(N)
        w, u, v, wt = spectrum_tuple(sp)
        for form, target, ev in _contexts(sp):
            try:
                for B in (5, 2):
                    X = _ctx_rows(sp, B)
                    what = "rows N=%d %s B=%d" % (N, form, B)
                    ref_R, ref_f = c_oracle.residual_batch(X, w, u, v, wt, threads=4)
                    R, f = ev.residual_batch(X, return_f=True)
                    assert ev.last_launch()["segments"] == (1 if form == "direct" else 2), (what, ev.last_launch())
                    close_f(f, ref_f, what=what)
                    np.testing.assert_allclose(R, ref_R, rtol=0, atol=1e-11 * np.abs(ref_R).max(), err_msg=what)
                    close_f(np.sqrt(np.mean(R * R, axis=1)), ref_f, what=what)
                    rec.save("R.%d.%s.%d" % (N, form, B), R)
                    rec.save("f.%d.%s.%d" % (N, form, B), f)
                    for mode, fit_im in ((1, True), (2, "sum")):       # tests/test_gpu_lsq_im.py, test_rows_of_both_channels
                        R_re, R_im, f2 = ev.residual_batch_im(X, fit_im)
                        assert np.array_equal(R_re, R) and np.array_equal(f2[:, 0], f), what
                        assert np.array_equal(0.5 * (f2[:, 0] + f2[:, 1]), ev.objective_batch(X, fit_im=fit_im)), what
                        rms = np.sqrt(np.mean(R_im * R_im, axis=1))
                        tol = f2[:, 1] * (lsq_support.sum_bound(N, 1.0) + 4 * lsq_support.U)
                        assert np.all(np.abs(rms - f2[:, 1]) <= tol), (what, rms, f2[:, 1], tol)
                        rec.save("R_im.%d.%s.%d.%d" % (N, form, B, mode), R_im)
                        rec.save("f2.%d.%s.%d.%d" % (N, form, B, mode), f2)
            finally:
                ev.close()


@case("ctx", "dev_buffers")
def ctx_dev_buffers(rec):
    """nmrfit_objective_batch_dev and nmrfit_residual_batch_dev, df given and null, into nmrfit_dev_alloc buffers that are
    read back whole: the host-pointer calls' bits, and the C oracle's values."""
    from oracle import c_oracle
    for N in CTX_N:
        sp = _ctx_spectrum(N)
        w, u, v, wt = spectrum_tuple(sp)
        for form, target, ev in _contexts(sp):
            try:
                S = 6
                X = _ctx_rows(sp, S)
                D = X.shape[1]
                what = "dev buffers N=%d %s" % (N, form)
                dX, df, dR, df2 = ev.dev_alloc(S * D * 8), ev.dev_alloc(S * 8), ev.dev_alloc(S * N * 8), ev.dev_alloc(S * 8)
                try:
                    ev.upload(dX, X)
                    ev.objective_batch_dev(S, CTX_P, dX, df)
                    f = ev.download(df, (S,))
                    assert np.array_equal(f, ev.objective_batch(X)), what
                    close_f(f, c_oracle.objective_batch(X, w, u, v, wt), what=what)
                    ev.residual_batch_dev(S, CTX_P, dX, dR, df2)
                    R, fR = ev.download(dR, (S, N)), ev.download(df2, (S,))
                    R0, f0 = ev.residual_batch(X, return_f=True)
                    assert np.array_equal(R, R0) and np.array_equal(fR, f0), what
                    ev.residual_batch_dev(S, CTX_P, dX, dR, None)          # f into the context's own buffer
                    assert np.array_equal(ev.download(dR, (S, N)), R0), what
                    ref_R, _ = c_oracle.residual_batch(X, w, u, v, wt)
                    np.testing.assert_allclose(R, ref_R, rtol=0, atol=1e-11 * np.abs(ref_R).max(), err_msg=what)
                    rec.save("f.%d.%s" % (N, form), f)
                    rec.save("R.%d.%s" % (N, form), R)
                    rec.save("fR.%d.%s" % (N, form), fR)
                finally:
                    for p in (dX, df, dR, df2):
                        ev.dev_free(p)
            finally:
                ev.close()


def _interior(sp, seed=7):
    from nmrfit_amd import synth
    return synth.make_swarm(sp["lower"], sp["upper"], 2, seed=seed)[1]


@case("ctx", "jacobian")
def ctx_jacobian(rec):
    """nmrfit_jacobian and nmrfit_jacobian_im with J, r, A, g and f on N = 700 (eleven lsq segments, a last tile of 60
    points) at D = 10 and D = 76, and nmrfit_jacobian at P = 25, the plain kernel (tests/test_gpu_lsq_batch.py and
    tests/test_gpu_lsq_im.py: J and r the host construction's bits, A and g within the bound of exactly summed truth)."""
    from nmrfit_amd import lsq
    from nmrfit_amd.equations import Evaluator
    from tests import lsq_support as S
    N = 700
    s = 1.0 / np.sqrt(N)
    for P in (2, 24):
        sp = _ctx_spectrum(N, P)
        with Evaluator(*spectrum_tuple(sp)) as ev:
            m = lsq.ResidualModel(ev, sp["lower"], sp["upper"])
            x = _interior(sp)
            rows, h = m.rows(x)
            c = s / h
            R, f = ev.residual_batch(rows, return_f=True)
            J_host = np.ascontiguousarray(((R[1:] - R[0]) * (s / h[:, None])).T)
            r_host = R[0] * s
            out = ev.jacobian(rows, c, s, J=True, r=True, normal=True)
            what = "jacobian P=%d" % P
            assert np.array_equal(out["J"], J_host) and np.array_equal(out["r"], r_host) and out["f"] == f[0], what
            assert np.array_equal(out["A"], out["A"].T), what
            Ax, gx, absA, absg = S.exact_normal_equations(J_host, r_host)
            assert np.all(np.abs(out["A"] - Ax) <= S.sum_bound(N, absA)), what
            assert np.all(np.abs(out["g"] - gx) <= S.sum_bound(N, absg)), what
            sums = ev.jacobian(rows, c, s, normal=True)                      # no J, no r: another layout of d_lsq
            assert np.array_equal(sums["A"], out["A"]) and np.array_equal(sums["g"], out["g"]) and sums["f"] == out["f"], what
            rec.save_dict("re.%d" % P, out)
            for mode, fit_im in ((1, True), (2, "sum")):
                R_re, R_im, f2 = ev.residual_batch_im(rows, fit_im)
                both = ev.jacobian_im(rows, c, s, fit_im, J=True, r=True, normal=True)
                what = "jacobian_im P=%d mode %d" % (P, mode)
                assert np.array_equal(both["f2"], f2[0]), what
                for ch, Rc in enumerate((R_re, R_im)):
                    Jc = np.ascontiguousarray(((Rc[1:] - Rc[0]) * (s / h[:, None])).T)
                    rc = Rc[0] * s
                    assert np.array_equal(both["J"][ch], Jc) and np.array_equal(both["r"][ch], rc), (what, ch)
                    assert np.array_equal(both["A"][ch], both["A"][ch].T), (what, ch)
                    if ch == 1:
                        Ax, gx, absA, absg = S.exact_normal_equations(Jc, rc)
                        assert np.all(np.abs(both["A"][ch] - Ax) <= S.sum_bound(N, absA)), (what, ch)
                        assert np.all(np.abs(both["g"][ch] - gx) <= S.sum_bound(N, absg)), (what, ch)
                for key in ("J", "r", "A", "g"):
                    assert np.array_equal(both[key][0], out[key]), (what, key)
                rec.save_dict("im%d.%d" % (mode, P), both)
    sp = _ctx_spectrum(N, 25)                                               # D = 79: J and r element by element
    with Evaluator(*spectrum_tuple(sp)) as ev:
        m = lsq.ResidualModel(ev, sp["lower"], sp["upper"])
        rows, h = m.rows(_interior(sp))
        R = ev.residual_batch(rows)
        out = ev.jacobian(rows, s / h, s, J=True, r=True)
        assert np.array_equal(out["J"], np.ascontiguousarray(((R[1:] - R[0]) * (s / h[:, None])).T))
        assert np.array_equal(out["r"], R[0] * s)
        rec.save_dict("plain", out)


@case("ctx", "reconstruction")
def ctx_reconstruction(rec):
    """nmrfit_generate_result and nmrfit_contributions on the context's own grid and on a shorter w_out (the scratch
    buffers of generate_one): tests/test_gpu_generate.py's numpy restatement, tests/test_gpu_kk.py's closed forms."""
    from nmrfit_amd import proc_autophase, synth
    from nmrfit_amd.equations import Evaluator
    from oracle import nmrfit_oracle as onp
    for N in CTX_N:
        sp = _ctx_spectrum(N)
        x = np.array(sp["x_true"])
        x[0], x[1] = 0.7, -1.3
        with Evaluator(*spectrum_tuple(sp)) as ev:
            for tag, wout in (("own", None), ("short", np.linspace(sp["w"][10], sp["w"][-10], 333))):
                what = "reconstruction N=%d %s" % (N, tag)
                grid = sp["w"] if wout is None else wout
                real, imag, fit, data = ev.generate_result(x, wout)
                real2, imag2 = ev.contributions(x, wout)
                assert np.array_equal(real, real2) and np.array_equal(imag, imag2), what
                want = np.stack([onp.voigt(grid, x[2], x[3], *x[4 + 3 * k:7 + 3 * k]) for k in range(CTX_P)])
                np.testing.assert_allclose(real, want, rtol=0, atol=1e-12 * np.abs(want).max(), err_msg=what)
                cf = np.stack([synth._dispersion(grid, x[2], *x[4 + 3 * k:7 + 3 * k]) for k in range(CTX_P)])
                np.testing.assert_allclose(imag, cf, rtol=0, atol=1e-13 * np.abs(cf).max(), err_msg=what)
                V, I = np.zeros(len(grid)), np.zeros(len(grid))
                for k in range(CTX_P):
                    V, I = V + real[k], I + imag[k]
                assert np.array_equal(fit[0], V) and np.array_equal(fit[1], I), what
                uf, vf = proc_autophase.ps2(V, I, inv=True, p0=x[0], p1=x[1])
                top = max(np.abs(V).max(), np.abs(I).max())
                np.testing.assert_allclose(fit[2], uf, rtol=0, atol=1e-14 * top, err_msg=what)
                np.testing.assert_allclose(fit[3], vf, rtol=0, atol=1e-14 * top, err_msg=what)
                Vd, Id = proc_autophase.ps2(sp["u"], sp["v"], x[0], x[1])
                top = max(np.abs(sp["u"]).max(), np.abs(sp["v"]).max())
                np.testing.assert_allclose(data[0], Vd, rtol=0, atol=1e-14 * top, err_msg=what)
                np.testing.assert_allclose(data[1], Id, rtol=0, atol=1e-14 * top, err_msg=what)
                for key, a in (("real", real), ("imag", imag), ("fit", fit), ("data", data)):
                    rec.save("%s.%d.%s" % (key, N, tag), a)


@case("ctx", "profiling")
def ctx_profiling(rec):
    """nmrfit_prof_enable's clock words (d_clk): zeroed at allocation, written by workgroup 0 of a profiled launch, read by
    nmrfit_prof_read.  The durations are not results (they differ from run to run): their counts are recorded, and the
    clock the two pairs of ticks give is held to a plausible range."""
    from nmrfit_amd.equations import Evaluator
    sp = _ctx_spectrum(700)
    X = _ctx_rows(sp, 5)
    with Evaluator(*spectrum_tuple(sp)) as ev:
        ev.prof_enable(4)
        ev.prof_mark()
        f = ev.objective_batch(X)
        ev.prof_mark()
        f2 = ev.objective_batch(X)
        ev.prof_mark()
        kernel_ms, step_ms, mhz = ev.prof_read()
        assert len(kernel_ms) == 2 and len(step_ms) == 2 and np.all(kernel_ms > 0) and np.all(step_ms > 0), (kernel_ms, step_ms)
        assert 100.0 < mhz < 5000.0, mhz
        ev.prof_enable(0)
        assert np.array_equal(f, f2) and np.array_equal(ev.objective_batch(X), f)
        rec.save("counts", [len(kernel_ms), len(step_ms)])
        rec.save("f", f)


# =========================================================================================================================
# swarm: a swarm's block (nmrfit_pso_create), and the context's d_partial under a swarm
# =========================================================================================================================
def _swarm_problem(N, P, seed=5):
    from nmrfit_amd import synth
    return synth.make_spectrum(N, P, seed=seed)


def _mirrored(rec, key, ev, sp, S, seed, gens, launches, plan_mode, want, tail=True, pbest=True, ev_host=None, reads=(4, 8),
              pair=None):
    """``gens`` generations through step() against HostSwarm, bit for bit: state, best, candidate and status read after
    generation 0, after the generations ``reads`` and at the end; the launch form held to the plan after every step."""
    from nmrfit_amd.pso import DeviceSwarm
    from tests import swarm_support
    P = (len(sp["lower"]) - 4) // 3
    host = swarm_support.HostSwarm((ev_host or ev).objective_batch, sp["lower"], sp["upper"], S, seed=seed, **FREE)
    dev = DeviceSwarm(ev, sp["lower"], sp["upper"], S, seed=seed, **FREE)
    try:
        dev.set_fused_tail(tail)
        dev.set_fused_pbest(pbest)
        host.init()
        host.apply_global(host.candidate()[None, :])
        dev.init()
        dev.step()                                           # folds generation 0
        rec.save_dict(key + ".gen0", assert_mirror(dev, host, key + " generation 0"))
        pending = False
        for gen in range(1, gens + 1):
            host_generations(host, 1)
            dev.step()
            mode = plan_mode + ("+pending" if plan_mode.endswith("+tail") and pending and want.get("tail") else "")
            q = ask(S, ev.N, P, pair, 0, mode)
            reached("%s generation %d" % (key, gen), ev, q, **want)
            assert dev.last_launches() == launches, (key, gen, dev.last_launches(), launches)
            pending = bool(want.get("tail"))
            if gen in reads:
                rec.save_dict("%s.gen%d" % (key, gen), assert_mirror(dev, host, "%s generation %d" % (key, gen)))
                pending = False                              # (reading folds the waiting generation)
        snap = assert_mirror(dev, host, key + " the end")
        assert snap["status"][0] == gens and snap["status"][1] == 0, snap["status"]
        rec.save_dict(key + ".end", snap)
    finally:
        dev.close()


@case("swarm", "before_init")
def swarm_before_init(rec):
    """What a caller sees before nmrfit_pso_init: status and best are defined (the state blocks are zeroed at creation),
    state and candidate are refused with NMRFIT_E_STATE (generation 0 is the first writer of those arrays)."""
    from nmrfit_amd import _cabi
    from nmrfit_amd.equations import Evaluator
    from nmrfit_amd.pso import DeviceSwarm
    sp = _swarm_problem(700, 3)
    with Evaluator(*spectrum_tuple(sp)) as ev:
        sw = DeviceSwarm(ev, sp["lower"], sp["upper"], 16, seed=1)
        try:
            assert sw.status() == dict(iteration=0, stop=0, fg=0.0)
            xb, fb = sw.best()
            assert fb == 0.0 and np.array_equal(xb, np.zeros(sw.D))
            for read in (sw.state, sw.candidate):
                try:
                    read()
                except _cabi.NmrfitError as e:
                    assert e.code == _cabi.E_STATE, (read, e)
                else:
                    raise AssertionError("%r before init was not refused" % (read,))
            sw.init()                                        # ... and the swarm is usable after the refusals
            sw.step()
            rec.save_dict("after", snapshot(sw))
            rec.save("best_x_before", xb)
        finally:
            sw.close()


@case("swarm", "small_16")
def swarm_small(rec):
    """S = 16 on a grid of two blocks: two segments per particle (d_partial), everything after the objective launch in the
    one-workgroup tail kernel (finalize, personal bests, argmin, fold)."""
    from nmrfit_amd.equations import Evaluator
    sp = _swarm_problem(700, 3)
    with Evaluator(*spectrum_tuple(sp)) as ev:
        _mirrored(rec, "s16", ev, sp, 16, 77, 12, 2, "fused+pbest+tail", dict(nseg=2, pbest=0, tail=0))


@case("swarm", "tail_204")
def swarm_tail(rec):
    """S = 204, P = 6, N = 4096 with the one-launch form off: the personal bests in the objective launch, argmin and fold
    in the one-workgroup tail kernel."""
    from nmrfit_amd.equations import Evaluator
    sp = _swarm_problem(4096, 6, seed=11)
    with Evaluator(*spectrum_tuple(sp)) as ev:
        _mirrored(rec, "tail", ev, sp, 204, 41, 12, 2, "fused+pbest", dict(nseg=8, wpb=8, pbest=1, tail=0), tail=False)


@case("swarm", "deferred_204")
def swarm_deferred(rec):
    """The same swarm in the one-launch form: the fold deferred into the next launch's prologue -- both state blocks, both
    (p, fp) buffers, the candidate record written by workgroup 0."""
    from nmrfit_amd.equations import Evaluator
    sp = _swarm_problem(4096, 6, seed=11)
    with Evaluator(*spectrum_tuple(sp)) as ev:
        _mirrored(rec, "deferred", ev, sp, 204, 41, 12, 1, "fused+pbest+tail", dict(nseg=8, wpb=8, pbest=1, tail=1))


@case("swarm", "select_1025_1026")
def swarm_select(rec):
    """S = 1025 and 1026 on a grid of two blocks: the many-workgroup select kernel (257 posts, one of them of one or two
    particles) and the final reduction as a launch of its own -- d_part_val, d_part_idx, d_partial."""
    from nmrfit_amd.equations import Evaluator
    sp = _swarm_problem(700, 6, seed=12)
    with Evaluator(*spectrum_tuple(sp)) as ev:
        for S in (1025, 1026):
            _mirrored(rec, "select%d" % S, ev, sp, S, 9, 12, 3, "fused+pbest+tail", dict(nseg=2, pbest=0, tail=0))


@case("swarm", "pair_own")
def swarm_pair(rec):
    """The pair form where the plan takes it by itself: S = 8 x compute units on a grid of 64 chunks; the mirror's values
    come from a context with the pair form off (tests/test_gpu_pair_swarm_modes.py)."""
    from nmrfit_amd import _cabi
    from nmrfit_amd.equations import Evaluator
    S = 8 * _cabi.device_info(0)["compute_units"]
    sp = _swarm_problem(32768, 2, seed=13)
    with env(NMRFIT_PAIR_WAVES=None):
        ev1 = Evaluator(*spectrum_tuple(sp))
    with env(NMRFIT_PAIR_WAVES=0):
        ev0 = Evaluator(*spectrum_tuple(sp))
    try:
        _mirrored(rec, "pair", ev1, sp, S, 7, 12, 2, "fused+pbest+tail", dict(unit="pair", pair=1, pbest=1, tail=0, rows=2),
                  ev_host=ev0)
    finally:
        ev1.close()
        ev0.close()


@case("swarm", "minfunc_stop")
def swarm_stop(rec):
    """pyswarm's rule armed: nmrfit_pso_run stops by minfunc or minstep at the mirror's generation with the mirror's answer
    (tests/test_gpu_pso.py, test_stop_flag_on_device_and_run_polling), and the generations after the stop change nothing."""
    from nmrfit_amd import pso
    from nmrfit_amd.equations import Evaluator
    from tests import swarm_support
    sp = _swarm_problem(2048, 3)
    with Evaluator(*spectrum_tuple(sp)) as ev:
        host = swarm_support.HostSwarm(ev.objective_batch, sp["lower"], sp["upper"], 64, seed=3)
        pso.run_sharded(host, pso.LocalExchange(), 400)
        assert host.stop in (1, 2), host.status()
        sw = pso.DeviceSwarm(ev, sp["lower"], sp["upper"], 64, seed=3)
        try:
            sw.run(400, check_every=7)
            snap = assert_mirror(sw, host, "stop")
            sw.step()
            sw.step()
            again = snapshot(sw)
            for k in snap:
                assert np.array_equal(snap[k], again[k]), k
            rec.save_dict("stop", snap)
        finally:
            sw.close()


@case("swarm", "second_in_freed_block")
def swarm_second(rec):
    """Two swarms of one shape on one context, one after the other: the second is created in the block the first has just
    freed, which holds the first's personal bests, posts and flags."""
    from nmrfit_amd.equations import Evaluator
    from nmrfit_amd.pso import DeviceSwarm
    sp = _swarm_problem(700, 6, seed=12)
    with Evaluator(*spectrum_tuple(sp)) as ev:
        first = DeviceSwarm(ev, sp["lower"], sp["upper"], 1025, seed=1, **FREE)
        first.run(5, 5)
        rec.save_dict("first", snapshot(first))
        first.close()
        _mirrored(rec, "second", ev, sp, 1025, 2, 12, 3, "fused+pbest+tail", dict(nseg=2, pbest=0, tail=0))


# =========================================================================================================================
# batch: a part's block (nmrfit_batch_create*), d_result, d_quality, the scratch of add_noise / spectrum / least squares
# =========================================================================================================================
BATCH_N = (300, 513, 1025, 512, 700, 1000, 2048)        # seven fits: two parts (3 + 4); lengths around the 512-point chunk
BATCH_P = (1, 2, 24, 1, 1, 2, 24)                       # (D = 76 twice: their residual rows do not share a 1 MiB group)
BATCH_S = 16
BATCH_SEEDS = [101 + k for k in range(7)]
BATCH_GENS = 12


def _batch_problems():
    from nmrfit_amd import synth
    return [synth.make_spectrum(n, p, seed=20 + k, physical=True) for k, (n, p) in enumerate(zip(BATCH_N, BATCH_P))]


def _uniform_problems():
    from nmrfit_amd import synth
    return [synth.make_spectrum(1700, p, seed=60 + k, physical=True) for k, p in enumerate((1, 2, 3, 1, 2, 3, 2))]


def _lone_swarms(problems, weights, fit_im, S=BATCH_S, seeds=BATCH_SEEDS, **kw):
    from nmrfit_amd.equations import Evaluator
    from nmrfit_amd.pso import DeviceSwarm
    evs, sws = [], []
    for sp, wt, seed in zip(problems, weights, seeds):
        ev = Evaluator(sp["w"], sp["u"], sp["v"], wt)
        ev.set_fit_im(fit_im)
        evs.append(ev)
        sws.append(DeviceSwarm(ev, sp["lower"], sp["upper"], S, seed=seed, **kw))
    return evs, sws


def _close_all(evs, sws):
    for sw in sws:
        sw.close()
    for ev in evs:
        ev.close()


def _same_as_lone(rec, key, fb, sws, what):
    st, best = fb.status(), fb.best()
    for k, sw in enumerate(sws):
        a, b = fb.state(k), sw.state()
        for name in STATE:
            assert np.all(np.isfinite(b[name])), (what, k, name)
            assert np.array_equal(a[name], b[name]), "%s: fit %d %s" % (what, k, name)
        ls = sw.status()
        assert (st[k]["iteration"], st[k]["stop"], st[k]["fg"]) == (ls["iteration"], ls["stop"], ls["fg"]), (what, k)
        xb, fbest = sw.best()
        assert np.array_equal(best[k][0], xb) and best[k][1] == fbest, (what, k)
        rec.save_dict("%s.state%d" % (key, k), a)
        rec.save("%s.best_x%d" % (key, k), best[k][0])
        rec.save("%s.best_f%d" % (key, k), best[k][1])
        rec.save("%s.status%d" % (key, k), [st[k]["iteration"], st[k]["stop"], st[k]["fg"]])


def _refused_with_state(call, what):
    from nmrfit_amd import _cabi
    try:
        call()
    except _cabi.NmrfitError as e:
        assert e.code == _cabi.E_STATE, (what, e)
    else:
        raise AssertionError("%s was not refused" % what)


@case("batch", "before_generation_0")
def batch_before(rec):
    """What a caller sees before generation 0: spectrum(k) is the upload (defined); status, best, state, generate and
    residual_stats of the best rows are refused with NMRFIT_E_STATE (the tail kernel is the summary's first writer)."""
    from nmrfit_amd.batch import FitBatch
    problems = _batch_problems()
    with FitBatch([spectrum_tuple(sp) for sp in problems], [sp["lower"] for sp in problems], [sp["upper"] for sp in problems],
                  swarmsize=BATCH_S, seeds=BATCH_SEEDS) as fb:
        for k, sp in enumerate(problems):
            u, v = fb.spectrum(k)
            assert u.tobytes() == sp["u"].tobytes() and v.tobytes() == sp["v"].tobytes(), k
        for what, call in (("status", fb.status), ("best", fb.best), ("state", lambda: fb.state(0)), ("state of the last fit", lambda: fb.state(6)),
                           ("generate", fb.generate), ("residual_stats", fb.residual_stats)):
            _refused_with_state(call, what)
        fb.run(2, 1)                                         # ... and the batch is usable after the refusals
        rec.save("best_f", [f for _, f in fb.best()])


@case("batch", "ragged_weights")
def batch_ragged_weights(rec):
    """Seven ragged fits in two parts, created from weights, fit_im off / reference / sum (the wave = particle form):
    12 generations against the lone swarms, bit for bit."""
    from nmrfit_amd.batch import FitBatch
    problems = _batch_problems()
    for tag, fit_im in (("off", False), ("ref", True), ("sum", "sum")):
        evs, sws = _lone_swarms(problems, [sp["weights"] for sp in problems], fit_im, **FREE)
        try:
            for sw in sws:
                sw.run(BATCH_GENS, 4)
            with FitBatch([spectrum_tuple(sp) for sp in problems], [sp["lower"] for sp in problems], [sp["upper"] for sp in problems],
                          swarmsize=BATCH_S, seeds=BATCH_SEEDS, fit_im=fit_im, **FREE) as fb:
                assert fb.geometry()["mode"] == "wave"
                fb.run(BATCH_GENS, 4)
                _same_as_lone(rec, tag, fb, sws, "ragged weights fit_im=%s" % tag)
        finally:
            _close_all(evs, sws)


@case("batch", "ragged_regions")
def batch_ragged_regions(rec):
    """The same fits created from regions: the weights plane built on the device (the region tables and the index pairs
    behind the landing buffer) against lone swarms on utils.compute_weights."""
    from nmrfit_amd import utils
    from nmrfit_amd.batch import FitBatch
    problems = _batch_problems()
    weights = [utils.compute_weights(sp["w"], sp["peaks"]) for sp in problems]
    regions = [utils.weight_regions(sp["w"], sp["peaks"]) for sp in problems]
    regions[3] = None                                        # one fit without regions: unit weights
    weights[3] = utils.compute_weights(problems[3]["w"], [])
    evs, sws = _lone_swarms(problems, weights, False, **FREE)
    try:
        for sw in sws:
            sw.run(BATCH_GENS, 4)
        with FitBatch([(sp["w"], sp["u"], sp["v"]) for sp in problems], [sp["lower"] for sp in problems], [sp["upper"] for sp in problems],
                      swarmsize=BATCH_S, seeds=BATCH_SEEDS, regions=regions, **FREE) as fb:
            fb.run(BATCH_GENS, 4)
            _same_as_lone(rec, "regions", fb, sws, "ragged regions")
    finally:
        _close_all(evs, sws)


@case("batch", "uniform_both_geometries")
def batch_uniform(rec):
    """Seven fits of one length and swarm size: both launch geometries, a change of geometry under a waiting fold."""
    from nmrfit_amd.batch import FitBatch
    problems = _uniform_problems()
    evs, sws = _lone_swarms(problems, [sp["weights"] for sp in problems], False, **FREE)
    try:
        for sw in sws:
            sw.run(BATCH_GENS, 4)
        for geometry in ("workgroup", "wave"):
            with FitBatch([spectrum_tuple(sp) for sp in problems], [sp["lower"] for sp in problems], [sp["upper"] for sp in problems],
                          swarmsize=BATCH_S, seeds=BATCH_SEEDS, **FREE) as fb:
                fb.set_geometry(geometry)
                g = fb.geometry()
                assert g["mode"] == geometry and (geometry == "wave" or g["segments"] == g["waves_per_workgroup"] == 4), g
                fb.run(BATCH_GENS // 2, 4)
                fb.set_geometry("wave" if geometry == "workgroup" else "workgroup")
                fb.run(BATCH_GENS - BATCH_GENS // 2, 4)
                _same_as_lone(rec, geometry, fb, sws, "uniform, starting in the %s form" % geometry)
    finally:
        _close_all(evs, sws)


def _stats_regions(sp):
    w = sp["w"]
    out = [tuple(p.bounds) for p in sp["peaks"][:3]]
    return out + [(w[len(w) // 2], w[len(w) // 2 + 1])]


@case("batch", "data_calls")
def batch_data_calls(rec):
    """generate / contributions on the own grids and on upsampled ones (d_result), residual_stats of the best rows and of
    given rows (d_quality: grown, then reused), against the lone reconstruction and the numpy mirror of the rows."""
    from nmrfit_amd import quality
    from nmrfit_amd.batch import FitBatch
    from tests.batch_walk_support import lone_result
    problems = _batch_problems()
    regions = [_stats_regions(sp) for sp in problems]
    regions[1] = []
    with FitBatch([spectrum_tuple(sp) for sp in problems], [sp["lower"] for sp in problems], [sp["upper"] for sp in problems],
                  swarmsize=BATCH_S, seeds=BATCH_SEEDS, **FREE) as fb:
        given = [sp["x_true"] for sp in problems]
        early = fb.residual_stats(given, regions)            # given rows: allowed before generation 0
        fb.run(BATCH_GENS, 4)
        best = fb.best()
        for scale in (1, 1.5):
            res = fb.generate(scale)
            for k, (sp, (x, _)) in enumerate(zip(problems, best)):
                fu, data = lone_result(sp, x, scale)
                r = res[k]
                what = "generate fit %d scale %r" % (k, scale)
                assert np.array_equal(r["real"], np.stack(fu.real_contribs)) and np.array_equal(r["imag"], np.stack(fu.imag_contribs)), what
                for name in ("V", "I", "u", "v"):
                    assert np.array_equal(r[name], getattr(fu, name)), (what, name)
                assert np.array_equal(r["data_V"], data.V) and np.array_equal(r["data_I"], data.I), what
                for name in ("real", "imag", "V", "I", "u", "v", "data_V", "data_I"):
                    rec.save("gen.%r.%d.%s" % (scale, k, name), r[name])
        gen = fb.generate()
        rows = fb.residual_stats(regions=regions)
        late = fb.residual_stats(given, regions)
        for k, (sp, reg) in enumerate(zip(problems, regions)):
            want = quality.residual_stats_host(gen[k]["V"], gen[k]["data_V"], sp["w"], reg)
            assert rows[k].rows.shape == (len(reg) + 2, 8) and np.array_equal(rows[k].rows, want), k
            assert np.array_equal(early[k].rows, late[k].rows, equal_nan=True), k
            lone = quality.residual_stats(sp["w"], sp["u"], sp["v"], sp["x_true"], reg)
            assert np.array_equal(late[k].rows, lone.rows, equal_nan=True), k
            rec.save("stats.best.%d" % k, rows[k].rows)
            rec.save("stats.given.%d" % k, late[k].rows)


@case("batch", "normal_equations")
def batch_normal_equations(rec):
    """nmrfit_batch_normal_equations and _im with NMRFIT_LSQ_WORKSPACE_MB=1 (the fits of a part go in more than one
    group: the call's scratch is allocated and freed per group) against lone contexts, bit for bit."""
    from nmrfit_amd import lsq
    from nmrfit_amd.batch import FitBatch
    from nmrfit_amd.equations import Evaluator
    problems = _batch_problems()
    X = [_interior(sp, seed=11 + k) for k, sp in enumerate(problems)]
    X[1] = np.array(problems[1]["upper"], dtype=float)       # one fit on its upper bound: flipped steps
    with env(NMRFIT_LSQ_WORKSPACE_MB=1):
        for tag, fit_im in (("off", False), ("ref", True), ("sum", "sum")):
            with FitBatch([spectrum_tuple(sp) for sp in problems], [sp["lower"] for sp in problems], [sp["upper"] for sp in problems],
                          swarmsize=BATCH_S, seeds=BATCH_SEEDS, fit_im=fit_im) as fb:
                got = fb.normal_equations(X)
                both = fb.normal_equations(X, channels="both") if fit_im else None
            for k, (sp, x) in enumerate(zip(problems, X)):
                with Evaluator(*spectrum_tuple(sp)) as ev:
                    A, g, f = lsq.ResidualModel(ev, sp["lower"], sp["upper"]).normal_equations(x)
                    assert np.array_equal(got[k][0], A) and np.array_equal(got[k][1], g) and got[k][2] == f, (tag, k)
                    rec.save("%s.A%d" % (tag, k), got[k][0])
                    rec.save("%s.g%d" % (tag, k), got[k][1])
                    rec.save("%s.f%d" % (tag, k), got[k][2])
                    if both is not None:
                        H, grad, fc = lsq.ResidualModel(ev, sp["lower"], sp["upper"], fit_im=fit_im).normal_equations(x)
                        assert np.array_equal(both[k][0], H) and np.array_equal(both[k][1], grad) and both[k][2] == fc, (tag, k)
                        rec.save("%s.H%d" % (tag, k), both[k][0])
                        rec.save("%s.grad%d" % (tag, k), both[k][1])
                        rec.save("%s.fc%d" % (tag, k), both[k][2])


@case("batch", "noise_and_spectrum")
def batch_noise(rec):
    """add_noise in place on the resident planes, then spectrum(k): noise.replicas of the upload, bit for bit (sigma 0:
    the upload's bits), and the fits that follow equal those of a batch uploaded with the replicas."""
    from nmrfit_amd import noise
    from nmrfit_amd.batch import FitBatch
    problems = _batch_problems()
    su = np.array([2e-3, 1e-3, 0.0, 5e-4, 3e-3, 0.0, 1e-3])
    sv = np.array([1e-3, 3e-3, 0.0, 5e-4, 0.0, 0.0, 2e-3])
    seeds = [11, 12, 13, (1 << 32) + 14, 15, 16, (1 << 63) + 17]
    noisy = noise.replicas([s["u"] for s in problems], [s["v"] for s in problems], su, sv, seeds)

    def make(uv):
        return FitBatch([(s["w"], u, v, s["weights"]) for s, (u, v) in zip(problems, uv)], [s["lower"] for s in problems],
                        [s["upper"] for s in problems], swarmsize=BATCH_S, seeds=BATCH_SEEDS)
    with make([(s["u"], s["v"]) for s in problems]) as fb, make(noisy) as fa:
        fb.add_noise(su, sv, seeds)
        for k, s in enumerate(problems):
            u, v = fb.spectrum(k)
            assert np.array_equal(u, noisy[k][0]) and np.array_equal(v, noisy[k][1]), k
            if k in (2, 5):
                assert u.tobytes() == s["u"].tobytes() and v.tobytes() == s["v"].tobytes(), k
            rec.save("u%d" % k, u)
            rec.save("v%d" % k, v)
        _refused_with_state(lambda: fb.add_noise(su, sv, seeds), "a second add_noise")
        fa.run(BATCH_GENS)
        fb.run(BATCH_GENS)
        for k, ((xa, fa_), (xb, fb_)) in enumerate(zip(fa.best(), fb.best())):
            assert np.array_equal(xa, xb) and fa_ == fb_, k
            rec.save("best_x%d" % k, xb)


@case("batch", "polish")
def batch_polish(rec):
    """One batch polish (lsq.lm_polish over nmrfit_batch_normal_equations) against the per-fit scipy path and the C oracle
    (tests/test_gpu_lsq_batch.py, test_batch_polish_against_the_per_fit_path)."""
    from nmrfit_amd import lsq
    from nmrfit_amd.batch import FitBatch
    from nmrfit_amd.equations import Evaluator
    from oracle import c_oracle
    from tests import lsq_support as S
    specs = [sp for sp, _ in S.polish_cases()[:2]]
    with FitBatch([spectrum_tuple(sp) for sp in specs], [sp["lower"] for sp in specs], [sp["upper"] for sp in specs],
                  swarmsize=64, seeds=[3, 4]) as fb:
        fb.run(100, 10)
        start = fb.best()
        res = fb.polish(max_launches=100 * max(fb.D))
    for k, (sp, (xs, fs), (x, f)) in enumerate(zip(specs, start, res)):
        assert f <= fs and np.all(x >= sp["lower"]) and np.all(x <= sp["upper"]), k
        ref = c_oracle.objective_batch(x, *spectrum_tuple(sp))[0]
        assert abs(f - ref) <= 1e-9 * abs(ref), (k, f, ref)
        with Evaluator(*spectrum_tuple(sp)) as ev:
            xp, fp, _ = lsq.polish(ev, xs, sp["lower"], sp["upper"], **S.TRF_TOL)
        assert abs(f - fp) / fp <= S.FINAL_F_BAR, (k, f, fp)
        rec.save("x%d" % k, x)
        rec.save("f%d" % k, f)


# =========================================================================================================================
# prep: the scratch of the preparation calls (noise, weights, quality, peaks, phase)
# =========================================================================================================================
@case("prep", "noise_replicas")
def prep_noise(rec):
    """noise.replicas, K = 5 around the 512-point chunk, one sigma 0, against replicas_host (tests/test_gpu_noise.py,
    test_mirror: within (B + 1) e sigma + ulp)."""
    from nmrfit_amd import noise
    B = 2.0
    Ns = (1, 511, 512, 513, 1025)
    rng = np.random.default_rng(4)
    us = [rng.standard_normal(n) for n in Ns]
    vs = [rng.standard_normal(n) for n in Ns]
    su = np.array([0.5, 2.0, 0.0, 1e-3, 0.25])
    sv = np.array([0.25, 1.0, 0.0, 2e-3, 4.0])
    seeds = [1, 2, 3, (1 << 32) + 5, (1 << 40) + 1]
    got = noise.replicas(us, vs, su, sv, seeds)
    want = noise.replicas_host(us, vs, su, sv, seeds)
    for k, n in enumerate(Ns):
        zu, zv = noise.normals(seeds[k], n)
        e = 2.0 ** -52 * np.maximum(1.0, np.hypot(zu, zv))
        for g, w, s in ((got[k][0], want[k][0], su[k]), (got[k][1], want[k][1], sv[k])):
            assert g.shape == (n,) and np.all(np.isfinite(g)), k
            tol = (B + 1.0) * e * s + np.spacing(np.abs(w))
            assert np.all(np.abs(g - w) <= tol), (k, np.max(np.abs(g - w) / tol))
        rec.save("u%d" % k, got[k][0])
        rec.save("v%d" % k, got[k][1])
    assert got[2][0].tobytes() == us[2].tobytes() and got[2][1].tobytes() == vs[2].tobytes()      # sigma 0: the bits stay


class _Pk:
    def __init__(self, b0, b1, height=1.0):
        self.bounds = [b0, b1]
        self.height = height


@case("prep", "compute_weights_many")
def prep_weights(rec):
    """compute_weights_many on a ragged call with a spectrum without regions and one of 1025 points (two tiles of the
    fill-and-smooth kernel): utils.compute_weights and the reference's loop, bit for bit; the index pairs numpy's."""
    from nmrfit_amd import utils
    from oracle import nmrfit_oracle as onp
    grids = [np.arange(40) / 2.0, np.arange(1025, dtype=float), np.arange(700, dtype=float)[::-1].copy(), np.arange(64) / 4.0]
    peaks = [[_Pk(2, 10, 1), _Pk(6, 14, 2), _Pk(7, 9, 4)],
             [_Pk(1000, 1030, 3.0), _Pk(1019, 1024, 1.0), _Pk(5, 40, 2.0), _Pk(1023.4, 1023.6, 5.0)],
             [_Pk(100, 300, 2.0), _Pk(250, 260, 1.0)],
             []]
    got, pairs = utils.compute_weights_many(grids, peaks, return_pairs=True)
    for k, (w, pk) in enumerate(zip(grids, peaks)):
        host = utils.compute_weights(w, pk)
        loop = onp.compute_weights(np.asarray(w), pk, 0.5) if pk else np.ones(len(w))
        assert np.array_equal(got[k], host) and np.array_equal(got[k], loop), k
        want = np.array([sorted(int(np.argmin(np.abs(w - b))) for b in p.bounds) for p in pk], dtype=np.int64).reshape(-1, 2)
        assert np.array_equal(pairs[k], want), (k, pairs[k], want)
        rec.save("weights%d" % k, got[k])
        rec.save("pairs%d" % k, pairs[k])


@case("prep", "quality_stats")
def prep_quality(rec):
    """nmrfit_quality_stats from host arrays with R = 0, 5 and 17 regions (19 rows: two row batches of the tiles kernel)
    against residual_stats_host of the lone reconstruction, bit for bit (tests/test_gpu_quality.py)."""
    from nmrfit_amd import quality, synth
    from tests.batch_walk_support import lone_result
    specs = [synth.make_spectrum(n, p, seed=30 + k, physical=True) for k, (n, p) in enumerate(((700, 3), (257, 2), (1025, 2)))]
    w0, w2 = specs[0]["w"], specs[2]["w"]
    h = w0[1] - w0[0]
    regions = [[(w0[100], w0[100] + 0.2 * h), (w0[63], w0[64]), (w0[255], w0[256]), (w0[300], w0[250]), (w0[690], 1.0e9)], [],
               [(w2[60 * r], w2[60 * r + 7 + r]) for r in range(17)]]
    X = [sp["x_true"] * (1.0 + 0.01 * np.cos(np.arange(len(sp["x_true"])))) for sp in specs]
    many = quality.residual_stats_many([(s["w"], s["u"], s["v"]) for s in specs], X, regions)
    for k, (sp, x, reg) in enumerate(zip(specs, X, regions)):
        fu, data = lone_result(sp, x, 1)
        want = quality.residual_stats_host(np.array(fu.V), np.array(data.V), sp["w"], reg)
        assert many[k].rows.shape == (len(reg) + 2, 8) and np.array_equal(many[k].rows, want), (k, many[k].rows, want)
        alone = quality.residual_stats(sp["w"], sp["u"], sp["v"], x, reg)
        assert np.array_equal(alone.rows, many[k].rows), k
        rec.save("rows%d" % k, many[k].rows)


@case("prep", "select_peaks_many")
def prep_peaks(rec):
    """select_peaks_many on three Data objects of different lengths against the host's select_peaks (tests/test_gpu_peaks.py:
    count, i, loc, width, bounds and idx exactly; baseline, height and area within 1e-12)."""
    from nmrfit_amd import containers, synth
    shapes = ((600, 2, 1), (1024, 3, 6), (333, 1, 9))
    hosts, devs = [], []
    for N, P, seed in shapes:
        sp = synth.make_spectrum(N, P, seed=seed)
        for out in (hosts, devs):
            d = containers.Data(sp["w"], sp["u"], np.zeros(N))
            d.shift_phase(method="manual", p0=0.0, p1=0.0)
            out.append(d)
    for d in hosts:
        d.select_peaks(method="auto", thresh=0.1, window=0.02)
    containers.select_peaks_many(devs, method="auto", thresh=0.1, window=0.02)

    def ok(a, b, scale):
        return abs(a - b) <= 1e-12 * max(abs(b), scale)
    for k, (dh, dd) in enumerate(zip(hosts, devs)):
        scale = np.abs(dh.V).max()
        assert len(dd.peaks) == len(dh.peaks) > 0 and dd.roibounds == dh.roibounds, (k, len(dd.peaks), len(dh.peaks))
        for g, p in zip(dd.peaks, dh.peaks):
            assert g.i == p.i and g.loc == p.loc and g.width == p.width and g.bounds == p.bounds, k
            assert np.array_equal(g.idx[0], p.idx[0]), k
            assert ok(g.baseline, p.baseline, scale) and ok(g.height, p.height, scale), k
            assert ok(g.area, p.area, scale * (p.bounds[1] - p.bounds[0])), k
        rec.save("peaks%d" % k, [[g.i, g.loc, g.width, g.bounds[0], g.bounds[1], g.baseline, g.height, g.area] for g in dd.peaks])


def _phase_spectra():
    from nmrfit_amd import synth
    out = []
    # 256 threads below 16384 points, 512 from there on; the first line lies at a tenth of the grid, beyond the first 100
    # points (where the reference's peak-minima window is empty and the score raises)
    for k, (N, P) in enumerate(((1200, 1), (16384, 2), (1537, 1), (20000, 4), (2000, 3))):
        sp = synth.make_spectrum(N, P, seed=31 + k, physical=True)
        out.append(sp["u"] + 1j * sp["v"])
    return out


@case("prep", "phase")
def prep_phase(rec):
    """phase_scores, estimate_many and brute_levels on ragged lengths that mix the 256- and the 512-thread form, against
    the host scores, scipy's fmin and the host's level loop (tests/test_gpu_phase.py)."""
    import scipy.optimize
    from nmrfit_amd import proc_autophase
    zs = _phase_spectra()
    ph = np.random.default_rng(11).uniform(-40, 40, (len(zs), 4, 2))
    ph[:, 0] = 0.0
    got = proc_autophase.phase_scores(zs, ph, "acme")
    want = np.array([[proc_autophase._ps_acme_score(p, z) for p in phk] for z, phk in zip(zs, ph)])
    rel = np.abs(got - want) / np.maximum(np.abs(want), 1e-300)
    assert np.all((got == want) | (rel <= 1e-12)), rel.max()
    rec.save("acme", got)
    got = proc_autophase.phase_scores(zs, ph, "peak_minima")
    want = np.array([[proc_autophase._ps_peak_minima_score(p, z) for p in phk] for z, phk in zip(zs, ph)])
    np.testing.assert_allclose(got, want, rtol=1e-12, atol=1e-15)
    rec.save("peak_minima", got)
    for fn, p0, p1 in (("acme", 0.0, 0.0), ("peak_minima", 5.0, -3.0)):
        x, f, nfev, nit = proc_autophase.estimate_many(zs, fn, p0, p1)
        for k, z in enumerate(zs):
            xs, fs, its, fev, _ = scipy.optimize.fmin(proc_autophase._SCORES[fn], [p0, p1], args=(z,), disp=False, full_output=True)
            np.testing.assert_allclose(x[k], xs, rtol=0, atol=1e-8)
            assert nfev[k] == fev and nit[k] == its, (fn, k, nfev[k], fev, nit[k], its)
        for key, a in (("x", x), ("f", f), ("nfev", nfev), ("nit", nit)):
            rec.save("estimate.%s.%s" % (fn, key), a)
    angles = np.arange(-np.pi, np.pi, np.pi / 45)
    levels = proc_autophase.brute_levels([z.real for z in zs], [z.imag for z in zs], angles)
    for k, z in enumerate(zs):
        u, v = z.real.copy(), z.imag.copy()
        n = max(1, int(len(u) / 5000))
        for m, a in enumerate(angles):
            V, _ = proc_autophase.ps2(u, v, a, 0.0)
            err = np.sqrt((V[:n].mean() - V[-n:].mean()) ** 2)
            if np.max(V) > abs(np.min(V)):
                assert levels[k, m] == err, (k, m, levels[k, m], err)
            else:
                assert np.isnan(levels[k, m]), (k, m)
    rec.save("levels", levels)
    given = proc_autophase.brute_levels([z.real for z in zs], [z.imag for z in zs], angles, n=[1, 3, 1, 4, 1])      # (d_n uploaded)
    assert np.array_equal(given[0], levels[0], equal_nan=True) and np.array_equal(given[1], levels[1], equal_nan=True)
    rec.save("levels_n", given)


# ---- the driver --------------------------------------------------------------------------------------------------------
def run_area(area, out):
    from nmrfit_amd import _cabi
    assert area in AREAS, area
    assert _cabi.device_count() >= 1, "no HIP device: the HIP path has no fallback"
    rec = Record()
    # NMRFIT_POISON_KEEP_GOING=1 (by hand, when a build is known to be wrong: which cases notice?): a case that fails is
    # reported and the next one runs; the process still exits with 1 and writes no file
    keep_going = os.environ.get("NMRFIT_POISON_KEEP_GOING") == "1"
    failed = []
    with nan_outputs():
        for name, fn in CASES[area]:
            rec.begin(name)
            try:
                fn(rec)
            except Exception as e:
                if not keep_going:
                    raise
                failed.append(name)
                print("poison_support: %s/%s FAILED: %s: %s" % (area, name, type(e).__name__, str(e).splitlines()[0][:300] if str(e) else ""),
                      flush=True)
                continue
            print("poison_support: %s/%s ran (%d arrays so far)" % (area, name, len(rec.arrays)), flush=True)
    assert rec.ran == case_names(area)
    if failed:
        raise SystemExit("poison_support: %d of %d cases of %s failed: %s" % (len(failed), len(rec.ran), area, ", ".join(failed)))
    np.savez(out, __cases__=np.array(rec.ran), __poison__=np.array(os.environ.get("NMRFIT_POISON_ALLOC", "")), **rec.arrays)
    return rec


def main(argv):
    if len(argv) != 3 or argv[1] not in AREAS:
        print("usage: python -m tests.poison_support {%s} OUT.npz" % "|".join(AREAS), file=sys.stderr)
        return 2
    run_area(argv[1], argv[2])
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))

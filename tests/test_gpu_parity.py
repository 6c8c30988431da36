"""
GPU tier (ii): the HIP path, called through the C-ABI (ctypes -> libnmrfit_amd.so), against
(1) the golden vectors the reference produced and (2) the oracle on seeded inputs.

Tolerance: north_star asks for 1e-6 relative on the objective.  The fp64 kernel is held to
RTOL_F = 1e-9 here (observed ~1e-13), i.e. three orders inside the bar.  Where f -> 0 a
relative test is meaningless, so |df| <= RTOL_F * max(f, F_FLOOR).
"""
import os

import numpy as np
import pytest

from nmrfit_amd import _cabi, synth

pytestmark = pytest.mark.gpu

RTOL_F = 1e-9
F_FLOOR = 1e-6
# the kernels of the loaded library: DEFAULT / FARFIELD / NOREC in the product build; with NMRFIT_LIB pointing at the
# A/B library (nmrfit_amd/csrc/build.sh --ab) also BASELINE, NOSKIP
VARIANTS = _cabi.available_variants()
HAS_AB = _cabi.has_ab_variants()
# the plainest kernel at hand to check the tuned ones against: IEEE divide + libdevice exp2 per unit (A/B build), else
# the general form without recurrence or scaled pairs
REFERENCE_VARIANT = _cabi.VARIANT_BASELINE if HAS_AB else _cabi.VARIANT_NOREC


def _close_f(f, ref, rtol=RTOL_F):
    f, ref = np.asarray(f), np.asarray(ref)
    tol = rtol * np.maximum(np.abs(ref), F_FLOOR)
    bad = np.abs(f - ref) > tol
    assert not bad.any(), "max rel err %.3g at %s" % (
        np.max(np.abs(f - ref) / np.maximum(np.abs(ref), F_FLOOR)), np.nonzero(bad)[0][:5])


@pytest.fixture(scope="module")
def eq():
    from nmrfit_amd import equations
    assert _cabi.device_count() >= 1, "no HIP device: the HIP path has no fallback"
    info = _cabi.device_info(0)
    assert info["arch"].startswith("gfx950"), info
    return equations


def _load(golden_dir, name):
    return np.load(os.path.join(golden_dir, name), allow_pickle=False)


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("name", ["objective_P6_N4096.npz", "objective_P12_N16384.npz"])
def test_golden_objective_and_residual(eq, golden_dir, name, variant):
    g = _load(golden_dir, name)
    with eq.Evaluator(g["w"], g["u"], g["v"], g["weights"]) as ev:
        ev.set_variant(variant)
        f = ev.objective_batch(g["X"])
        _close_f(f, g["f"])
        rows = g["R_rows"]
        R, fR = ev.residual_batch(g["X"][rows], return_f=True)
        scale = np.abs(g["R"]).max()
        np.testing.assert_allclose(R, g["R"], rtol=0, atol=1e-11 * scale)
        _close_f(fR, g["f"][rows])
        # f is the RMS of the residual row
        _close_f(np.sqrt(np.mean(R * R, axis=1)), g["f"][rows])


@pytest.mark.parametrize("variant", VARIANTS)
def test_golden_c3_shape(eq, golden_dir, variant):
    g = _load(golden_dir, "objective_P24_N65536.npz")
    sp = synth.make_spectrum(65536, 24, seed=int(g["seed"]))
    with eq.Evaluator(sp["w"], sp["u"], sp["v"], sp["weights"]) as ev:
        ev.set_variant(variant)
        _close_f(ev.objective_batch(g["X"]), g["f"])


@pytest.mark.parametrize("variant", VARIANTS)
def test_golden_edge_cases(eq, golden_dir, variant):
    """Ragged N (1, 2, 63, 64, 65, 257, 1000), P = 0/1/3, non-uniform grids crossing zero,
    needle / very wide lines, loc outside the grid, |phase| up to 1e3, r outside [0,1]."""
    g = _load(golden_dir, "objective_edge_cases.npz")
    for i in range(int(g["n_cases"])):
        k = "e%d" % i
        w, u, v, wt, x = g[k + "_w"], g[k + "_u"], g[k + "_v"], g[k + "_wt"], g[k + "_x"]
        with eq.Evaluator(w, u, v, wt) as ev:
            ev.set_variant(variant)
            f = ev.objective_batch(x)
            R = ev.residual_batch(x)
        # phases of ~1e3 rad: the reference itself carries ~1e-13 abs error in phi there
        _close_f(f, [float(g[k + "_f"])], rtol=1e-9)
        np.testing.assert_allclose(R[0], g[k + "_R"], rtol=0,
                                   atol=1e-10 * max(1.0, np.abs(g[k + "_R"]).max()), err_msg=k)


def test_scalar_shim_matches_reference_signature(eq, golden_dir):
    g = _load(golden_dir, "objective_P6_N4096.npz")
    f0 = eq.objective(list(g["X"][3]), g["w"], g["u"], g["v"], g["weights"])
    assert isinstance(f0, float)
    _close_f([f0], [g["f"][3]])
    # negative-stride views, as nmrfit.load hands out (core.py:60): reversing all four arrays
    # changes the phase ramp index, so compare against the oracle on the same reversed views
    from oracle import c_oracle
    wr, ur, vr, wtr = g["w"][::-1], g["u"][::-1], g["v"][::-1], g["weights"][::-1]
    f1 = eq.objective(g["X"][3], wr, ur, vr, wtr)
    _close_f([f1], c_oracle.objective_batch(g["X"][3], wr, ur, vr, wtr))
    with pytest.raises(ValueError):
        eq.objective(g["X"][3], g["w"], g["u"], g["v"], g["weights"], fit_im="nonsense")


@pytest.mark.parametrize("S", [1, 3, 50, 204, 1024, 5000])
def test_against_oracle_swarm_sizes(eq, S):
    """Every segmentation regime (split grid for small S, one wave per particle for large)."""
    from oracle import c_oracle
    sp = synth.make_spectrum(4096, 6, seed=21)
    X = synth.make_swarm(sp["lower"], sp["upper"], S, seed=22, x_true=sp["x_true"])
    ref = c_oracle.objective_batch(X, sp["w"], sp["u"], sp["v"], sp["weights"], threads=8)
    with eq.Evaluator(sp["w"], sp["u"], sp["v"], sp["weights"]) as ev:
        f = ev.objective_batch(X)
        geom = ev.last_launch()
    _close_f(f, ref)
    assert geom["waves"] == S * geom["segments"]


@pytest.mark.parametrize("N", [100, 511, 512, 513, 1536, 7777])
def test_against_oracle_ragged_grids(eq, N):
    from oracle import c_oracle
    sp = synth.make_spectrum(N, 5, seed=31)
    X = synth.make_swarm(sp["lower"], sp["upper"], 37, seed=32, x_true=sp["x_true"])
    ref_R, ref_f = c_oracle.residual_batch(X, sp["w"], sp["u"], sp["v"], sp["weights"], threads=8)
    with eq.Evaluator(sp["w"], sp["u"], sp["v"], sp["weights"]) as ev:
        f = ev.objective_batch(X)
        R = ev.residual_batch(X)
    _close_f(f, ref_f)
    np.testing.assert_allclose(R, ref_R, rtol=0, atol=1e-11 * np.abs(ref_R).max())


def test_empty_batch_and_errors(eq):
    sp = synth.make_spectrum(256, 2, seed=1)
    with eq.Evaluator(sp["w"], sp["u"], sp["v"], sp["weights"]) as ev:
        f = ev.objective_batch(np.zeros((0, 10)))
        assert f.shape == (0,)
        with pytest.raises(ValueError):
            ev.objective_batch(np.zeros((2, 9)))          # 9 != 4 + 3P
        if HAS_AB:
            ev.set_variant(_cabi.VARIANT_BASELINE)       # fit_im exists for DEFAULT / NOREC / FARFIELD
            with pytest.raises(eq.NmrfitError) as ei:
                ev.objective_batch(sp["x_true"][None, :], fit_im=True)
            assert ei.value.code == _cabi.E_UNSUPPORTED
        else:                                            # the product library does not have the A/B kernels at all
            with pytest.raises(eq.NmrfitError) as ei:
                ev.set_variant(_cabi.VARIANT_BASELINE)
            assert ei.value.code == _cabi.E_UNSUPPORTED
    with pytest.raises(ValueError):
        eq.Evaluator(sp["w"], sp["u"][:-1], sp["v"], sp["weights"])
    with pytest.raises(eq.NmrfitError) as ei:
        eq.Evaluator(sp["w"], sp["u"], sp["v"], sp["weights"], device=99)
    assert ei.value.code == _cabi.E_NO_DEVICE


def test_set_weights_and_linearity(eq):
    """Size-independent properties: f scales linearly with the weights; with unit weights and
    P = 0 the objective is the RMS of the rotated real part, and rotating by p0 then -p0
    composes (|u + i v| is preserved)."""
    from oracle import c_oracle
    sp = synth.make_spectrum(2048, 4, seed=41)
    X = synth.make_swarm(sp["lower"], sp["upper"], 16, seed=42)
    with eq.Evaluator(sp["w"], sp["u"], sp["v"], sp["weights"]) as ev:
        f1 = ev.objective_batch(X)
        ev.set_weights(3.0 * sp["weights"])
        f3 = ev.objective_batch(X)
        np.testing.assert_allclose(f3, 3.0 * f1, rtol=1e-13)
        ev.set_weights(np.ones(2048))
        x0 = np.array([[0.7, 0.0, 0.5, 0.0], [0.7 + np.pi / 2, 0.0, 0.5, 0.0]])
        R = ev.residual_batch(x0)                      # rows: Re and (shifted by 90 deg) -Im
        np.testing.assert_allclose(R[0] ** 2 + R[1] ** 2, sp["u"] ** 2 + sp["v"] ** 2, rtol=1e-12)
        ref = c_oracle.objective_batch(x0, sp["w"], sp["u"], sp["v"], np.ones(2048))
        _close_f(ev.objective_batch(x0), ref)


def test_full_size_c3_properties(eq):
    """BASELINE config C3 at full size (S=4096, N=65536, P=24): size-independent checks --
    (a) every 97th particle against the oracle, (b) determinism (bitwise equal reruns),
    (c) default vs baseline variant agree to 1e-11, (d) permuting particles permutes f."""
    from oracle import c_oracle
    sp, X = synth.make_workload("C3")
    with eq.Evaluator(sp["w"], sp["u"], sp["v"], sp["weights"]) as ev:
        f = ev.objective_batch(X)
        f2 = ev.objective_batch(X)
        np.testing.assert_array_equal(f, f2)
        idx = np.arange(0, X.shape[0], 97)
        ref = c_oracle.objective_batch(X[idx], sp["w"], sp["u"], sp["v"], sp["weights"], threads=16)
        _close_f(f[idx], ref)
        perm = np.random.default_rng(0).permutation(X.shape[0])
        np.testing.assert_array_equal(ev.objective_batch(X[perm]), f[perm])
        ev.set_variant(REFERENCE_VARIANT)
        fb = ev.objective_batch(X[:512])
        np.testing.assert_allclose(f[:512], fb, rtol=1e-11)
        assert np.isfinite(f).all() and f[0] == f.min()       # row 0 is the generating vector


def test_objective_is_independent_of_launch_geometry(eq):
    """The sum of squares is accumulated in one canonical order (lane, wave tree, chunks in
    grid order), so a particle's f is bit-identical whether its grid is cut into 8 segments
    (small batch), 4 (medium) or handled by one wave (large batch) -- which is what makes a
    sharded swarm reproduce the single-GPU swarm exactly."""
    sp = synth.make_spectrum(4096, 6, seed=51)
    X = synth.make_swarm(sp["lower"], sp["upper"], 20000, seed=52, x_true=sp["x_true"])
    with eq.Evaluator(sp["w"], sp["u"], sp["v"], sp["weights"]) as ev:
        f_big = ev.objective_batch(X)
        g_big = ev.last_launch()
        f_mid = ev.objective_batch(X[:3000])
        g_mid = ev.last_launch()
        f_one = np.concatenate([ev.objective_batch(X[i:i + 1]) for i in (0, 1, 2999)])
        g_one = ev.last_launch()
        fi_big = ev.objective_batch(X[:17000], fit_im="sum")
        fi_small = ev.objective_batch(X[:7], fit_im="sum")
    assert g_big["segments"] == 1 and g_mid["segments"] > 1 and g_one["segments"] > g_mid["segments"]
    np.testing.assert_array_equal(f_mid, f_big[:3000])
    np.testing.assert_array_equal(f_one, f_big[[0, 1, 2999]])
    np.testing.assert_array_equal(fi_small, fi_big[:7])


@pytest.mark.parametrize("variant", ["default", "farfield", "norec"])
def test_four_segment_workgroup_reduction_matches_the_other_geometries(eq, variant):
    """Four segments per particle: the four waves of a workgroup ARE the particle, its block sums meet in
    LDS and the workgroup writes f itself (round 3; no partial-sum buffer, no finalize pass).  Same canonical
    summation order as one wave per particle (20000 particles) and as eight segments with finalize_kernel
    (60 particles): bit-identical f, in every fit_im mode."""
    sp = synth.make_spectrum(4096, 6, seed=51)
    X = synth.make_swarm(sp["lower"], sp["upper"], 20000, seed=52, x_true=sp["x_true"])
    with eq.Evaluator(sp["w"], sp["u"], sp["v"], sp["weights"]) as ev:
        ev.set_variant(_cabi.variant_id(variant))
        for mode in (False, True, "sum"):
            f_one = ev.objective_batch(X, fit_im=mode)
            assert ev.last_launch()["segments"] == 1
            f_four = ev.objective_batch(X[:1200], fit_im=mode)
            assert ev.last_launch()["segments"] == 4
            f_eight = ev.objective_batch(X[:60], fit_im=mode)
            assert ev.last_launch()["segments"] == 8
            # eight segments: ONE eight-wave workgroup per particle (round 4; objective launches without the
            # imaginary channel of the kernels fit() selects), block sums through LDS like the four-wave form
            wide = mode is False and variant in ("default", "farfield", "norec")
            assert ev.last_launch()["waves_per_workgroup"] == (8 if wide else 4)
            np.testing.assert_array_equal(f_four, f_one[:1200], err_msg=str(mode))
            np.testing.assert_array_equal(f_eight, f_one[:60], err_msg=str(mode))
        R = ev.residual_batch(X[:1200][:8])          # (residual rows are a small batch: eight segments)
        Rb = ev.residual_batch(X[:3])
        np.testing.assert_array_equal(Rb, R[:3])


@pytest.mark.parametrize("P", [9, 64, 65, 130, 960])
def test_many_peaks(eq, P):
    """More peaks than a 64-peak window-mask block (P = 65, 130), group tails of every size and
    the LDS limit (P = 960 -> one workgroup per CU)."""
    from oracle import c_oracle
    N = 1500 if P < 960 else 600
    sp = synth.make_spectrum(N, P, seed=61)
    X = synth.make_swarm(sp["lower"], sp["upper"], 9, seed=62, x_true=sp["x_true"])
    ref_R, ref_f = c_oracle.residual_batch(X, sp["w"], sp["u"], sp["v"], sp["weights"], threads=8)
    with eq.Evaluator(sp["w"], sp["u"], sp["v"], sp["weights"]) as ev:
        for variant in [v for v in (_cabi.VARIANT_DEFAULT, _cabi.VARIANT_NOSKIP, _cabi.VARIANT_BASELINE, _cabi.VARIANT_FARFIELD,
                                    _cabi.VARIANT_NOREC) if v in VARIANTS]:
            ev.set_variant(variant)
            _close_f(ev.objective_batch(X), ref_f)
        ev.set_variant(_cabi.VARIANT_DEFAULT)
        R = ev.residual_batch(X[:2])
    np.testing.assert_allclose(R, ref_R[:2], rtol=0, atol=1e-11 * np.abs(ref_R).max())
    if P == 960:
        with eq.Evaluator(sp["w"], sp["u"], sp["v"], sp["weights"]) as ev:
            with pytest.raises(eq.NmrfitError) as ei:
                ev.objective_batch(np.zeros((1, 4 + 3 * 961)))
            assert ei.value.code == _cabi.E_INVALID and "960 peaks" in str(ei.value)


def test_non_finite_parameters_do_not_crash(eq):
    """width = 0, NaN and inf parameters: the reference returns nan/inf (with numpy warnings);
    the kernel must return a non-finite value for those particles and leave the others alone."""
    sp = synth.make_spectrum(1024, 3, seed=71)
    X = synth.make_swarm(sp["lower"], sp["upper"], 6, seed=72, x_true=sp["x_true"])
    good = X.copy()
    X[1, 4] = 0.0            # width 0
    X[2, 5] = np.nan         # loc NaN
    X[3, 6] = np.inf         # area inf
    X[4, 0] = np.nan         # p0 NaN
    with eq.Evaluator(sp["w"], sp["u"], sp["v"], sp["weights"]) as ev:
        for variant in VARIANTS:
            ev.set_variant(variant)
            f = ev.objective_batch(X)
            f_good = ev.objective_batch(good)
            assert np.isfinite(f[[0, 5]]).all() and (f[[0, 5]] == f_good[[0, 5]]).all(), variant
            assert not np.isfinite(f[1:5]).any(), variant


def test_context_churn_does_not_leak(eq):
    """Contexts that come and go (one per fitted spectrum) while another stays: the library recycles a closed
    context's idle HIP stream for the next one on the device (a new stream costs ~4 ms at first use, a default fit
    ~25 ms; csrc/host_call.hip) -- never a stream that a live context still owns."""
    sp = synth.make_spectrum(4096, 2, seed=81)
    X = synth.make_swarm(sp["lower"], sp["upper"], 8, seed=82)
    sp2 = synth.make_spectrum(3000, 5, seed=83)
    X2 = synth.make_swarm(sp2["lower"], sp2["upper"], 40, seed=84)
    f0 = None
    with eq.Evaluator(sp2["w"], sp2["u"], sp2["v"], sp2["weights"]) as stays:
        g0 = stays.objective_batch(X2)
        for it in range(200):
            with eq.Evaluator(sp["w"], sp["u"], sp["v"], sp["weights"]) as ev:
                d2 = stays.dev_alloc(X2.nbytes) if it % 7 == 0 else None      # (work queued on the long-lived context's stream
                f = ev.objective_batch(X)                                      # while the short-lived one runs on its own)
                np.testing.assert_array_equal(stays.objective_batch(X2), g0)
                if d2 is not None:
                    stays.dev_free(d2)
            f0 = f if f0 is None else f0
            np.testing.assert_array_equal(f, f0)


def test_farfield_variant_full_size_and_geometry(eq):
    """The opt-in far-field variant at BASELINE's C3 size: every particle agrees with the direct
    kernel to 1e-12 relative (observed ~1e-15), and it is segmentation-independent too."""
    sp, X = synth.make_workload("C3")
    with eq.Evaluator(sp["w"], sp["u"], sp["v"], sp["weights"]) as ev:
        f = ev.objective_batch(X)
        ev.set_variant(_cabi.VARIANT_FARFIELD)
        ff = ev.objective_batch(X)
        np.testing.assert_allclose(ff, f, rtol=1e-12)
        ff_small = ev.objective_batch(X[:5])
        assert ev.last_launch()["segments"] > 4
        np.testing.assert_array_equal(ff_small, ff[:5])
        R = ev.residual_batch(X[:2])
        ev.set_variant(REFERENCE_VARIANT)
        Rb = ev.residual_batch(X[:2])
    np.testing.assert_allclose(R, Rb, rtol=0, atol=1e-14 * np.abs(Rb).max())


def test_float32_spectra_as_nmrglue_delivers_them(eq):
    """nmrfit.load hands out float32 u, v (complex64 FFT output) as reversed views (core.py:52-60).
    The reference then rotates in complex64 (proc_autophase.py:29-32); the ABI upcasts to float64.
    The two differ by the float32 rounding of the rotation only: 1e-9 ... 2e-7 relative on f (largest
    where f is small), inside the 1e-6 bar; asserted at 5e-7 against the numpy oracle running the
    reference's float32 path."""
    from oracle import nmrfit_oracle as onp
    sp = synth.make_spectrum(4096, 6, seed=1)
    X = synth.make_swarm(sp["lower"], sp["upper"], 5, seed=2, x_true=sp["x_true"])
    u32, v32 = sp["u"].astype(np.float32)[::-1], sp["v"].astype(np.float32)[::-1]
    w, wt = sp["w"][::-1], sp["weights"][::-1]
    ref = np.array([onp.objective(X[i], w, u32, v32, wt) for i in range(5)])
    with eq.Evaluator(w, u32, v32, wt) as ev:
        f = ev.objective_batch(X)
    np.testing.assert_allclose(f, ref, rtol=5e-7)


def test_float32_spectra_against_the_reference_golden(eq, golden_dir):
    """The same against the REFERENCE's own values (tests/golden/objective_float32.npz, generated by
    oracle/make_golden.py from the reference's complex64 path): the generating parameters, eight
    near-optimum particles -- where f is smallest and the relative gap of the float64 upcast largest --
    and three random ones, at the C1/C2, C5 and C3 shapes, with the DEFAULT and the FARFIELD kernel.
    north_star's bar is 1e-6 relative; asserted at 5e-7 (observed <= 1.2e-7)."""
    import os
    d = np.load(os.path.join(golden_dir, "objective_float32.npz"))
    worst = 0.0
    for tag in ("P6_N4096", "P12_N16384", "P24_N65536"):
        N, P, seed = (int(t) for t in d[tag + "_shape"])
        sp = synth.make_spectrum(N, P, seed=seed)
        u32, v32 = sp["u"].astype(np.float32), sp["v"].astype(np.float32)
        X, ref = d[tag + "_X"], d[tag + "_f"]
        with eq.Evaluator(sp["w"], u32, v32, sp["weights"]) as ev:
            for variant in (_cabi.VARIANT_DEFAULT, _cabi.VARIANT_FARFIELD):
                ev.set_variant(variant)
                f = ev.objective_batch(X)
                np.testing.assert_allclose(f, ref, rtol=5e-7)
                worst = max(worst, float(np.max(np.abs(f - ref) / ref)))
    print("float32 spectra vs reference golden: worst relative difference %.2e" % worst)


def test_large_shapes(eq):
    """A million-point grid and a 200k-particle swarm: 64-bit indexing, block table, multi-pass
    launches.  Sampled particles against the oracle."""
    from oracle import c_oracle
    sp = synth.make_spectrum(1 << 20, 40, seed=91)
    X = synth.make_swarm(sp["lower"], sp["upper"], 600, seed=92, x_true=sp["x_true"])
    with eq.Evaluator(sp["w"], sp["u"], sp["v"], sp["weights"]) as ev:
        f = ev.objective_batch(X)
        ev.set_variant(_cabi.VARIANT_FARFIELD)
        ff = ev.objective_batch(X)
    idx = np.array([0, 1, 299, 599])
    ref = c_oracle.objective_batch(X[idx], sp["w"], sp["u"], sp["v"], sp["weights"], threads=16)
    _close_f(f[idx], ref)
    np.testing.assert_allclose(ff, f, rtol=1e-12)
    sp = synth.make_spectrum(4096, 6, seed=93)
    X = synth.make_swarm(sp["lower"], sp["upper"], 200000, seed=94, x_true=sp["x_true"])
    with eq.Evaluator(sp["w"], sp["u"], sp["v"], sp["weights"]) as ev:
        f = ev.objective_batch(X)
    idx = np.arange(0, 200000, 9973)
    ref = c_oracle.objective_batch(X[idx], sp["w"], sp["u"], sp["v"], sp["weights"], threads=16)
    _close_f(f[idx], ref)
    assert np.isfinite(f).all()


def test_randomized_shapes_and_parameters(eq):
    """300 random cases: N in [1, 5000] (non-uniform, unsorted and reversed grids included),
    P in [0, 70], widths from needles to wider than the grid, lines on and off the grid, phases
    up to +-60 rad; every kernel variant against the plain-C oracle."""
    from oracle import c_oracle
    rng = np.random.default_rng(20261003)
    worst = 0.0
    for case in range(300):
        N = int(rng.integers(1, 5001)) if case % 7 else int(rng.choice([1, 2, 63, 64, 65, 511, 512, 513, 1024, 4097]))
        P = int(rng.integers(0, 71)) if case % 5 else int(rng.choice([0, 1, 7, 8, 9, 15, 16, 17, 63, 64, 65]))
        S = int(rng.integers(1, 12))
        kind = case % 4
        if kind == 0:
            w = np.linspace(rng.uniform(-5, 5), rng.uniform(6, 12), N)
        elif kind == 1:
            w = np.sort(rng.uniform(-3.0, 9.0, N))
        elif kind == 2:
            w = np.linspace(8.0, -2.0, N)                       # descending, as nmrfit.load delivers
        else:
            w = rng.uniform(0.0, 4.0, N)                          # unsorted
        span = max(float(np.ptp(w)), 1.0)
        u, v = rng.standard_normal(N), rng.standard_normal(N)
        wt = 0.25 + rng.random(N)
        X = np.empty((S, 4 + 3 * P))
        X[:, 0] = rng.uniform(-60, 60, S)
        X[:, 1] = rng.uniform(-60, 60, S)
        X[:, 2] = rng.uniform(-0.2, 1.2, S)
        X[:, 3] = rng.uniform(-0.05, 0.05, S)
        X[:, 4::3] = span * 10.0 ** rng.uniform(-5, 0.5, (S, P))  # widths: needles ... wider than the grid
        X[:, 5::3] = rng.uniform(w.min() - 0.2 * span, w.max() + 0.2 * span, (S, P))
        X[:, 6::3] = rng.uniform(-1.0, 3.0, (S, P))
        ref = c_oracle.objective_batch(X, w, u, v, wt, threads=4)
        with eq.Evaluator(w, u, v, wt) as ev:
            for variant in VARIANTS:
                ev.set_variant(variant)
                f = ev.objective_batch(X)
                err = np.max(np.abs(f - ref) / np.maximum(np.abs(ref), F_FLOOR))
                worst = max(worst, err)
                assert err <= RTOL_F, (case, N, P, S, kind, variant, err)
    assert worst < 1e-10, worst


def test_contexts_on_concurrent_host_threads(eq):
    """include/nmrfit_amd.h: 'different contexts may be driven from different host threads'.
    Six threads, one context (own stream, own workspaces) each, different spectra and shapes,
    interleaved calls; every result equals the same call made serially."""
    import threading
    jobs = []
    for t in range(6):
        sp = synth.make_spectrum(1500 + 700 * t, 2 + 3 * t, seed=40 + t)
        X = synth.make_swarm(sp["lower"], sp["upper"], 30 + 25 * t, seed=50 + t)
        with eq.Evaluator(sp["w"], sp["u"], sp["v"], sp["weights"]) as ev:
            want_f, want_r = ev.objective_batch(X), ev.residual_batch(X[:3])
        jobs.append((sp, X, want_f, want_r))
    errors = []
    start = threading.Barrier(len(jobs))

    def work(sp, X, want_f, want_r):
        try:
            with eq.Evaluator(sp["w"], sp["u"], sp["v"], sp["weights"]) as ev:
                start.wait()
                for it in range(40):
                    np.testing.assert_array_equal(ev.objective_batch(X), want_f)
                    if it % 8 == 0:
                        np.testing.assert_array_equal(ev.residual_batch(X[:3]), want_r)
        except BaseException as e:      # surfaced in the main thread below
            errors.append(e)

    threads = [threading.Thread(target=work, args=j) for j in jobs]
    for th in threads:
        th.start()
    for th in threads:
        th.join(120)
    assert not errors, errors[0]
    assert not any(th.is_alive() for th in threads)


def test_source_derived_properties_on_the_gpu(eq):
    """SURVEY section 4, properties 1-4, asserted on the HIP path itself (no oracle involved)."""
    from nmrfit_amd import proc_autophase
    # 1. voigt is area-normalised: the per-peak real contribution integrates to `a`
    w = np.linspace(-2000.0, 2000.0, 2_000_001)
    zeros = np.zeros_like(w)
    with eq.Evaluator(w, zeros, zeros, np.ones_like(w)) as ev:
        for r in (0.0, 0.4, 1.0):
            real, _ = ev.contributions(np.array([0.0, 0.0, r, 0.0, 0.7, 0.3, 2.5]))
            area = np.sum(0.5 * (real[0][1:] + real[0][:-1]) * np.diff(w))
            assert area == pytest.approx(2.5, abs=2.5 * r * 0.7 / (np.pi * 2000) * 1.1 + 1e-9)
    # 2. ps2 round trip: rotating by (p0, p1) and back returns the data
    sp = synth.make_spectrum(4096, 6, seed=1, noise=0.0)
    V, I = proc_autophase.ps2(sp["u"], sp["v"], 0.7, -1.3)
    ub, vb = proc_autophase.ps2(V, I, 0.7, -1.3, inv=True)
    np.testing.assert_allclose(ub, sp["u"], atol=1e-15)
    np.testing.assert_allclose(vb, sp["v"], atol=1e-15)
    with eq.Evaluator(sp["w"], sp["u"], sp["v"], sp["weights"]) as ev:
        # 3. the objective of a noiseless spectrum at its generating parameters is rounding noise
        assert ev.objective_batch(sp["x_true"])[0] < 1e-14
        X = synth.make_swarm(sp["lower"], sp["upper"], 8, seed=6)
        f0 = ev.objective_batch(X)
    # 4. invariant to shifting w and every loc together ...
    X2 = X.copy()
    X2[:, 5::3] += 0.25
    with eq.Evaluator(sp["w"] + 0.25, sp["u"], sp["v"], sp["weights"]) as ev:
        np.testing.assert_allclose(ev.objective_batch(X2), f0, rtol=1e-10)
    # ... but not to reversing the arrays: the phase ramp runs over the array index (proc_autophase.py:30-31)
    with eq.Evaluator(sp["w"][::-1], sp["u"][::-1], sp["v"][::-1], sp["weights"][::-1]) as ev:
        f_rev = ev.objective_batch(X)
    assert not np.allclose(f_rev, f0, rtol=1e-3)
    Xr = X.copy()
    Xr[:, 0] = X[:, 0] + X[:, 1] * (1.0 - 1.0 / sp["w"].size)    # ramp reversed: phi'_j = p0 + p1 (N-1-j)/N
    Xr[:, 1] = -X[:, 1]
    with eq.Evaluator(sp["w"][::-1], sp["u"][::-1], sp["v"][::-1], sp["weights"][::-1]) as ev:
        np.testing.assert_allclose(ev.objective_batch(Xr), f0, rtol=1e-10)


def test_gaussian_recurrence_against_point_by_point(eq):
    """DEFAULT runs the in-window Gaussians of a uniformly spaced grid by recurrence; NOREC is the
    same kernel with one exp2 per point.  Scan line widths across the |d| <= 2 switch (d = 64 grid
    steps in half-widths), ascending / descending / jittered / non-uniform grids, pure Gaussians
    (r = 0, the worst case for the recurrence) and the ragged tail: f agrees to 1e-12."""
    from oracle import c_oracle
    rng = np.random.default_rng(8)
    N = 40000 + 77                                   # ragged tail chunk
    grids = {
        "ascending": np.linspace(3.0, 4.0, N),
        "descending": np.linspace(4.0, 3.0, N),
        "jitter 1e-9 of a step": np.linspace(3.0, 4.0, N) + 1e-9 / N * rng.standard_normal(N),
        "non-uniform": np.sort(rng.uniform(3.0, 4.0, N)),
        "far from zero": np.linspace(3.0e3, 3.0e3 + 1.0, N),
    }
    step = 1.0 / (N - 1)
    for name, w in grids.items():
        u, v = rng.standard_normal(N), rng.standard_normal(N)
        wt = 0.5 + rng.random(N)
        P, S = 9, 12
        X = np.empty((S, 4 + 3 * P))
        X[:, 0:2] = rng.uniform(-1, 1, (S, 2))
        X[:, 2] = np.linspace(0.0, 1.0, S)                       # from pure Gaussian to pure Lorentzian
        X[:, 3] = 0.001
        # widths from 8 to 4000 grid steps: d = 128 step / width runs from 16 down to 0.03
        X[:, 4::3] = step * 2.0 ** rng.uniform(3, 12, (S, P))
        X[:, 5::3] = rng.uniform(w.min(), w.max(), (S, P))
        X[:, 6::3] = rng.uniform(0.5, 2.0, (S, P)) * X[:, 4::3] * 100
        with eq.Evaluator(w, u, v, wt) as ev:
            f = ev.objective_batch(X)
            ev.set_variant(_cabi.VARIANT_FARFIELD)
            ff = ev.objective_batch(X)
            ev.set_variant(_cabi.VARIANT_NOREC)
            f_direct = ev.objective_batch(X)
            Rrow = ev.residual_batch(X[:2])
            ev.set_variant(_cabi.VARIANT_DEFAULT)
            # rows are always evaluated point by point: DEFAULT and NOREC differ only by the
            # pair form of the Lorentzian groups (rounding)
            np.testing.assert_allclose(ev.residual_batch(X[:2]), Rrow, rtol=0, atol=1e-13 * np.abs(Rrow).max())
        np.testing.assert_allclose(f, f_direct, rtol=1e-12, err_msg=name)
        np.testing.assert_allclose(ff, f_direct, rtol=1e-12, err_msg=name)
        ref = c_oracle.objective_batch(X, w, u, v, wt, threads=8)
        _close_f(f, ref)
        if name == "non-uniform":
            np.testing.assert_allclose(f, f_direct, rtol=1e-13)                  # the recurrence is off



def adversarial_case(case):
    """Spectra where the far-field variant's premise fails or is stressed (see
    test_farfield_adversarial_spectra); also used by tests/test_gpu_perf_guards.py."""
    N, P, S = 16384, 24, 256
    rng = np.random.default_rng(5)
    w = np.linspace(3.0, 4.0, N)
    u, v = rng.standard_normal(N) * 0.01, rng.standard_normal(N) * 0.01
    wt = 1.0 + rng.random(N)
    X = np.empty((S, 4 + 3 * P))
    X[:, 0] = rng.uniform(-np.pi, np.pi, S)
    X[:, 1] = rng.uniform(-np.pi, np.pi, S)
    X[:, 2] = rng.uniform(0, 1, S)
    X[:, 3] = rng.uniform(-0.01, 0.01, S)
    if case == "overlapping_broad":
        X[:, 4::3] = rng.uniform(0.3, 0.8, (S, P))              # widths comparable to the whole span
        X[:, 5::3] = rng.uniform(3.2, 3.8, (S, P))
        X[:, 6::3] = rng.uniform(0.001, 0.01, (S, P))
    elif case == "dense_cluster_1e12":
        X[:, 4::3] = rng.uniform(0.002, 0.006, (S, P))
        X[:, 5::3] = np.concatenate((rng.uniform(3.49, 3.51, (S, P - 4)), rng.uniform(3.05, 3.95, (S, 4))), axis=1)
        X[:, 6::3] = 10.0 ** rng.uniform(-12, 0, (S, P))
    else:
        X[:, 4::3] = 10.0 ** rng.uniform(-7, -5, (S, P))         # grid step is 6e-5
        X[:, 5::3] = rng.uniform(3.0, 4.0, (S, P))
        X[:, 6::3] = rng.uniform(0.001, 0.01, (S, P))
    return N, P, S, w, u, v, wt, X


@pytest.mark.parametrize("case", ["overlapping_broad", "dense_cluster_1e12", "needles_everywhere"])
def test_farfield_adversarial_spectra(eq, case):
    """The far-field variant where its premise fails or is stressed: (a) 24 broad overlapping lines
    -- NO peak is far from any chunk, everything takes the direct path; (b) a dense cluster whose
    amplitudes span twelve orders of magnitude next to far satellites; (c) needle-narrow lines
    (a fraction of a grid step wide) for which every chunk but one is far at huge |t|.  Parity
    with the C oracle at 1e-9 like every other variant, agreement with DEFAULT at 1e-12.  (The
    wall-clock side of it -- no slowdown where the expansion cannot help -- is a non-gating guard
    in tests/test_gpu_perf_guards.py.)"""
    from oracle import c_oracle
    N, P, S, w, u, v, wt, X = adversarial_case(case)
    ref = c_oracle.objective_batch(X, w, u, v, wt, threads=8)
    with eq.Evaluator(w, u, v, wt) as ev:
        f_def = ev.objective_batch(X)
        ev.set_variant(_cabi.VARIANT_FARFIELD)
        f_far = ev.objective_batch(X)
        R_far = ev.residual_batch(X[:3])
        ev.set_variant(_cabi.VARIANT_DEFAULT)
        R_def = ev.residual_batch(X[:3])
    _close_f(f_far, ref)
    _close_f(f_def, ref)
    # needles a fraction of a grid step wide: t = (w - loc)*(2/width) is conditioned like 1e-16 * 2e7 near a
    # core, so any two formulations (these two, or either and the oracle) agree to ~1e-10 only
    tight = 1e-9 if case == "needles_everywhere" else 1e-12
    np.testing.assert_allclose(f_far, f_def, rtol=tight)
    np.testing.assert_allclose(R_far, R_def, rtol=0, atol=(1e-9 if case == "needles_everywhere" else 1e-13) * np.abs(R_def).max())
    print("   vs oracle: default %.2e, farfield %.2e; farfield vs default %.2e" % (
        np.max(np.abs(f_def - ref) / ref), np.max(np.abs(f_far - ref) / ref), np.max(np.abs(f_far - f_def) / f_def)))


def test_farfield_as_context_default_runs_the_swarm(eq):
    """fit(options={"variant": "farfield"}): the swarm on the far-field kernel reaches the same
    optimum region as on the direct kernel (trajectories differ by rounding, so not bit for bit)."""
    import nmrfit_amd
    sp = synth.make_spectrum(8192, 6, seed=3)
    data = synth.SynthData(sp["w"], sp["u"], sp["v"], sp["peaks"])
    opts = {"swarmsize": 204, "maxiter": 300, "seed": 12}
    a = nmrfit_amd.fit(data, list(sp["lower"]), list(sp["upper"]), summary=False, options=opts)
    b = nmrfit_amd.fit(data, list(sp["lower"]), list(sp["upper"]), summary=False, options=dict(opts, variant="farfield"))
    assert b.error == pytest.approx(a.error, rel=0.05)
    for mode in (True, "sum"):
        c = nmrfit_amd.fit(data, list(sp["lower"]), list(sp["upper"]), fit_im=mode, summary=False,
                           options=dict(opts, maxiter=40, variant="farfield"))
        d = nmrfit_amd.fit(data, list(sp["lower"]), list(sp["upper"]), fit_im=mode, summary=False,
                           options=dict(opts, maxiter=40))
        assert np.isfinite(c.error) and c.error == pytest.approx(d.error, rel=0.2)


def test_mixed_precision_farfield_variant(eq):
    """NMRFIT_VARIANT_FARFIELD32 (opt-in): orders 1..15 of the far-field kernel's shared polynomial in packed
    fp32, everything else fp64.  Bar: 1e-8 relative on f against the fp64 kernels; measured <= 5e-12 --
    asserted at 1e-10 on the C3 workload, on a dense spectrum where every peak is near every chunk, and on the
    reference-generated C3-shape golden; residual rows of a context set to it are the fp64 far-field kernel's, bit for
    bit; fit() takes it by name."""
    import nmrfit_amd
    sp, X = synth.make_workload("C3")
    Xd = synth.make_dense_swarm(128, 24, seed=5, w_lo=float(sp["w"].min()), w_hi=float(sp["w"].max()))
    with eq.Evaluator(sp["w"], sp["u"], sp["v"], sp["weights"]) as ev:
        out = {}
        for v in (_cabi.VARIANT_DEFAULT, _cabi.VARIANT_FARFIELD, _cabi.VARIANT_FARFIELD32):
            ev.set_variant(v)
            out[v] = (ev.objective_batch(X[:1024]), ev.objective_batch(Xd), ev.objective_batch(X[:7]), ev.residual_batch(X[:2]))
        for k in range(3):
            ref = out[_cabi.VARIANT_DEFAULT][k]
            got = out[_cabi.VARIANT_FARFIELD32][k]
            assert np.max(np.abs(got - ref) / np.maximum(np.abs(ref), 1e-6)) < 1e-10
        assert not np.array_equal(out[_cabi.VARIANT_FARFIELD32][0], out[_cabi.VARIANT_FARFIELD][0])   # (it IS another kernel)
        np.testing.assert_array_equal(out[_cabi.VARIANT_FARFIELD32][0][:7], out[_cabi.VARIANT_FARFIELD32][2])   # geometry-independent
        np.testing.assert_array_equal(out[_cabi.VARIANT_FARFIELD32][3], out[_cabi.VARIANT_FARFIELD][3])         # residual rows: fp64
        # the imaginary channel of such a context runs the fp64 far-field kernel
        ev.set_variant(_cabi.VARIANT_FARFIELD)
        f_im = ev.objective_batch(X[:64], fit_im=True)
        ev.set_variant(_cabi.VARIANT_FARFIELD32)
        np.testing.assert_array_equal(ev.objective_batch(X[:64], fit_im=True), f_im)
    spf = synth.make_spectrum(16384, 12, seed=3)
    data = synth.SynthData(spf["w"], spf["u"], spf["v"], spf["peaks"])
    opts = {"seed": 11, "maxiter": 60, "swarmsize": 128}
    a = nmrfit_amd.fit(data, list(spf["lower"]), list(spf["upper"]), summary=False, options=dict(opts, variant="farfield"))
    b = nmrfit_amd.fit(data, list(spf["lower"]), list(spf["upper"]), summary=False, options=dict(opts, variant="farfield32"))
    assert b.error == pytest.approx(a.error, rel=1e-6)

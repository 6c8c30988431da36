"""
CPU tier: the C-ABI library loads and exports every symbol include/nmrfit_amd.h declares,
the ctypes table covers all of them, and -- with no GPU -- the product path fails loudly
instead of falling back to anything.  No compute calls here.
"""
import ctypes
import os
import re

import numpy as np
import pytest

from nmrfit_amd import _cabi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared_symbols(header="nmrfit_amd.h"):
    text = open(os.path.join(ROOT, "include", header)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(nmrfit_[a-z0-9_]+)\s*\(", text)))


def test_library_is_built_and_exports_every_declared_symbol():
    if not os.path.exists(_cabi.LIB_PATH):
        _cabi.build()
    L = ctypes.CDLL(_cabi.LIB_PATH)
    names = _declared_symbols() + _declared_symbols("nmrfit_amd_diag.h")
    assert len(names) >= 60
    for n in names:
        assert hasattr(L, n), "libnmrfit_amd.so does not export " + n


def test_ctypes_table_covers_header():
    """The product interface (include/nmrfit_amd.h: what a binding for the hot path binds) and the diagnostic one
    (include/nmrfit_amd_diag.h) against the two ctypes tables; the product header stays a thin interface."""
    names = set(_declared_symbols())
    bound = set(_cabi.SIGNATURES) | {"nmrfit_last_error"}
    assert names == bound, (names - bound, bound - names)
    assert len(names) <= 46, len(names)
    diag = set(_declared_symbols("nmrfit_amd_diag.h"))
    assert diag == set(_cabi.DIAG_SIGNATURES), (diag - set(_cabi.DIAG_SIGNATURES), set(_cabi.DIAG_SIGNATURES) - diag)
    assert not (names & diag)


def test_ab_variants_exist_in_the_ab_library_only():
    """The A/B kernel forms are not part of the product: the product library refuses them by name (no GPU needed:
    the check precedes any device work), the A/B library says what it is."""
    L = _cabi.lib()
    if os.environ.get("NMRFIT_LIB"):
        pytest.skip("another library is loaded through NMRFIT_LIB")
    assert L.nmrfit_diag_ab_build() == 0
    assert not _cabi.has_ab_variants() and _cabi.available_variants() == [0, 6, 7, 8]
    if os.path.exists(_cabi.AB_LIB_PATH):
        A = ctypes.CDLL(_cabi.AB_LIB_PATH)
        assert A.nmrfit_diag_ab_build() == 1


def test_abi_version():
    assert _cabi.lib().nmrfit_abi_version() == _cabi.ABI_VERSION


def test_no_silent_fallback_without_gpu():
    """On a box without a GPU every evaluation must raise; on a GPU box this test checks the
    invalid-device path instead."""
    from nmrfit_amd import equations
    w = np.linspace(0, 1, 64)
    if _cabi.device_count() == 0:
        with pytest.raises(equations.NmrfitError) as ei:
            equations.Evaluator(w, w, w, w)
        assert ei.value.code == _cabi.E_NO_DEVICE
        with pytest.raises(equations.NmrfitError):
            equations.objective(np.zeros(7), w, w, w, w)
    else:
        with pytest.raises(equations.NmrfitError) as ei:
            equations.Evaluator(w, w, w, w, device=1 << 20)
        assert ei.value.code == _cabi.E_NO_DEVICE


def test_argument_validation_needs_no_gpu():
    L = _cabi.lib()
    out = ctypes.c_void_p()
    rc = L.nmrfit_ctx_create(0, 0, None, None, None, None, ctypes.byref(out))
    assert rc == _cabi.E_INVALID
    assert b"N must be" in L.nmrfit_last_error()
    assert L.nmrfit_ctx_destroy(None) == _cabi.OK
    assert L.nmrfit_pso_destroy(None) == _cabi.OK


def test_product_package_never_imports_the_oracle():
    pkg = os.path.join(ROOT, "nmrfit_amd")
    for dirpath, _, files in os.walk(pkg):
        for fn in files:
            if fn.endswith((".py", ".hip", ".h", ".sh")):
                text = open(os.path.join(dirpath, fn)).read()
                assert "oracle" not in text.lower(), \
                    "%s mentions the oracle: product code must not depend on it" % fn


def test_product_package_never_imports_torch():
    """Nothing under nmrfit_amd/ imports torch (the gloo rehearsal of the CPU tests, TorchExchange, lives in
    tests/swarm_support.py since round 5)."""
    pkg = os.path.join(ROOT, "nmrfit_amd")
    for dirpath, _, files in os.walk(pkg):
        for fn in files:
            if fn.endswith(".py"):
                text = open(os.path.join(dirpath, fn)).read()
                for line in text.splitlines():
                    if re.match(r"^(import|from)\s+torch\b", line):
                        raise AssertionError("%s imports torch at module level" % fn)
                assert not re.search(r"^\s+(import|from)\s+torch\b", text, flags=re.M), fn
    import subprocess
    import sys
    code = "import sys; sys.path.insert(0, %r); import nmrfit_amd, nmrfit_amd.rendezvous; assert 'torch' not in sys.modules" % ROOT
    subprocess.run([sys.executable, "-c", code], check=True)


def test_comm_argument_validation_needs_no_gpu():
    L = _cabi.lib()
    out = ctypes.c_void_p()
    assert L.nmrfit_comm_create(None, 0, 1, None, ctypes.byref(out)) == _cabi.E_INVALID
    assert L.nmrfit_comm_destroy(None) == _cabi.OK
    assert L.nmrfit_comm_barrier(None) == _cabi.E_INVALID
    assert L.nmrfit_pso_step(None) == _cabi.E_INVALID
    assert L.nmrfit_prof_enable(None, 4) == _cabi.E_INVALID


def test_batch_argument_validation_needs_no_gpu():
    """nmrfit_batch_*: argument errors are reported before anything touches a device; without a GPU the creation itself
    fails loudly (NMRFIT_E_NO_DEVICE) -- there is no CPU path behind nmrfit_amd.fit_many either."""
    L = _cabi.lib()
    out = ctypes.c_void_p()
    assert L.nmrfit_batch_create(0, 0, 64, None, None, None, None, None, None, None, 8, None, 0, 0, ctypes.byref(out)) == _cabi.E_INVALID
    assert b"K, N, swarmsize" in L.nmrfit_last_error()
    assert L.nmrfit_batch_destroy(None) == _cabi.OK
    assert L.nmrfit_batch_run(None, 1, 1) == _cabi.E_INVALID
    assert L.nmrfit_batch_status(None, None, None, None) == _cabi.E_INVALID
    assert L.nmrfit_batch_step(None) == _cabi.E_INVALID
    if _cabi.device_count() == 0:
        from nmrfit_amd import synth
        from nmrfit_amd.batch import FitBatch
        sp = synth.make_spectrum(1024, 2, seed=1)
        with pytest.raises(_cabi.NmrfitError) as ei:
            FitBatch([(sp["w"], sp["u"], sp["v"], sp["weights"])] * 2, [sp["lower"]] * 2, [sp["upper"]] * 2, swarmsize=8, seeds=[1, 2])
        assert ei.value.code == _cabi.E_NO_DEVICE


_CTX_PREFIXES = ("nmrfit_ctx_", "nmrfit_objective_", "nmrfit_residual_", "nmrfit_jacobian", "nmrfit_contributions",
                 "nmrfit_generate_result", "nmrfit_dev_", "nmrfit_memcpy_", "nmrfit_timer_", "nmrfit_prof_", "nmrfit_last_launch")


def test_every_entry_point_on_a_context_refuses_a_null_context():
    """Every call that takes a context (but create and destroy, above) returns NMRFIT_E_INVALID for a null one, with its
    other arguments valid-looking, before it touches a device: no GPU is needed, and none is opened where there is one."""
    L = _cabi.lib()
    tables = (_cabi.SIGNATURES, _cabi.DIAG_SIGNATURES, _cabi.LSQ_SIGNATURES, _cabi.LSQ_IM_SIGNATURES)
    names = sorted(n for t in tables for n in t if n.startswith(_CTX_PREFIXES) and n not in ("nmrfit_ctx_create", "nmrfit_ctx_destroy"))
    assert len(names) == 26, names
    P, B, N = 1, 8, 16
    D = 4 + 3 * P
    X, c, buf = np.full((B, D), 0.5), np.ones(D), np.zeros(2 * B * N)
    i64, i32, dbl, vp = ctypes.c_int64(), ctypes.c_int32(), ctypes.c_double(), ctypes.c_void_p()
    p, ref = _cabi.ptr, ctypes.byref
    calls = {
        "nmrfit_ctx_set_weights": (p(buf),), "nmrfit_ctx_synchronize": (), "nmrfit_ctx_set_variant": (0,),
        "nmrfit_ctx_set_fit_im": (0,), "nmrfit_ctx_set_stream": (None,), "nmrfit_ctx_n": (ref(i64),),
        "nmrfit_objective_batch": (B, P, p(X), 0, p(buf)), "nmrfit_residual_batch": (B, P, p(X), p(buf), None),
        "nmrfit_objective_batch_dev": (B, P, p(X), p(buf)), "nmrfit_residual_batch_dev": (B, P, p(X), p(buf), None),
        "nmrfit_residual_batch_im": (B, P, p(X), 1, p(buf), None),
        "nmrfit_contributions": (P, p(X), N, None, p(buf), p(buf)),
        "nmrfit_generate_result": (P, p(X), N, None, p(buf), p(buf), p(buf), p(buf)),
        "nmrfit_jacobian": (P, p(X), p(c), 1.0, None, None, None, None, p(buf)),
        "nmrfit_jacobian_im": (P, p(X), p(c), 1.0, 1, None, None, None, None, p(buf)),
        "nmrfit_dev_alloc": (64, ref(vp)), "nmrfit_dev_free": (p(buf),),
        "nmrfit_memcpy_h2d": (p(buf), p(X), 64), "nmrfit_memcpy_d2h": (p(buf), p(X), 64),
        "nmrfit_timer_begin": (), "nmrfit_timer_end": (ref(dbl),),
        "nmrfit_prof_enable": (4,), "nmrfit_prof_mark": (), "nmrfit_prof_read": (p(buf), 4, ref(i64), p(X), 4, ref(i64), ref(dbl)),
        "nmrfit_last_launch": (ref(i64), ref(i32), ref(i64)), "nmrfit_last_launch_workgroup": (ref(i32),),
    }
    assert sorted(calls) == names
    for name in names:
        assert getattr(L, name)(None, *calls[name]) == _cabi.E_INVALID, name
        assert L.nmrfit_last_error(), name
    assert not vp.value and not buf.any()


def test_every_device_entry_point_reports_a_bad_device_index_alike():
    """The eight entry points that take a device index share one device check: with arguments that are otherwise valid and
    an index no machine has, each returns NMRFIT_E_NO_DEVICE with the same message -- that no device is visible (or, on
    a box without a driver, what nmrfit_device_count says there) where there is no GPU, that the index is out of range
    where there is one."""
    L = _cabi.lib()
    dev, S, n, M, P, swarm = 1 << 20, 2, 16, 1, 1, 8
    D = 4 + 3 * P
    w = np.tile(np.linspace(0.0, 1.0, n), S)
    u, v, wt = np.cos(7.0 * w), np.sin(7.0 * w), np.ones(S * n)
    N = np.full(S, n, dtype=np.int64)
    peaks = np.full(S, P, dtype=np.int32)
    lower, upper = np.zeros(S * D), np.ones(S * D)
    params = (_cabi.PsoParams * S)(*[_cabi.PsoParams(0.5, 0.5, 0.5, 1e-8, 1e-8, k + 1) for k in range(S)])
    cand, x0 = np.zeros(2 * S * M), np.zeros(2 * S)
    score, x, f = np.zeros(S * M), np.zeros(2 * S), np.zeros(S)
    status, nfev, nit = (np.zeros(S, dtype=np.int32) for _ in range(3))
    n_mean, order = np.full(S, 4, dtype=np.int64), np.ones(S, dtype=np.int64)
    edges, thresh, baseline = np.zeros(10 * S), np.zeros(S), np.zeros(S)
    count = np.zeros(S, dtype=np.int64)
    nslots = S * ((100 * n - 1) // 2 + 1)
    pidx, pval = np.zeros(3 * nslots, dtype=np.int64), np.zeros(5 * nslots)
    U, Sm = np.zeros(100 * S * n), np.zeros(100 * S * n)
    out = ctypes.c_void_p()
    p = _cabi.ptr
    calls = {
        "nmrfit_ctx_create": lambda: L.nmrfit_ctx_create(dev, n, p(w), p(u), p(v), p(wt), ctypes.byref(out)),
        "nmrfit_batch_create": lambda: L.nmrfit_batch_create(dev, S, n, p(w), p(u), p(v), p(wt), p(peaks), p(lower), p(upper),
                                                             swarm, params, 0, 0, ctypes.byref(out)),
        "nmrfit_phase_scores": lambda: L.nmrfit_phase_scores(dev, _cabi.PHASE_ACME, S, p(N), p(u), p(v), M, p(cand), p(score),
                                                             p(status)),
        "nmrfit_phase_brute_levels": lambda: L.nmrfit_phase_brute_levels(dev, S, p(N), p(n_mean), p(u), p(v), M, p(cand),
                                                                         p(score)),
        "nmrfit_phase_estimate": lambda: L.nmrfit_phase_estimate(dev, _cabi.PHASE_ACME, S, p(N), p(u), p(v), p(x0), p(x), p(f),
                                                                 p(nfev), p(nit), p(status)),
        "nmrfit_diag_phase_nm_rosenbrock": lambda: L.nmrfit_diag_phase_nm_rosenbrock(dev, S, p(x0), p(x), p(f), p(nfev), p(nit)),
        "nmrfit_peaks_pick": lambda: L.nmrfit_peaks_pick(dev, S, p(N), p(w), p(u), p(edges), p(order), p(thresh), p(baseline),
                                                         p(count), p(pidx), p(pval)),
        "nmrfit_diag_peaks_smooth": lambda: L.nmrfit_diag_peaks_smooth(dev, S, p(N), p(w), p(u), p(edges), p(U), p(Sm)),
    }
    visible = ctypes.c_int(0)
    if L.nmrfit_device_count(ctypes.byref(visible)) != _cabi.OK:   # (no driver at all: the runtime's own refusal is passed on)
        expected = L.nmrfit_last_error()
        assert expected.startswith(b"hipGetDeviceCount failed: ")
    elif visible.value == 0:
        expected = b"no HIP device visible: libnmrfit_amd has no CPU fallback"
    else:
        expected = b"device index out of range"
    for name, call in calls.items():
        assert call() == _cabi.E_NO_DEVICE, name
        assert L.nmrfit_last_error() == expected, (name, L.nmrfit_last_error())
    assert not out.value


def test_variant_names():
    import pytest
    assert _cabi.variant_id("farfield") == _cabi.VARIANT_FARFIELD == 6
    assert _cabi.variant_id("Default") == 0 and _cabi.variant_id(2) == _cabi.VARIANT_NOSKIP
    for name in ("fastest", "quad", "single", "staged"):   # (the last three: retired A/B forms)
        with pytest.raises(ValueError):
            _cabi.variant_id(name)
    with pytest.raises(ValueError):
        _cabi.variant_id(9)


def test_build_stamp_names_the_sources_and_the_library(tmp_path, monkeypatch):
    """build() leaves the digests of the sources and of the libraries next to them; smoke() checks the
    library it loads against them on the GPU box (and rebuilds: the build is deterministic).  Here: the digest follows
    the sources, and the stamp of the library on disk matches it."""
    d0 = _cabi.source_digest()
    assert len(d0) == 64 and d0 == _cabi.source_digest()
    stamp = _cabi.read_stamp()
    if stamp is not None and stamp["source_sha256"] == d0:      # (a library built by __graft_entry__.build() from these sources)
        rec = stamp["libraries"]["libnmrfit_amd.so"]
        assert rec["sha256"] == _cabi.file_sha256(_cabi.LIB_PATH) and rec["bytes"] == os.path.getsize(_cabi.LIB_PATH)
    # the build script pins what would make two builds of the same sources differ
    script = open(_cabi.BUILD_SCRIPT).read()
    assert "-cuid=" in script and "-ffile-prefix-map=" in script

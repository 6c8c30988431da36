"""
No result may depend on what a fresh device allocation holds.

Every device allocation of the library goes through device_alloc (csrc/host_call.hip), which fills a new block with
the byte NMRFIT_POISON_ALLOC names before anybody sees it.  For each AREA of allocations -- ctx, swarm, batch, prep --
the case driver tests/poison_support.py runs in three fresh processes, one after the other:

    knob unset                 what the runtime hands out (in a young process: mostly zeros)
    NMRFIT_POISON_ALLOC=255    every fresh double is a NaN: garbage x 0, an output nobody wrote
    NMRFIT_POISON_ALLOC=63     every fresh double is 4.8e-4, every fresh index 0x3f3f3f3f...: the plausible finite value a
                               reduction that skips a slot by comparison would accept where it skips a NaN

Inside each process every result is asserted against the oracle of the existing test of that call, at that test's
tolerance; here the three files are held byte-identical, array by array, and the list of cases that ran is held equal in
the three and equal to the module's: no case may be skipped anywhere.  The test stops at the first child that does not
exit with 0 and starts no further one.  DESIGN.md 3.6 is the audit the runs confirm: for every piece of every allocation,
who writes it before whom may read it.

A child's time limit is ten times its wall time measured on the MI355X (profiles/r16/poison.txt), at least 60 s.
"""
import os
import subprocess
import sys
import time

import numpy as np
import pytest

from tests import poison_support

pytestmark = pytest.mark.gpu

ROOT = poison_support.ROOT
PATTERNS = (("unset", None), ("255", "255"), ("63", "63"))
# seconds per child: max(60, 10 x the slowest of the three children of the area, profiles/r16/poison.txt)
LIMIT = {"ctx": 60, "swarm": 60, "batch": 60, "prep": 60}


@pytest.fixture(scope="module")
def plan_query(tmp_path_factory):
    """tests/launch_plan/plan_query.hip, compiled once for the children of every area."""
    return poison_support.build_plan_query(str(tmp_path_factory.mktemp("plan_query") / "plan_query"))


@pytest.mark.parametrize("area", poison_support.AREAS)
def test_results_do_not_depend_on_fresh_device_memory(area, tmp_path, plan_query):
    files = {}
    for tag, poison in PATTERNS:
        out = str(tmp_path / ("%s_%s.npz" % (area, tag)))
        child_env = dict(os.environ, NMRFIT_POISON_PLAN_QUERY=plan_query)
        child_env.pop("NMRFIT_POISON_ALLOC", None)
        if poison is not None:
            child_env["NMRFIT_POISON_ALLOC"] = poison
        t0 = time.perf_counter()
        try:
            run = subprocess.run([sys.executable, "-m", "tests.poison_support", area, out], cwd=ROOT, env=child_env,
                                 capture_output=True, text=True, timeout=LIMIT[area])
        except subprocess.TimeoutExpired as e:       # (no further child)
            pytest.fail("%s, pattern %s: no exit within %d s\n%s" % (area, tag, LIMIT[area], (e.stderr or b"")[-3000:]))
        wall = time.perf_counter() - t0
        print("poison: area %-5s pattern %-5s child wall time %.2f s, exit %d" % (area, tag, wall, run.returncode))
        # (a signal shows as a negative code: the same stop, and no further child)
        assert run.returncode == 0, "%s, pattern %s: exit %d\n%s\n%s" % (area, tag, run.returncode, run.stdout[-1500:], run.stderr[-3000:])
        with np.load(out, allow_pickle=False) as z:
            files[tag] = {k: z[k] for k in z.files}
    want_cases = poison_support.case_names(area)
    base = files["unset"]
    for tag, poison in PATTERNS:
        got = files[tag]
        assert list(got["__cases__"]) == want_cases, (tag, list(got["__cases__"]))
        assert str(got["__poison__"]) == (poison or ""), (tag, got["__poison__"])      # (the child did see the knob)
        assert set(got) == set(base), (tag, sorted(set(got) ^ set(base))[:10])
    arrays = sorted(k for k in base if not k.startswith("__"))
    assert len(arrays) >= len(want_cases)
    differ = []
    for k in arrays:
        for tag in ("255", "63"):
            a, b = base[k], files[tag][k]
            if a.dtype != b.dtype or a.shape != b.shape or a.tobytes() != b.tobytes():
                differ.append((k, tag))
    assert not differ, "%d arrays differ from the unpoisoned run's: %s" % (len(differ), differ[:12])
    # nothing the library wrote into is still the NaN the driver put there: no copy came up short
    # (rows of the residual statistics may hold the NaN of an empty region's ratio: not raw outputs, not looked at here)
    for k in arrays:
        a = base[k]
        if a.dtype.kind == "f" and not k.split(":")[1].startswith(("stats.", "rows", "levels")):
            assert not np.isnan(a).any(), k

"""
CPU tier: the launch plan of the objective kernel (csrc/objective_plan.h) decides what launch_objective decided before
the plan had a header of its own.  tests/launch_plan/plan_sweep.hip walks the plan over 4.4 million launches (sweep.h:
2 chips x 2 wave targets x 5 variants x 3 fit_im x 2 x 3 A/B knobs x 14 ways of calling x 10 grids x 11 swarms x 8 peak
counts), folds what launch_objective makes of every plan into one FNV-1a hash and counts the cases per outcome class,
for the product and the A/B library and for both segment rules.  The hashes below, and the class counts in
tests/golden/launch_plan_parent.txt, were recorded from launch_objective itself at the commit before the plan moved
(profiles/r12/launch_objective_record.hip: the function with its kernel units, workspace and launches replaced by
recorders).  The program also checks the invariants of every planned launch (LDS within the CU's 160 KiB, segments
that tile the grid in whole blocks, when a workgroup may be wide or a pair, where f goes, what of a swarm generation
rides along and how many copies of a fused row a workgroup keeps for it) and fails on the first violation.  No HIP call: hipcc compiles it, nothing needs a GPU.
"""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"

# (build, segment rule) -> hash of launch_objective's decisions over the grid, at the parent of the plan's commit
PARENT_HASH = {
    ("product", 4): "cf70845ee74f17f8",
    ("product", 3): "49441320ef781d74",
    ("ab", 4): "81d9876ab13d4450",
    ("ab", 3): "23e9530d8713fc98",
}
CASES = 4435200


def sections(text):
    """{(build, rule): (cases, hash, [class lines])} of a record in sweep.h's print format."""
    out, cur = {}, None
    for line in text.splitlines():
        m = re.match(r"build=(\w+) seg_rule=(\d) cases=(\d+) hash=([0-9a-f]{16}) classes=(\d+)$", line)
        if m:
            cur = (m.group(1), int(m.group(2)))
            out[cur] = (int(m.group(3)), m.group(4), [])
        elif line.startswith("  code=") and cur is not None:
            out[cur][2].append(line.strip())
    return out


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_plan_decides_what_launch_objective_decided_and_keeps_its_invariants(tmp_path):
    exe = str(tmp_path / "plan_sweep")
    cc = subprocess.run([HIPCC, "--offload-arch=gfx950", "--cuda-host-only", "-O2", "-std=c++17",
                         "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "nmrfit_amd", "csrc"),
                         os.path.join(ROOT, "tests", "launch_plan", "plan_sweep.hip"), "-o", exe],
                        capture_output=True, text=True, timeout=300)
    assert cc.returncode == 0, cc.stderr[-3000:]
    runs = [subprocess.Popen([exe, rule], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for rule in ("4", "3")]
    got = {}
    for p in runs:
        out = p.communicate(timeout=300)[0]
        assert p.returncode == 0 and re.search(r"planned launches checked=\d{7} violations=0$", out, re.M), out[-3000:]
        got.update(sections(out))
    with open(os.path.join(ROOT, "tests", "golden", "launch_plan_parent.txt")) as f:
        want = sections(f.read())
    assert set(got) == set(want) == set(PARENT_HASH)
    for key, h in PARENT_HASH.items():
        assert want[key][:2] == (CASES, h), key                  # the golden file is the record the constants are from
        assert got[key][2] == want[key][2], (key, "\n".join(got[key][2]))   # (first: names the class that moved)
        assert got[key][:2] == (CASES, h), (key, got[key][:2])
        assert all(int(l.split()[-1]) > 0 for l in want[key][2]) and len(want[key][2]) >= 48, key

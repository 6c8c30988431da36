"""
CPU tier: the pair form of the DEFAULT objective kernel (csrc/objective_pair.h) stays inside the budget it pays in --
at most 128 VGPRs, no scratch, four waves per SIMD (three would leave its 2048 workgroups at C3 in 2.67 rounds of the
chip) -- by the compiler's own resource remarks (tools/kernel_resources.py --check; hipcc cross-compiles without a GPU).
"""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="hipcc not available")
def test_pair_form_fits_128_registers_without_scratch_at_four_waves():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"), "--check", "--unit", "objective_pair.hip"],
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-2000:]
    rows = {}
    for line in out.stdout.splitlines():
        m = re.match(r"(objective_kernel_pair<[^>]+>)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)", line)
        if m:
            rows[m.group(1)] = dict(vgpr=int(m.group(2)), scratch=int(m.group(4)), waves=int(m.group(5)), lds=int(m.group(6)))
    assert list(rows) == ["objective_kernel_pair<DEFAULT,objective,fit_im=0>"], out.stdout[-2000:]
    r = rows["objective_kernel_pair<DEFAULT,objective,fit_im=0>"]
    assert r["vgpr"] <= 128 and r["scratch"] == 0 and r["waves"] >= 4, r
    assert r["lds"] == 2 * (2 * 16 + 8) * 8, r      # static LDS: one block of sums and parked values per particle

"""
CPU tier of the poisoned-allocation check (tests/test_gpu_poison.py): what can be held without a GPU.

  * every device allocation of the library goes through device_alloc (csrc/host_call.hip): no other file under
    nmrfit_amd/csrc calls hipMalloc or one of its relatives, and that file calls it once, where the poison fill follows;
  * NMRFIT_POISON_ALLOC is parsed as INTEGRATION.md says (csrc/poison_knob.h, asked through tests/poison/knob_parse.hip
    compiled for the host): a decimal byte 0..255 fills, unset or anything else leaves the knob off;
  * the audit table of DESIGN.md 3.6 names, for every piece of every device allocation, the case of
    tests/poison_support.py that reaches it -- every named case exists, every case of the driver is named, every
    allocation site has its rows, and the only rows without a case are the ones a single-GPU process without RCCL cannot
    reach (the communicator's two buffers), marked as such.
"""
import os
import re
import subprocess

from tests import poison_support

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "nmrfit_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
HOME = "host_call.hip"
# (hipHostMalloc is the pinned staging buffer's: host memory, written in full before it is read, not poisoned)
ALLOCATORS = r"\b(hipMalloc|hipMallocAsync|hipMallocManaged|hipMallocPitch|hipMalloc3D|hipExtMallocWithFlags|hipMallocFromPoolAsync)\s*\("
# the allocation sites (ISSUE: 11 of them), as the audit table names them
SITES = ("ensure", "ctx d_block", "nmrfit_dev_alloc", "d_clk", "pso d_block", "batch d_block", "d_result", "d_quality",
         "d_gather", "d_scratch", "Scratch::alloc")
UNREACHED = ("needs RCCL",)


def _sources():
    return sorted(f for f in os.listdir(CSRC) if f.endswith((".hip", ".h")))


def test_no_file_allocates_device_memory_but_the_one_function():
    calls = {}
    for name in _sources():
        with open(os.path.join(CSRC, name)) as fh:
            text = fh.read()
        n = len(re.findall(ALLOCATORS, text))
        if n:
            calls[name] = n
    assert calls == {HOME: 1}, calls
    with open(os.path.join(CSRC, HOME)) as fh:
        text = fh.read()
    body = re.search(r"hipError_t device_alloc\(void \*\*p, size_t bytes\)\n\{(.*?)\n\}\n", text, re.S)
    assert body, "device_alloc not found in " + HOME
    body = body.group(1)
    assert re.search(ALLOCATORS, body), "the one call is not inside device_alloc"
    # the fill is the runtime's memset (no kernel of the library's own) and is waited for before the function returns
    assert 'parse_poison_byte(getenv("NMRFIT_POISON_ALLOC"))' in body and "static const int poison" in body
    assert re.search(r"hipMemset\(\*p, poison, bytes\)", body) and "hipStreamSynchronize(nullptr)" in body
    assert "hipLaunchKernelGGL" not in body and "<<<" not in body
    users = [name for name in _sources() if name != HOME and re.search(r"\bdevice_alloc\(", open(os.path.join(CSRC, name)).read())]
    assert users == ["batch_create.hip", "batch_data.hip", "comm.hip", "ctx.hip", "host_call.h", "pso.hip"], users


def test_the_knob_is_parsed_as_documented(tmp_path):
    exe = str(tmp_path / "knob_parse")
    cc = subprocess.run([HIPCC, "--offload-arch=gfx950", "--cuda-host-only", "-O1", "-std=c++17", "-I" + CSRC,
                         os.path.join(ROOT, "tests", "poison", "knob_parse.hip"), "-o", exe],
                        capture_output=True, text=True, timeout=300)
    assert cc.returncode == 0, cc.stderr[-3000:]
    cases = [("UNSET", -1), ("", -1), ("0", 0), ("63", 63), ("255", 255), ("007", 7), ("256", -1), ("1000", -1), ("-1", -1),
             ("+5", -1), ("0x3f", -1), ("63 ", -1), (" 63", -1), ("6.3", -1), ("on", -1), ("NaN", -1), ("99999999999999999999", -1)]
    run = subprocess.run([exe] + [text for text, _ in cases], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0, run.stderr
    got = [int(line) for line in run.stdout.split()]
    assert got == [want for _, want in cases], list(zip(cases, got))
    with open(os.path.join(ROOT, "INTEGRATION.md")) as fh:
        doc = fh.read()
    assert "NMRFIT_POISON_ALLOC" in doc and "0..255" in doc


def _audit_rows():
    """The rows of the audit table: [(allocation, piece, case column)]."""
    with open(os.path.join(ROOT, "DESIGN.md")) as fh:
        text = fh.read()
    m = re.search(r"^### 3\.6 .*?$(.*?)(?=^##+ )", text, re.S | re.M)
    assert m, "DESIGN.md has no section 3.6"
    rows = []
    for line in m.group(1).splitlines():
        cells = [c.strip() for c in line.strip().strip("|").split("|")]
        if not line.startswith("|") or len(cells) != 7 or cells[0] in ("allocation", "") or set(cells[0]) <= set("-: "):
            continue
        rows.append((cells[0], cells[1], cells[6]))
    return rows


def test_the_audit_table_names_a_case_for_every_piece_a_single_gpu_process_reaches():
    rows = _audit_rows()
    assert len(rows) >= 40, len(rows)
    known = set(poison_support.case_ids())
    named = set()
    for allocation, piece, cases in rows:
        if cases in UNREACHED:
            continue
        ids = [c.strip(" `") for c in cases.split(",")]
        assert ids and all(ids), (allocation, piece, cases)
        for c in ids:
            assert c in known, "%s / %s names the case %r, which tests/poison_support.py does not have" % (allocation, piece, c)
        named.update(ids)
    assert named == known, sorted(known - named)
    for site in SITES:
        assert any(site in allocation for allocation, _, _ in rows), "no row for the allocation site %r" % site
    # what stays without a case: the communicator's two buffers (RCCL)
    unreached = [(a, p) for a, p, c in rows if c in UNREACHED]
    assert all("d_gather" in a or "d_scratch" in a for a, _ in unreached), unreached
    assert len(poison_support.case_ids()) == len(set(poison_support.case_ids()))
    for area in poison_support.AREAS:
        assert poison_support.case_names(area), area

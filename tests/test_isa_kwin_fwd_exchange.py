"""Build-time guard for the forward exchange of the fused N = 4096 kernel (fft_r16.hpp xchg_b2f_read, DESIGN.md section
5.1): role B's sixteen reads behind the forward transform's barrier are sixteen ds_read_b64.  Written as plain C++ loads
the compiler pairs them into eight ds_read2_b64, which cost twice the LDS-array cycles per byte and bank by 32; kept apart
through a volatile pointer they push the kernel into scratch memory.  This test disassembles the built library and fails if
a code or compiler change brings either back: no ds_read2_b64 anywhere in k_win / k_win_lb, at most 227 VGPRs, no spills,
no private segment."""
import os
import re
import shutil
import subprocess

import pytest

from conftest import ROOT

OBJDUMP = "/opt/rocm/lib/llvm/bin/llvm-objdump"
READELF = "/opt/rocm/lib/llvm/bin/llvm-readelf"
KERNELS = ("_ZN3rmx5k_winILb0EE", "_ZN3rmx5k_winILb1EE", "_ZN3rmx8k_win_lbILb0EE", "_ZN3rmx8k_win_lbILb1EE")


@pytest.fixture(scope="module")
def code_object(tmp_path_factory):
    if not (os.path.exists(OBJDUMP) and os.path.exists(READELF)):
        pytest.skip("no llvm-objdump / llvm-readelf")
    import __graft_entry__ as g
    g.build()
    work = str(tmp_path_factory.mktemp("kwin_fwd_isa"))
    shutil.copy(os.path.join(ROOT, "radio-mapper_amd", "csrc", "librmx_hip.so"), os.path.join(work, "lib.so"))
    subprocess.run([OBJDUMP, "--offloading", "lib.so"], cwd=work, check=True, capture_output=True)
    objs = [f for f in os.listdir(work) if "gfx950" in f]
    assert objs, "no gfx950 code object in the library"
    return os.path.join(work, objs[0])


def test_forward_exchange_reads_are_not_paired(code_object):
    dis = subprocess.run([OBJDUMP, "-d", "--no-show-raw-insn", code_object], check=True, capture_output=True, text=True).stdout
    bodies, cur = {}, None
    for ln in dis.splitlines():
        m = re.match(r"^[0-9a-f]+ <(\S+)>:", ln)
        if m:
            cur = next((k for k in KERNELS if m.group(1).startswith(k)), None)
            if cur:
                bodies[cur] = []
            continue
        if cur:
            t = ln.split("//")[0].strip()
            if t:
                bodies[cur].append(t)
    assert sorted(bodies) == sorted(KERNELS), list(bodies)
    for name, ins in bodies.items():
        ops = [t.split()[0] for t in ins]
        assert "ds_read2_b64" not in ops and "ds_read2st64_b64" not in ops, (name, ops.count("ds_read2_b64"))
        # the parser still sees this kernel's LDS reads: three copies of the forward transform, sixteen reads each, besides
        # the role-A reads of the pair halves
        assert ops.count("ds_read_b64") >= 3 * 16 + 16, (name, ops.count("ds_read_b64"))
        print(name, "ds_read_b64:", ops.count("ds_read_b64"), "instructions:", len(ins))


def test_fused_kernels_stay_inside_their_register_budget(code_object):
    notes = subprocess.run([READELF, "--notes", code_object], check=True, capture_output=True, text=True).stdout
    seen = {}
    for b in re.split(r"\n\s*- \.agpr_count:", notes)[1:]:
        name = re.search(r"\.name:\s+(\S+)", b)
        key = next((k for k in KERNELS if name and name.group(1).startswith(k)), None)
        if key:
            seen[key] = {k: int(re.search(r"\.%s:\s+(\d+)" % k, b).group(1)) for k in
                         ("private_segment_fixed_size", "vgpr_count", "vgpr_spill_count")}
    assert sorted(seen) == sorted(KERNELS), list(seen)
    for n, f in seen.items():
        assert f["vgpr_count"] <= 227, (n, f)
        assert f["vgpr_spill_count"] == 0, (n, f)
        assert f["private_segment_fixed_size"] == 0, (n, f)
    print(seen)

"""Compare the gfx950 kernels of two builds of librmx_hip.so: instruction bodies and resources (VGPR / SGPR / AGPR counts,
spills, LDS, scratch) of every kernel the OLD library has, matched by demangled name with the template's trailing empty
argument pack removed (k_pair_res<>  ==  k_pair_res), and the resources of the kernels only the NEW one has.

    python tools/isa_diff.py OLD.so NEW.so

Branch targets are compared as offsets (the comments objdump adds, which carry absolute addresses, are dropped); a
PC-relative literal of a global address (s_getpc_b64 + s_add_u32 / s_addc_u32) is compared as "a relocation" only, since
it moves with the code object's layout.  Exit status 1 if any old kernel differs."""
import os
import re
import subprocess
import sys
import tempfile

LLVM = "/opt/rocm/lib/llvm/bin"
FIELDS = ("vgpr_count", "sgpr_count", "agpr_count", "vgpr_spill_count", "sgpr_spill_count", "group_segment_fixed_size",
          "private_segment_fixed_size", "kernarg_segment_size")


def _code_object(lib, work):
    import shutil
    shutil.copy(lib, os.path.join(work, "lib.so"))
    subprocess.run([os.path.join(LLVM, "llvm-objdump"), "--offloading", "lib.so"], cwd=work, check=True, capture_output=True)
    objs = [f for f in os.listdir(work) if "gfx950" in f]
    assert objs, "no gfx950 code object in %s" % lib
    return os.path.join(work, objs[0])


def _demangle(names):
    import shutil
    tool = os.path.join(LLVM, "llvm-cxxfilt")
    tool = tool if os.path.exists(tool) else shutil.which("llvm-cxxfilt") or shutil.which("c++filt")
    out = subprocess.run([tool], input="\n".join(names), capture_output=True, text=True,
                         check=True).stdout.splitlines()
    return dict(zip(names, out))


def _key(dem):
    """'void rmx::k_pair_res<>(...)' and 'rmx::k_pair_res(...)' -> 'rmx::k_pair_res'"""
    depth = 0
    for i, ch in enumerate(dem):
        if ch == "<":
            depth += 1
        elif ch == ">":
            depth -= 1
        elif ch == "(" and depth == 0:
            dem = dem[:i]
            break
    if dem.startswith("void "):
        dem = dem[5:]
    return dem.replace("<>", "").replace(", >", ">").strip()


def load(lib):
    with tempfile.TemporaryDirectory() as work:
        obj = _code_object(lib, work)
        dis = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", "--no-show-raw-insn", obj], check=True,
                             capture_output=True, text=True).stdout
        notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", obj], check=True, capture_output=True,
                               text=True).stdout
    bodies, cur = {}, None
    for ln in dis.splitlines():
        m = re.match(r"^[0-9a-f]+ <(.+)>:$", ln)
        if m:
            cur = m.group(1)
            bodies[cur] = []
            continue
        if cur is None:
            continue
        ins = ln.split("//")[0].strip()
        if ins:
            bodies[cur].append(ins)
    res = {}
    for b in re.split(r"\n\s*- \.agpr_count:", notes)[1:]:
        b = ".agpr_count:" + b
        name = re.search(r"\.name:\s+(\S+)", b)
        if not name:
            continue
        res[name.group(1)] = {f: int(re.search(r"\.%s:\s+(\d+)" % f, b).group(1)) if re.search(r"\.%s:\s+(\d+)" % f, b)
                              else None for f in FIELDS}
    kernels = [n for n in res]
    dem = _demangle(kernels)
    out = {}
    for n in kernels:
        body = list(bodies.get(n, []))
        while body and body[-1] in ("s_nop 0", "..."):   # the padding behind the last s_endpgm
            body.pop()
        # PC-relative literals of global addresses move with the layout
        norm, prev = [], ""
        for ins in body:
            if re.match(r"s_add(c)?_u32 s\d+, s\d+, 0x[0-9a-f]+$", ins) and prev.startswith(("s_getpc_b64", "s_add_u32")):
                ins = re.sub(r"0x[0-9a-f]+$", "<reloc>", ins)
            norm.append(ins)
            prev = ins
        out[_key(dem[n])] = {"sym": n, "res": res[n], "body": norm}
    return out


def main(old_lib, new_lib):
    old, new = load(old_lib), load(new_lib)
    bad = 0
    print("%-64s %6s %6s %6s %6s %8s %8s  %s" % ("kernel (old library)", "vgpr", "sgpr", "spill", "lds", "scratch", "insns",
                                                 "vs new"))
    for k in sorted(old):
        o = old[k]
        n = new.get(k)
        if n is None:
            verdict = "MISSING"
        elif o["body"] != n["body"]:
            verdict = "BODY DIFFERS"
        elif o["res"] != n["res"]:
            # kernarg_segment_size is compared too: the unbounded kernels take exactly their old arguments
            verdict = "RESOURCES DIFFER %s" % {f: (o["res"][f], n["res"][f]) for f in FIELDS if o["res"][f] != n["res"][f]}
        else:
            verdict = "identical" + ("" if o["sym"] == n["sym"] else " (symbol renamed)")
        bad += verdict.split()[0] != "identical"
        r = o["res"]
        print("%-64s %6s %6s %6s %6s %8s %8d  %s" % (k[:64], r["vgpr_count"], r["sgpr_count"], r["vgpr_spill_count"],
                                                     r["group_segment_fixed_size"], r["private_segment_fixed_size"],
                                                     len(o["body"]), verdict))
    print("\nkernels only in the new library:")
    print("%-64s %6s %6s %6s %6s %8s %8s" % ("kernel", "vgpr", "sgpr", "spill", "lds", "scratch", "insns"))
    for k in sorted(set(new) - set(old)):
        r = new[k]["res"]
        print("%-64s %6s %6s %6s %6s %8s %8d" % (k[:64], r["vgpr_count"], r["sgpr_count"], r["vgpr_spill_count"],
                                                 r["group_segment_fixed_size"], r["private_segment_fixed_size"],
                                                 len(new[k]["body"])))
    print("\n%d of %d old kernels differ" % (bad, len(old)))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2]))

#!/usr/bin/env python3
"""Do two builds hold the same instructions for the kernels named?

    tools/isa_identity.py OLD_BUILD_DIR NEW_BUILD_DIR [kernel ...]

Unbundles the gfx950 code object of snappy_kernels_c.o and snappy_kernels_d.o
of both build directories (the objcopy / clang-offload-bundler / llvm-objdump
steps of tests/test_abi.py::test_kernel_register_budget), takes each named
kernel's disassembly, strips addresses and encodings (branch targets stay, as
offsets from the kernel's own start; the pc-relative address of a called
function and the padding after the last instruction do not) and compares.
Prints one line per kernel and exits 1 if any differs.  Default kernels: the
five of the fixed layouts (K1r, K1r64, K2, K4 pass 1 and 2).
"""
import hashlib
import os
import re
import subprocess
import sys
import tempfile

LLVM = "/opt/rocm/lib/llvm/bin"
DEFAULT = ["k1r_match_units", "k1r_match_units64", "k2_emit_units", "k4_decompress_units", "k4_decompress_back"]


def disassemble(obj: str, tmp: str) -> str:
    fat, co = os.path.join(tmp, "fat.bin"), os.path.join(tmp, "k.co")
    subprocess.run(["objcopy", f"--dump-section=.hip_fatbin={fat}", obj, os.path.join(tmp, "copy.o")], check=True)
    subprocess.run([f"{LLVM}/clang-offload-bundler", "--unbundle", "--type=o", f"--input={fat}",
                    "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--output={co}"], check=True)
    return subprocess.run([f"{LLVM}/llvm-objdump", "-d", co], check=True, capture_output=True, text=True).stdout


def kernels(dis: str) -> dict:
    """demangled-ish kernel name -> its instructions, addresses stripped"""
    out, name, body = {}, None, []
    for ln in dis.splitlines():
        m = re.match(r"^[0-9a-f]+ <(\S+)>:$", ln)
        if m:
            if name:
                out[name] = body
            name, body = m.group(1), []
        elif name and ln.startswith("\t"):
            ins = ln.split("//")[0].rstrip()
            # a branch's comment names its target as <symbol+0xoff>: keep that offset
            t = re.search(r"<[^>+]+(\+0x[0-9a-f]+)?>\s*$", ln)
            if "branch" in ins:  # the encoded distance stays; the target is named from the kernel's start
                ins += " -> " + ((t.group(1) or "+0x0") if t else "?")
            elif body and "s_getpc_b64" in body[-1] and "s_add_u32" in ins:
                # the pc-relative address of a function called (k4_wait, k4_literal_hbm): it moves
                # with whatever else the object holds
                ins = ins.rsplit(",", 1)[0] + ", <pcrel>"
            body.append(ins)
    if name:
        out[name] = body
    for b in out.values():  # the padding up to the next function's alignment
        while b and b[-1].strip().startswith("s_nop"):
            b.pop()
    return out


def find(ks: dict, kernel: str):
    # _ZN10snappy_amd<len><name>E...: the exact name, not a longer one that contains it
    hits = [k for k in ks if re.search(rf"\d{re.escape(kernel)}E", k)]
    return ks[hits[0]] if len(hits) == 1 else None


def main(argv):
    if len(argv) < 3:
        print(__doc__)
        return 2
    old_dir, new_dir, names = argv[1], argv[2], argv[3:] or DEFAULT
    sides = []
    for d in (old_dir, new_dir):
        ks = {}
        for o in ("snappy_kernels_c.o", "snappy_kernels_d.o"):
            with tempfile.TemporaryDirectory() as tmp:
                ks.update(kernels(disassemble(os.path.join(d, o), tmp)))
        sides.append(ks)
    bad = 0
    for k in names:
        a, b = find(sides[0], k), find(sides[1], k)
        if a is None or b is None:
            print(f"{k}: missing ({'old' if a is None else 'new'})")
            bad += 1
            continue
        same = a == b
        bad += not same
        print(f"{k}: {len(a)} / {len(b)} instructions, sha256 {hashlib.sha256(chr(10).join(b).encode()).hexdigest()[:16]}, "
              f"{'identical' if same else 'DIFFERENT'}")
    print("all identical" if not bad else f"{bad} kernel(s) differ")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))

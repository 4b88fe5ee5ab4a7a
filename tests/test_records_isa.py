"""CPU: the record entry points in the built gfx950 code objects.

kr1_match_records / kr1_match_records64 instantiate k1r_body with the record's
source, token base and segment base taken from the plan's tables: values the
asm statements take as "s" operands.  Had one of them become a VGPR the kernels
would leave the 168-VGPR budget of 3 waves per SIMD or spill, and the unit's
registers v2..v129 would no longer be safe -- the checks the fixed-layout
kernels pass in tests/test_abi.py, run on the new symbols.  Skips, as those
tests do, without the in-tree build objects or the ROCm LLVM tools.
"""
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = "/opt/rocm/lib/llvm/bin"
sys.path.insert(0, os.path.join(ROOT, "tools"))


def code_object(tmp_path, obj):
    path = os.path.join(ROOT, "lightweight-snappy_amd", "build", obj)
    if not (os.path.exists(path) and os.path.exists(f"{LLVM}/llvm-objdump") and shutil.which("objcopy")):
        pytest.skip("needs the in-tree build object and the ROCm LLVM tools")
    fat, co = tmp_path / f"{obj}.fat", tmp_path / f"{obj}.co"
    # (an output file: with none, objcopy rewrites the build object in place)
    subprocess.run(["objcopy", f"--dump-section=.hip_fatbin={fat}", path, str(tmp_path / f"{obj}.copy")], check=True)
    subprocess.run([f"{LLVM}/clang-offload-bundler", "--unbundle", "--type=o", f"--input={fat}",
                    "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--output={co}"], check=True)
    return co


def whole_kernels(dis: str) -> str:
    """The disassembly with every kernel in one piece.  The K1r asm statements'
    labels (L3_top, L3_end, ...) are symbols of the object: llvm-objdump starts a
    new <label>: section at each and names branch targets from the nearest one
    (<L3_end+0x2348>).  The checkers read sections as kernels and targets as
    <kernel+0xOFF>, so on the raw text they see a kernel up to its first label
    only and resolve such a target against the wrong base.  Here the label
    headers are dropped and every branch's target is recomputed from its own
    offset field (address + 4 + 4 * simm16), relative to its kernel."""
    out, kname, kbase = [], None, 0
    for ln in dis.splitlines():
        m = re.match(r"^([0-9a-f]+) <(\w+)>:", ln)
        if m:
            if m.group(2).startswith("_Z"):
                kname, kbase = m.group(2), int(m.group(1), 16)
                out.append(ln)
            continue
        b = re.match(r"^\t(s_c?branch\w*) (\d+)\s+// ([0-9A-F]+): (\w+)", ln)
        if b and kname:
            n = int(b.group(2))
            n -= (n & 0x8000) << 1
            target = int(b.group(3), 16) + 4 + 4 * n
            ln = f"\t{b.group(1)} {b.group(2)}  // {b.group(3)}: {b.group(4)} <{kname}+0x{target - kbase:x}>"
        out.append(ln)
    return "\n".join(out) + "\n"


def kernel_notes(co):
    notes = subprocess.run([f"{LLVM}/llvm-readobj", "--notes", str(co)], check=True, capture_output=True,
                           text=True).stdout
    out = {}
    for blk in notes.split("- .agpr_count")[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        out[name] = {k: int(re.search(rf"\.{k}:\s+(\d+)", blk).group(1))
                     for k in ("vgpr_count", "vgpr_spill_count", "private_segment_fixed_size")}
    return out


def only(notes, kernel):
    hits = [v for k, v in notes.items() if re.search(rf"\d{kernel}E", k)]
    assert len(hits) == 1, (kernel, sorted(notes))
    return hits[0]


def test_record_match_kernels_keep_the_register_budget(tmp_path):
    import check_asm_waits
    import check_ring
    co = code_object(tmp_path, "snappy_kernels_c.o")
    notes = kernel_notes(co)
    for k in ("kr1_match_records", "kr1_match_records64"):
        n = only(notes, k)
        assert n["vgpr_count"] <= 168 and n["vgpr_spill_count"] == 0 and n["private_segment_fixed_size"] == 0, (k, n)
    dis = subprocess.run([f"{LLVM}/llvm-objdump", "-d", str(co)], check=True, capture_output=True, text=True).stdout
    dis = whole_kernels(dis)
    # check_ring picks its kernels by name: show it the record kernels under a name it picks
    only_records = dis.replace("k1r_match_units", "k1r_fixed_layout").replace("kr1_match_records", "k1r_match_units_records")
    picked = check_ring.kernels(only_records)
    assert len(picked) == 2 and all(len(ins) > 5000 for ins in picked.values())  # (whole kernels, asm loops included)
    assert check_ring.check(only_records) == []
    assert check_asm_waits.check_m0(dis, names=("kr1_match_records",)) == []
    assert "global_load_lds" in dis
    assert check_asm_waits.check(dis) == []  # (every kernel of the object, the LDS-DMA of kr1_match_records64 included)


def test_record_decode_kernel_keeps_the_register_budget(tmp_path):
    import check_asm_waits
    co = code_object(tmp_path, "snappy_kernels_d.o")
    n = only(kernel_notes(co), "kr4_decode_records")
    assert n["vgpr_count"] <= 64 and n["vgpr_spill_count"] == 0 and n["private_segment_fixed_size"] == 0, n
    dis = subprocess.run([f"{LLVM}/llvm-objdump", "-d", str(co)], check=True, capture_output=True, text=True).stdout
    dis = whole_kernels(dis)
    assert check_asm_waits.check(dis) == []
    # the element-start bitmap check picks k4_decompress* kernels: the record kernel under such a name
    renamed = dis.replace("kr4_decode_records", "k4_decompress_records")
    assert sum("k4_decompress_records" in k for k in check_asm_waits.kernels(renamed)) == 1
    assert check_asm_waits.check_k4_bitmap(renamed) == []


def test_sources_pass_the_asm_lints():
    import check_asm_waits
    csrc = os.path.join(ROOT, "lightweight-snappy_amd", "csrc")
    for f in ("snappy_records.hip", "snappy_kernels.hip", "snappy_k2_emit.inc"):
        assert check_asm_waits.lint_source(os.path.join(csrc, f)) == [], f
        assert check_asm_waits.lint_scc(os.path.join(csrc, f)) == [], f

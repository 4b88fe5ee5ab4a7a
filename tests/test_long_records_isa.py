"""CPU: the long-record entry points in the built gfx950 code objects.

kr1_match_lunits / kr1_match_lunits64 instantiate k1r_body with the unit's
source, token base and segment base computed from the plan's and the
expansion's tables (record start + 65,536 x block, scratch + sbase[unit]) and
with a preamble mode that differs from unit to unit: all of it values the asm
statements take as "s" operands.  Had one of them become a VGPR the kernels would
leave the 168-VGPR budget of 3 waves per SIMD or spill, and the unit's registers
v2..v129 would no longer be safe.  kr4_decode_lunits / kr4_back_lunits enter
k4_body with one record's shifted pointers and must keep K4's 64 VGPRs (8 waves
per SIMD).  The checks of tests/test_records_isa.py, run on the new symbols;
skips, as those do, without the in-tree build objects or the ROCm LLVM tools.
"""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from test_records_isa import LLVM, code_object, kernel_notes, only, whole_kernels  # noqa: E402


def test_long_match_kernels_keep_the_register_budget(tmp_path):
    import check_asm_waits
    import check_ring
    co = code_object(tmp_path, "snappy_kernels_c.o")
    notes = kernel_notes(co)
    for k in ("kr1_match_lunits", "kr1_match_lunits64"):
        n = only(notes, k)
        assert n["vgpr_count"] <= 168 and n["vgpr_spill_count"] == 0 and n["private_segment_fixed_size"] == 0, (k, n)
    # the emit entry point shares the short records' budget (6 waves per SIMD)
    assert only(notes, "kr2_emit_lunits")["vgpr_count"] <= 80
    dis = subprocess.run([f"{LLVM}/llvm-objdump", "-d", str(co)], check=True, capture_output=True, text=True).stdout
    dis = whole_kernels(dis)
    # check_ring picks its kernels by name: show it the long-record kernels under a name it picks
    only_long = dis.replace("k1r_match_units", "k1r_fixed_layout").replace("kr1_match_lunits", "k1r_match_units_long")
    picked = check_ring.kernels(only_long)
    assert len(picked) == 2 and all(len(ins) > 5000 for ins in picked.values())  # (whole kernels, asm loops included)
    assert check_ring.check(only_long) == []
    assert check_asm_waits.check_m0(dis, names=("kr1_match_lunits",)) == []
    assert check_asm_waits.check(dis) == []  # (every kernel of the object, the LDS-DMA of kr1_match_lunits64 included)


def test_long_decode_kernels_keep_the_register_budget(tmp_path):
    import check_asm_waits
    co = code_object(tmp_path, "snappy_kernels_d.o")
    notes = kernel_notes(co)
    for k in ("kr4_decode_lunits", "kr4_back_lunits"):
        assert only(notes, k)["vgpr_count"] <= 64, (k, only(notes, k))
    n = only(notes, "kr4_decode_lunits")  # pass 1, the path every block takes
    assert n["vgpr_spill_count"] == 0 and n["private_segment_fixed_size"] == 0, n
    dis = subprocess.run([f"{LLVM}/llvm-objdump", "-d", str(co)], check=True, capture_output=True, text=True).stdout
    dis = whole_kernels(dis)
    assert check_asm_waits.check(dis) == []
    # the element-start bitmap check picks k4_decompress* kernels: the long-record kernels under such names
    renamed = dis.replace("kr4_decode_lunits", "k4_decompress_lunits").replace("kr4_back_lunits", "k4_decompress_lback")
    assert sum("k4_decompress_l" in k for k in check_asm_waits.kernels(renamed)) == 2
    assert check_asm_waits.check_k4_bitmap(renamed) == []


def test_sources_pass_the_asm_lints():
    import check_asm_waits
    csrc = os.path.join(ROOT, "lightweight-snappy_amd", "csrc")
    for f in ("snappy_long_records.hip", "snappy_kernels.hip", "snappy_k2_emit.inc"):
        assert check_asm_waits.lint_source(os.path.join(csrc, f)) == [], f
        assert check_asm_waits.lint_scc(os.path.join(csrc, f)) == [], f

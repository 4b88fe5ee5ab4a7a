"""CPU: the framed range-decode entry point in the built gfx950 code object.

kr4_decode_frame_units enters k4_body's record instantiation with everything
taken per planned unit from tables in HBM: the chunk's position and header bytes,
its decoded length from the seek table, a staging slot or a place in the caller's
buffer as an absolute address, a status pointer shifted by the chunk's number.
It must keep K4's 64 VGPRs (8 waves per SIMD) without a spill or a private
segment.  The checks of tests/test_ranges_isa.py, run on the new symbol; skips,
as those do, without the in-tree build objects or the ROCm LLVM tools.
"""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from test_records_isa import LLVM, code_object, kernel_notes, only, whole_kernels  # noqa: E402


def test_frame_range_decode_kernel_keeps_the_register_budget(tmp_path):
    import check_asm_waits
    co = code_object(tmp_path, "snappy_kernels_d.o")
    n = only(kernel_notes(co), "kr4_decode_frame_units")
    assert n["vgpr_count"] <= 64 and n["vgpr_spill_count"] == 0 and n["private_segment_fixed_size"] == 0, n
    dis = subprocess.run([f"{LLVM}/llvm-objdump", "-d", str(co)], check=True, capture_output=True, text=True).stdout
    dis = whole_kernels(dis)
    assert check_asm_waits.check(dis) == []
    # the element-start bitmap check picks k4_decompress* kernels: the frame kernel under such a name
    renamed = dis.replace("kr4_decode_frame_units", "k4_decompress_frame_units")
    assert sum("k4_decompress_frame_units" in k for k in check_asm_waits.kernels(renamed)) == 1
    assert check_asm_waits.check_k4_bitmap(renamed) == []


def test_sources_pass_the_asm_lints():
    import check_asm_waits
    csrc = os.path.join(ROOT, "lightweight-snappy_amd", "csrc")
    for f in ("snappy_frame_ranges.hip", "snappy_frame.hip", "snappy_ranges.hip", "snappy_kernels.hip"):
        assert check_asm_waits.lint_source(os.path.join(csrc, f)) == [], f
        assert check_asm_waits.lint_scc(os.path.join(csrc, f)) == [], f

"""CPU: the plan rule that the device call and the host forms of range decode
share (csrc/snappy_ranges.h), compiled as plain C into a stand-alone program
with AddressSanitizer and UBSan (tests/ranges_plan_check.c) and run on stream
lengths, unit sizes and ranges at every edge of the rule, each array in an
exactly sized heap block.  Every status and every unit entry must be the Python
model's (tests/ranges_model.py).  Nothing is loaded into this process."""
import os
import shutil
import struct
import subprocess

import high_positions as hp
import ranges_model as rm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "ranges_plan_check.c")
B = rm.BLOCK
U64 = rm.U64


def ranges_for(n, unit):
    """Ranges at the rule's edges for a stream of n bytes in units of `unit`"""
    r = [(0, 0), (0, 1), (0, n), (n, 0), (n + 1, 0), (1, n), (0, n + 1), (n - 1 if n else 0, 1), (n - 1 if n else 0, 2),
         (U64, 1), (U64, U64), (1, U64), (U64 - 5, 10), (5, U64 - 4), (1 << 63, 1 << 63)]
    for b in (unit, 2 * unit, 4 * unit):
        r += [(b - 1, 2), (b, unit), (b - 1, 1), (b, 1), (b - unit, unit), (b - unit + 1, unit - 1 if unit > 1 else 0),
              (b - unit, unit + 1), (b - 1, unit + 2)]
    if n:
        last = (n - 1) // unit * unit
        r += [(last, n - last), (last, 1), (last + (n - last) // 2, (n - last) - (n - last) // 2), (last - 1 if last else 0, 2)]
    # consecutive output offsets of every residue mod 16, whatever the range
    out, oo = [], 3
    for k, (s, ln) in enumerate(r):
        out.append((s, ln, oo))
        oo += (ln if s <= n and ln <= n - s else 0) + (k % 16) + 1
    return out, oo


def build_cases():
    cases = []
    for n in (0, 1, 65535, 65536, 65537, 4 * 65536 + 1234):
        for unit in (B, 1, 17):
            if unit != B and n > 70000:
                r = [(0, 40, 0), (16, 18, 40), (n - 20, 20, 58), (n - 17, 17, 78), (33, 1, 95), (34, 0, 96),
                     (n, 1, 96), (0, 100, U64), (0, 100, 1 << 40)]
                cases.append((n, 96 if unit == 17 else 1 << 41, unit, r))
                continue
            r, need = ranges_for(n, unit)
            cases.append((n, need + 16, unit, r))
            # output ranges that leave out_bytes: a buffer that ends inside the ranges, offsets that overflow
            cases.append((n, need // 2, unit, r + [(0, min(n, 1), U64), (0, min(n, 2), U64 - 1), (0, 0, need // 2),
                                                    (0, 0, need // 2 + 1), (0, min(n, 1), need // 2)]))
    cases.append((100, 100, 0, [(0, 1, 0)]))        # no unit size
    cases.append((100, 100, B + 1, [(0, 1, 0)]))    # a unit above a block
    cases.append((3 * B, 0, B, []))                 # no ranges
    # the (n, unit) and ranges of test_high_positions' raw cases: units around 2^32 of a stream of more
    # than 4 GiB, and the same moved to 2^40 - 2^16 and 2^62 (no GPU test goes above 2^33)
    cases += hp.raw_plan_cases()
    return cases


def expected_lines(cases):
    out = []
    for n, out_bytes, unit, r in cases:
        if unit == 0 or unit > B:
            out.append("case -1 0 0")
            continue
        st, units = rm.plan(n, unit, r, out_bytes)
        out.append(f"case 0 {len(units)} {sum(1 for u in units if u[5])}")
        out += [f"r {s}" for s in st]
        out += ["u %d %d %d %d %d %d" % u for u in units]
    return out


def test_plan_rule_under_asan_and_ubsan(tmp_path):
    # clang links the sanitizer runtime into the program; gcc is told to (as tests/host_check does)
    clang = os.environ.get("CLANG", "/opt/rocm/lib/llvm/bin/clang")
    if os.path.exists(clang):
        cc_cmd = [clang]
    else:
        assert shutil.which("gcc"), "no C compiler"
        cc_cmd = ["gcc", "-static-libasan", "-static-libubsan"]
    cases = build_cases()
    data = tmp_path / "cases.bin"
    blob = struct.pack("<I", len(cases))
    for n, out_bytes, unit, r in cases:
        blob += struct.pack("<QQII", n, out_bytes, unit, len(r)) + b"".join(struct.pack("<QQQ", *x) for x in r)
    data.write_bytes(blob)
    exe = tmp_path / "ranges_plan_check"
    b = subprocess.run(cc_cmd + ["-std=gnu11", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                                 "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "include"),
                                 "-I", os.path.join(ROOT, "lightweight-snappy_amd", "csrc"), SRC, "-o", str(exe)],
                       capture_output=True, text=True)
    assert b.returncode == 0, b.stderr[-4000:]
    r = subprocess.run([str(exe), str(data)], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    got = r.stdout.split("\n")[:-1]
    want = expected_lines(cases)
    assert len(got) == len(want) > 1000
    bad = [(i, g, w) for i, (g, w) in enumerate(zip(got, want)) if g != w]
    assert not bad, bad[:10]
    # the cases reach every status and both kinds of unit
    assert {"r 0", "r -1", "r -6"} <= set(want)
    assert any(w.startswith("u ") and w.endswith(" 0") for w in want)
    assert any(w.startswith("u ") and not w.endswith(" 0") for w in want)

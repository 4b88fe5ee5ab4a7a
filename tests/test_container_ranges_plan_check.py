"""CPU: the plan rule that the device kernels and the host forms of the container
range decode share (csrc/snappy_container_ranges.h), compiled as plain C into a
stand-alone program with AddressSanitizer and UBSan
(tests/container_ranges_plan_check.c) and run on chunk tables and ranges at every
edge of the rule -- sorted, unsorted, constant and non-contiguous tables,
sub-tables, no chunks at all, ranges that wrap past 2^64, windows cut at every
edge of a chunk -- each array in an exactly sized heap block.  Every status, every
unit entry, every staging place and every table verdict must be the Python
model's (tests/container_ranges_model.py).  Nothing is loaded into this process."""
import os
import shutil
import struct
import subprocess

import container_cases as cc
import container_model as cm
import container_ranges_cases as rc
import container_ranges_model as crm
import high_positions as hp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "container_ranges_plan_check.c")
U64 = crm.U64
BUDGET = 1 << 26


def edge_ranges(outp):
    """ranges at the rule's edges for a (sub-)table, whatever its order"""
    s0 = outp[0][0] if outp else 0
    s1 = (outp[-1][0] + outp[-1][1]) & U64 if outp else 0
    r = [(s0, 0), (s0, 1), (s1, 0), (s1, 1), ((s1 - 1) & U64, 1), ((s1 - 1) & U64, 2), (s0, (s1 - s0) & U64),
         (s0, (s1 - s0 + 1) & U64), ((s0 - 1) & U64, 1), ((s0 - 1) & U64, 2), ((s1 + 1) & U64, 0), (U64, 1), (U64, U64),
         (1, U64), (U64 - 5, 10), (5, U64 - 4), (1 << 63, 1 << 63), (s0, U64), ((s0 + 1) & U64, U64)]
    for b, size in outp:
        e = (b + size) & U64
        r += [((b - 1) & U64, 1), ((b - 1) & U64, 2), (b, 1), (b, 0), (b, 2), (b, size), (b, (size + 1) & U64),
              ((b + 1) & U64, size), ((e - 1) & U64, 1), ((e - 1) & U64, 2), (e, 1), ((b - 1) & U64, (size + 2) & U64)]
    out, oo = [], 3
    for k, (a, ln) in enumerate(r):
        out.append((a, ln, oo))
        oo += (ln if ln < 1 << 20 else 0) + k % 16 + 1
    return out, oo


def table_checks():
    """(payload bytes, co, cl, w0, w1, size, hi) for unit_check: every chunk of small
    containers through windows cut at the payload's edges, and tables that disagree
    with the chunk"""
    out = []
    streams = [rc.SLICE[n]() for n in ("hadoop: one block of five chunks (1, 17, 64, 200, 3)",
                                       "xerial: chunks of 200, 0, 1, 16, 33, the header again inside")]
    streams.append((cm.HADOOP, cc.two_byte_varint(), None))
    for fmt, stream, _ in streams:
        comp, outp, _ = crm.tables(stream, fmt)
        n = len(stream)
        for (co, cl), (_, size) in zip(comp, outp):
            five = lambda at, ln: bytes(stream[at:at + min(ln, 5)])  # noqa: E731
            for w0, w1 in ((0, n), (co, co + cl), (co + 1, n), (0, co + cl - 1), (0, co), (0, co + 2), (co, co),
                           (co + cl, n), (0, 0)):
                for hi in (1, size, crm.BAD):
                    out.append((five(co, cl), co, cl, w0, w1, size, hi))
            # tables that disagree with the chunk: a length off by one, no payload, a payload
            # begun late or cut short (the preamble's bytes are then others), one past 2^64
            out.append((five(co, cl), co, cl, 0, n, size + 1, 1))
            out.append((five(co, cl), co, cl, 0, n, (1 << 30) + 1, crm.BAD))
            out.append((b"", co, 0, 0, n, size, 1))
            out.append((five(co + 1, cl - 1), co + 1, cl - 1, 0, n, size, 1))
            out.append((five(co, 1), co, 1, 0, n, size, 1))
            out.append((b"", co, U64, 0, n, size, 1))
            out.append((b"", U64, 2, 0, n, size, 1))
    out.append((b"\x80\x80\x80\x80\x80", 4, 9, 0, 100, 0, 1))     # a preamble of more than five bytes
    out.append((b"\x80\x80\x80\x80\x04", 4, 9, 0, 100, 1 << 30, 1))   # 2^30 in five bytes
    return out


def build_cases():
    cases = []
    tabs = [crm.tables(*reversed(rc.SLICE[name]()[:2]))[1] for name in rc.SLICE]
    base = tabs[3]                                      # (0, 1) (1, 17) (18, 64) (82, 200) (282, 3)
    tabs.append([])                                     # no chunks
    tabs.append([(0, 0)])                               # one empty chunk
    tabs.append([(5, 0)])
    tabs.append([(0, 1 << 30)])
    tabs.append([(0, (1 << 30) + 1)])                   # a chunk no container holds
    tabs.append(base[2:4])                              # sub-tables: offsets stay absolute
    tabs.append(base[1:])
    tabs.append(base[3:4])
    swapped = list(base)
    swapped[2], swapped[3] = swapped[3], swapped[2]
    tabs.append(swapped)                                # not sorted
    tabs.append(list(reversed(base)))
    tabs.append([base[3]] * 5)                          # constant
    tabs.append([(7, 2), (7, 2), (7, 2), (9, 4), (9, 4), (9, 4)])
    tabs.append([(0, 10), (12, 10), (22, 10)])          # not contiguous: a hole
    tabs.append([(0, 10), (8, 10), (18, 10)])           # overlapping
    tabs.append([(0, 10), (10, 0), (10, 0), (10, 5)])   # empty chunks inside
    tabs.append([(0, 0), (0, 0), (0, 5), (5, 0)])       # ... at the ends
    tabs.append([(U64 - 10, 7), (U64 - 3, 3)])          # at the top of the positions
    tabs.append([(U64 - 10, 7), (U64 - 3, 9)])          # an extent that wraps
    tabs.append([(100, 10), (50, 10), (200, 10), (150, 10), (300, 10)])
    tabs.append([(0, 5), (5, (1 << 30) + 1), ((1 << 30) + 6, 5)])   # a length above 2^30 inside a span
    for t in tabs:
        r, need = edge_ranges(t)
        cases.append((need + 16, BUDGET, t, r, []))
        cases.append((need // 2, 64, t, r + [(t[0][0] if t else 0, 0, need // 2), (t[0][0] if t else 0, 0, need // 2 + 1),
                                             (t[0][0] if t else 0, 0, U64)], []))
    for name in list(rc.SLICE)[:4]:
        fmt, stream, raw, comp, outp, ranges, out_bytes = rc.slice_case(name)
        cases.append((out_bytes, 4096, outp, ranges, []))
    # the shifted chunk tables and ranges of test_high_positions' container cases (one with an entry's
    # length raised by 1): offsets around 2^32, and the same moved to 2^40 - 2^16 and 2^62 (no GPU test
    # goes above 2^33); a staging budget of three blocks, as with SNAPPY_AMD_RANGE_SLOTS=3
    cases += [(out_bytes, 3 * 65536, outp, ranges, []) for out_bytes, outp, ranges in hp.container_plan_cases()]
    cases.append((0, BUDGET, [(0, 10)], [], table_checks()))
    return cases


def expected_lines(cases):
    out = []
    for out_bytes, budget, outp, r, checks in cases:
        st, units = crm.plan(outp, r, out_bytes)
        out.append(f"case {len(units)} {sum(1 for u in units if u[5])}")
        out += [f"r {s}" for s in st]
        out += ["u %d %d %d %d %d %d" % u for u in units]
        places, gstart, stage = crm.pack(outp, units, budget)
        out += ["s %d %d %d" % (p, places[e[5]], p in gstart[1:]) for p, e in enumerate(units) if e[5]]
        out.append(f"stage {stage}")
        out += ["k %d" % crm.unit_check(*c) for c in checks]
    return out


def test_container_plan_rule_under_asan_and_ubsan(tmp_path):
    # clang links the sanitizer runtime into the program; gcc is told to (as tests/host_check does)
    clang = os.environ.get("CLANG", "/opt/rocm/lib/llvm/bin/clang")
    if os.path.exists(clang):
        cc_cmd = [clang]
    else:
        assert shutil.which("gcc"), "no C compiler"
        cc_cmd = ["gcc", "-static-libasan", "-static-libubsan"]
    cases = build_cases()
    data = tmp_path / "cases.bin"
    blob = [struct.pack("<I", len(cases))]
    for out_bytes, budget, outp, r, checks in cases:
        blob.append(struct.pack("<QQIII", out_bytes, budget, len(outp), len(r), len(checks)))
        blob.append(b"".join(struct.pack("<QQ", *p) for p in outp) + b"".join(struct.pack("<QQQ", *x) for x in r))
        for w, co, cl, w0, w1, size, hi in checks:
            blob.append(w.ljust(5, b"\0")[:5] + struct.pack("<QQQQQI", co, cl, w0, w1, size, hi))
    data.write_bytes(b"".join(blob))
    exe = tmp_path / "container_ranges_plan_check"
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
    # the cases reach every status, every kind of unit, group openings and every table verdict
    # (ERR_INDEX for u1 < u0 is a guard no table reaches: the search's answer cannot fall when
    # the position rises, sorted table or not -- every comparison that held still holds -- so
    # on the unsorted and constant tables above the units' own checks do the refusing)
    assert {"r 0", "r -1", "r -6"} <= set(want) and "r -11" not in want
    units = [w.split() for w in want if w.startswith("u ")]
    assert any(u[6] == "0" and u[5] not in ("0", str(crm.BAD)) for u in units)   # interior
    assert any(u[6] != "0" and int(u[6]) % 2 == 1 for u in units)                # a first edge
    assert any(u[6] != "0" and int(u[6]) % 2 == 0 for u in units)                # a last edge
    assert any(u[5] == "0" for u in units)                                       # empty inside a span
    assert any(u[5] == str(crm.BAD) for u in units)                              # the tables contradict themselves
    staged = [w.split() for w in want if w.startswith("s ")]
    assert any(s[3] == "1" for s in staged) and any(s[3] == "0" and s[2] != "0" for s in staged)
    assert {"k 0", "k -2", "k -3", "k -9", "k -11"} <= set(want)

"""CPU: the plan rule that the device kernels and the host forms of the framed
range decode share (csrc/snappy_frame_ranges.h), compiled as plain C into a
stand-alone program with AddressSanitizer and UBSan
(tests/frame_ranges_plan_check.c) and run on seek tables and ranges at every edge
of the rule -- sorted, unsorted and constant tables, sub-tables, no chunks at all,
ranges that wrap past 2^64 -- each array in an exactly sized heap block.  Every
status, every unit entry and every header verdict must be the Python model's
(tests/frame_ranges_model.py).  Nothing is loaded into this process."""
import os
import shutil
import struct
import subprocess

import frame_model as fm
import frame_ranges_cases as fc
import frame_ranges_model as frm
import high_positions as hp
from test_frame import FOREIGN, comp, pieces

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "frame_ranges_plan_check.c")
U64 = frm.U64


def edge_ranges(starts):
    """ranges at the rule's edges for a (sub-)table, whatever its order"""
    s0, s1 = starts[0], starts[-1]
    r = [(s0, 0), (s0, 1), (s1, 0), (s1, 1), ((s1 - 1) & U64, 1), ((s1 - 1) & U64, 2), (s0, (s1 - s0) & U64),
         (s0, (s1 - s0 + 1) & U64), ((s0 - 1) & U64, 1), ((s0 - 1) & U64, 2), ((s1 + 1) & U64, 0), (U64, 1), (U64, U64),
         (1, U64), (U64 - 5, 10), (5, U64 - 4), (1 << 63, 1 << 63), (s0, U64), (s0 + 1, U64)]
    for b in starts:
        r += [((b - 1) & U64, 1), ((b - 1) & U64, 2), (b, 1), (b, 0), (b, 2), ((b + 1) & U64, 65536), (b, 65536), (b, 65537)]
    out, oo = [], 3
    for k, (a, ln) in enumerate(r):
        out.append((a, ln, oo))
        oo += (ln if ln < 1 << 20 else 0) + k % 16 + 1
    return out, oo


def header_checks():
    """(stream, chunks, starts, u, hi, w0, w1) for unit_check: every chunk of streams
    with padding, stored and empty chunks and of broken chunks, through windows cut
    at the chunk's edges"""
    out = []
    p = pieces([300, 200], "R")
    broken = [fm.chunk(0x00, b"abc"), fm.chunk(0x02, b"abcdef"), fm.chunk(0x00, bytes(4) + fm.varint(65537) + b"\x00a"),
              fm.chunk(0x00, bytes(4) + b"\x80\x80\x80\x80\x80"), fm.padding(3), fm.IDENTIFIER, fm.stored(p[1])]
    streams = [FOREIGN[n]()[0] for n in ("padding of 0 and of 7 bytes", "empty chunks between full ones",
                                         "stored chunks of 1 byte")]
    for b in broken:
        streams.append(fm.IDENTIFIER + comp(p[0]) + b + comp(p[1]))
    for stream in streams:
        # the table of whatever follows the identifier, data chunk or not, with sizes from the walk where it knows them
        pos, chunks = 10, []
        while pos < len(stream):
            chunks.append(pos)
            pos += 4 + (stream[pos + 1] | stream[pos + 2] << 8 | stream[pos + 3] << 16)
        chunks.append(len(stream))
        starts, total = [], 0
        for c in chunks[:-1]:
            st, kind, ln, d = frm.chunk_info(stream, c)
            starts.append(total)
            total += d if st == frm.OK else 7
        starts.append(total)
        for u in range(len(chunks) - 1):
            size = starts[u + 1] - starts[u]
            for w0, w1 in ((0, len(stream)), (chunks[u], chunks[u + 1]), (chunks[u] + 1, len(stream)),
                           (0, chunks[u + 1] - 1), (0, chunks[u] + 3), (0, chunks[u] + 9), (0, chunks[u])):
                for hi in (1, size, size + 1, frm.BAD):
                    out.append((stream, chunks, starts, u, hi, w0, w1))
            # tables that disagree with the chunk: a size off by one, a next entry inside the chunk
            bad = list(starts)
            bad[u + 1] += 1
            out.append((stream, chunks, bad, u, 1, 0, len(stream)))
            near = list(chunks)
            near[u + 1] -= 1
            out.append((stream, near, starts, u, 1, 0, len(stream)))
            near[u + 1] = 0
            out.append((stream, near, starts, u, 1, 0, len(stream)))
    return out


def build_cases():
    cases = []
    tabs = []
    for name in fc.SLICE_STREAMS:
        tabs.append(fc.tables(FOREIGN[name]()[0])[1])
    base = tabs[0]
    tabs.append([0])                                    # no chunks
    tabs.append([5])
    tabs.append([0, 0])                                 # one empty chunk
    tabs.append([0, 65536])
    tabs.append([0, 65537])                             # a chunk no stream holds
    tabs.append(base[2:5])                              # sub-tables: positions stay absolute
    tabs.append(base[1:])
    tabs.append(base[3:4])
    swapped = list(base)
    swapped[2], swapped[3] = swapped[3], swapped[2]
    tabs.append(swapped)                                # not sorted
    tabs.append(list(reversed(base)))
    tabs.append([base[3]] * 5)                          # constant
    tabs.append([7, 7, 7, 9, 9, 9])
    tabs.append([base[0]] + [base[3]] * 4 + [base[-1]])
    tabs.append([U64 - 10, U64 - 3, U64])               # at the top of the positions
    tabs.append([100, 50, 200, 150, 300])
    for s in tabs:
        r, need = edge_ranges(s)
        cases.append((need + 16, s, r, []))
        cases.append((need // 2, s, r + [(s[0], 0, need // 2), (s[0], 0, need // 2 + 1), (s[0], 0, U64)], []))
    for name in fc.SLICE_STREAMS:
        chunks, starts, ranges, out_bytes = fc.slice_case(FOREIGN[name]()[0])
        cases.append((out_bytes, starts, ranges, []))
    # the shifted seek tables and ranges of test_high_positions' framed cases: starts around 2^32, and the
    # same moved to 2^40 - 2^16 and 2^62 (no GPU test goes above 2^33)
    cases += [(out_bytes, starts, ranges, []) for out_bytes, starts, ranges in hp.frame_plan_cases()]
    cases.append((0, [0, 10], [], header_checks()))
    return cases


def expected_lines(cases):
    out = []
    for out_bytes, starts, r, checks in cases:
        st, units = frm.plan(starts, r, out_bytes)
        out.append(f"case {len(units)} {sum(1 for u in units if u[5])}")
        out += [f"r {s}" for s in st]
        out += ["u %d %d %d %d %d %d" % u for u in units]
        out += ["k %d" % frm.unit_check(s, ch, ss, u, hi, w0, w1) for s, ch, ss, u, hi, w0, w1 in checks]
    return out


def test_frame_plan_rule_under_asan_and_ubsan(tmp_path):
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
    for out_bytes, starts, r, checks in cases:
        blob += struct.pack("<QIII", out_bytes, len(starts) - 1, len(r), len(checks))
        blob += struct.pack(f"<{len(starts)}Q", *starts) + b"".join(struct.pack("<QQQ", *x) for x in r)
        for s, ch, ss, u, hi, w0, w1 in checks:
            pos = ch[u]
            w = bytes(s[pos:min(pos + 16, w1)]) if w0 <= pos < w1 else b""
            blob += w.ljust(16, b"\0") + struct.pack("<QQQQQI", pos, ch[u + 1], w0, w1, (ss[u + 1] - ss[u]) & U64, hi)
    data.write_bytes(blob)
    exe = tmp_path / "frame_ranges_plan_check"
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
    # the cases reach every status, every kind of unit and every header verdict
    # (ERR_INDEX for u1 < u0 is a guard no table reaches: the search's answer cannot fall when
    # the position rises, sorted table or not -- every comparison that held still holds -- so
    # on the unsorted and constant tables above the units' own checks do the refusing)
    assert {"r 0", "r -1", "r -6"} <= set(want) and "r -11" not in want
    units = [w.split() for w in want if w.startswith("u ")]
    assert any(u[6] == "0" and u[5] not in ("0", str(frm.BAD)) for u in units)   # interior
    assert any(u[6] != "0" for u in units)                                       # edge
    assert any(u[5] == "0" for u in units)                                       # empty inside a span
    assert any(u[5] == str(frm.BAD) for u in units)                              # the tables contradict themselves
    assert {"k 0", "k -2", "k -3", "k -5", "k -9", "k -11"} <= set(want)

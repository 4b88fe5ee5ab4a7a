"""CPU: the model of range decode over a framed stream (tests/frame_ranges_model.py)
against the reference bytes, and that the planted inputs of the GPU tests
(tests/frame_ranges_cases.py) reach every case of the rule."""
import frame_model as fm
import frame_ranges_cases as fc
import frame_ranges_model as frm
from test_frame import FOREIGN


def planned(name):
    stream, raw = FOREIGN[name]()
    chunks, starts, ranges, out_bytes = fc.slice_case(stream)
    st, units = frm.plan(starts, ranges, out_bytes)
    return stream, raw, chunks, starts, ranges, out_bytes, st, units


def test_seek_table_is_the_running_sum_of_the_chunks():
    for name, make in FOREIGN.items():
        stream, raw = make()
        st, chunks, total = fm.chunk_table(stream)
        st, starts = frm.seek_table(stream, chunks)
        assert st == frm.OK and len(starts) == len(chunks) and starts[0] == 0 and starts[-1] == len(raw) == total
        assert all(a <= b and b - a <= frm.CH for a, b in zip(starts, starts[1:]))


def test_the_plan_cuts_exactly_the_slices():
    for name in fc.SLICE_STREAMS:
        stream, raw, chunks, starts, ranges, out_bytes, st, units = planned(name)
        assert st == [frm.OK] * len(ranges) and len(ranges) > 30
        buf = bytearray([fc.SENT]) * out_bytes
        for u, land, r, lo, hi, edge in units:
            assert hi != frm.BAD and 0 <= lo <= hi <= starts[u + 1] - starts[u]
            buf[land + lo:land + hi] = raw[starts[u] + lo:starts[u] + hi]
        assert bytes(buf) == fc.expected(raw, ranges, out_bytes)
        # edge units are numbered 1, 2, ... in plan order
        assert [e[5] for e in units if e[5]] == list(range(1, 1 + sum(1 for e in units if e[5])))


def test_planted_ranges_reach_every_case():
    seen = set()
    for name in fc.SLICE_STREAMS:
        stream, raw, chunks, starts, ranges, out_bytes, st, units = planned(name)
        by_range = {}
        for e in units:
            by_range.setdefault(e[2], []).append(e)
        for i, (a, ln, oo) in enumerate(ranges):
            us = by_range[i]
            if any(e[5] == 0 and e[4] > 0 for e in us):
                seen.add("interior")
            if any(e[4] == 0 for e in us):
                seen.add("empty inside")
                assert us[0][4] > 0 and us[-1][4] > 0  # never a span's first or last unit
            if len(us) == 1 and us[0][5]:
                seen.add("single edge")
            if len(us) > 1 and us[0][5] and not us[-1][5]:
                seen.add("first only")
            if len(us) > 1 and us[-1][5] and not us[0][5]:
                seen.add("last only")
            if len(us) > 1 and us[0][5] and us[-1][5]:
                seen.add("both edges")
            u0 = us[0][0]
            if u0 > 0 and starts[u0 - 1] == starts[u0] == a:
                seen.add("empty at start")
            if a + ln in starts[1:] and us[-1][4] == starts[us[-1][0] + 1] - starts[us[-1][0]]:
                seen.add("ends on a last byte")
            if a + ln - 1 in starts[1:-1] and us[-1][4] == 1 and len(us) > 1:
                seen.add("ends on a first byte")
        offs = [oo % 16 for _, _, oo in ranges[-16:]]
        assert sorted(offs) == list(range(16))
    assert seen == {"interior", "empty inside", "single edge", "first only", "last only", "both edges", "empty at start",
                    "ends on a last byte", "ends on a first byte"}


def test_hostile_tables_never_plan_outside_the_range():
    stream, raw = FOREIGN["three runs"]()
    chunks, starts = fc.tables(stream)
    hostile = []
    s = list(starts)
    s[2], s[3] = s[3], s[2]
    hostile.append(s)
    s = list(starts)
    s[2] += 1
    hostile.append(s)
    hostile.append([starts[0]] + [starts[3]] * (len(starts) - 2) + [starts[-1]])
    for k, s in enumerate(hostile):
        ranges, out_bytes = fc.lay_out(fc.slice_spans(starts))
        st, units = frm.plan(s, ranges, out_bytes)
        # (an entry raised by 1 leaves a consistent table: only the header stage can tell)
        assert k == 1 or frm.ERR_INDEX in st or any(e[4] == frm.BAD for e in units)
        for u, land, r, lo, hi, edge in units:
            if hi in (0, frm.BAD):
                assert edge == 0
                continue
            a, ln, oo = ranges[r]
            assert 0 <= lo < hi <= frm.CH and oo <= land + lo and land + hi <= oo + ln

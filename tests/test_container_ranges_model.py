"""CPU: the model of the container range decode (tests/container_ranges_model.py)
pinned to plain bytes, and the proof that the planted inputs of
tests/container_ranges_cases.py reach every case the GPU tests rest on.  Each case
is asserted through the model's own classification of the range, not assumed."""
import random

import pytest

import container_cases as cc
import container_model as cm
import container_ranges_cases as rc
import container_ranges_model as crm

FORMATS = [cm.HADOOP, cm.XERIAL]


def assemble(stream, comp, outp, ranges, out_bytes):
    """the output buffer the plan gives: every unit's wanted bytes of its decoded chunk
    at land + [lo, hi)"""
    chunks = {}
    st, units = crm.plan(outp, ranges, out_bytes)
    assert st == [0] * len(ranges)
    buf = bytearray([rc.SENT]) * out_bytes
    for u, land, i, lo, hi, edge in units:
        assert hi != crm.BAD
        if hi == 0:
            continue
        if u not in chunks:
            at, c = comp[u]
            chunks[u] = rc.decode(stream[at:at + c])
            assert len(chunks[u]) == outp[u][1]
        a, ln, oo = ranges[i]
        at = (land + lo) & crm.U64                              # (land is taken mod 2^64)
        assert oo <= at and at + hi - lo <= oo + ln             # the write bound
        buf[at:at + hi - lo] = chunks[u][lo:hi]
    return bytes(buf), units


# ---- hand-written vectors ------------------------------------------------------
def test_span_units_and_packing_by_hand():
    outp = [(0, 0), (0, 10), (10, 0), (10, 20)]                 # cc: chunks of no bytes inside a block
    assert [crm.seek(outp, p) for p in (0, 9, 10, 29)] == [1, 1, 3, 3]
    assert crm.span(outp, (0, 30, 0), 30) == (0, 1, 3, 3)
    assert crm.span(outp, (0, 31, 0), 31) == (crm.ERR_ARG, 0, 0, 0)
    assert crm.span(outp, (30, 0, 0), 0) == (0, 0, 0, 0)
    assert crm.span(outp, (31, 0, 0), 0) == (crm.ERR_ARG, 0, 0, 0)
    assert crm.span(outp, (3, 4, 7), 10) == (crm.ERR_CAPACITY, 0, 0, 0)
    assert crm.span([], (0, 0, 0), 0) == (0, 0, 0, 0) and crm.span([], (0, 1, 0), 1)[0] == crm.ERR_ARG
    st, units = crm.plan(outp, [(0, 30, 5), (3, 20, 40), (10, 20, 70), (9, 2, 100)], 200)
    assert st == [0, 0, 0, 0]
    assert units == [(1, 5, 0, 0, 10, 0), (2, 15, 0, 0, 0, 0), (3, 15, 0, 0, 20, 0),
                     (1, 37, 1, 3, 10, 3), (2, 47, 1, 0, 0, 0), (3, 47, 1, 0, 13, 4),
                     (3, 70, 2, 0, 20, 0),
                     (1, 91, 3, 9, 10, 7), (2, 101, 3, 0, 0, 0), (3, 101, 3, 0, 1, 8)]
    # edge chunks of 10 and 20 bytes stage at 16-byte places; a budget of 48 holds three of the four
    assert crm.pack(outp, units, 1 << 26) == ({3: 0, 4: 16, 7: 48, 8: 64}, [0], 96)
    assert crm.pack(outp, units, 48) == ({3: 0, 4: 16, 7: 0, 8: 16}, [0, 7], 48)
    assert crm.pack(outp, units, 16) == ({3: 0, 4: 0, 7: 0, 8: 0}, [0, 5, 7, 9], 32)   # a chunk above the budget: alone


def test_hostile_tables_by_hand():
    good = [(0, 10), (10, 10), (20, 10)]
    whole = (2, 26, 0)
    bad = lambda outp, rng=whole: [e[4] == crm.BAD for e in crm.plan(outp, [rng], 64)[1]]  # noqa: E731
    assert bad(good) == [False, False, False]
    assert bad([(0, 10), (11, 9), (20, 10)]) == [True, False, False]      # a hole behind chunk 0
    assert bad([(0, 10), (10, 11), (20, 10)]) == [False, True, False]     # chunk 1 runs into chunk 2
    assert bad([(0, 10), (10, 10), (20, 7), (40, 9)]) == [False, False, True]  # the range ends in a hole behind chunk 2
    assert crm.span([(0, 10), (10, 10), (20, 7)], whole, 64)[0] == crm.ERR_ARG  # (past the last chunk: the extent's)
    assert bad([(0, 10), (1, 10), (20, 10)]) == [True, False]             # the search starts at chunk 1, which overlaps
    assert bad([(0, 10), (10, 10), (15, 5), (20, 10)]) == [False, True, False, False]
    # not sorted: entry 5 is never probed by the search for 12, and begins before the range
    assert bad([(10, 2), (12, 2), (14, 2), (16, 2), (18, 2), (3, 2), (22, 2), (24, 2)], (12, 13, 0)) == \
        [False, False, False, True, True, False, False]
    assert bad([(0, 10), (10, 0), (20, 10)]) == [False, True, False]      # a hole behind an empty chunk
    assert bad([(0, 10), (10, 0), (10, 10)], (2, 16, 0)) == [False, False, False] and \
        crm.plan([(0, 10), (10, 0), (10, 10)], [(2, 16, 0)], 64)[1][1][4] == 0
    assert bad([(0, 0), (10, 10)], (0, 5, 0)) == [True]                   # an empty first chunk
    assert bad([(0, 10), (10, (1 << 30) + 1)], (2, 10, 0)) == [False, True]
    assert bad([(0, 10), (10, 1 << 30)], (2, 10, 0)) == [False, False]
    # whatever the table says, a unit that is not refused lies inside its range
    rnd = random.Random(5)
    seen = 0
    for _ in range(3000):
        outp = [(rnd.randrange(0, 40), rnd.choice([0, 1, 5, 10, 20])) for _ in range(rnd.randrange(1, 6))]
        if rnd.random() < 0.5:
            outp.sort()
        rng = (rnd.randrange(0, 50), rnd.randrange(0, 40), 7)
        st, units = crm.plan(outp, [rng], 100)
        for u, land, i, lo, hi, edge in units:
            if hi not in (0, crm.BAD):
                seen += 1
                assert 0 <= lo < hi <= outp[u][1] and rng[0] <= outp[u][0] + lo and outp[u][0] + hi <= rng[0] + rng[1]
                assert land == 7 + outp[u][0] - rng[0] or outp[u][0] < rng[0]
    assert seen > 200
    # the verdict, in its order
    pre = cm.varint(300)
    chk = lambda **k: crm.unit_check(**{**dict(payload5=pre + b"\x00\x00\x00", co=100, cl=9, w0=50, w1=200,  # noqa: E731
                                               size=300, hi=300), **k})
    assert chk() == 0
    assert chk(co=49) == chk(co=192) == chk(cl=101) == crm.ERR_TRUNCATED and chk(co=191) == 0
    assert chk(cl=0) == crm.ERR_HEADER and chk(cl=0, co=200) == crm.ERR_HEADER and chk(cl=1, co=200) == crm.ERR_TRUNCATED
    assert chk(size=(1 << 30) + 1, hi=crm.BAD) == crm.ERR_UNSUPPORTED
    assert chk(hi=crm.BAD) == crm.ERR_INDEX
    assert chk(size=299, hi=1) == crm.ERR_HEADER and chk(cl=1) == crm.ERR_HEADER
    assert chk(payload5=b"\x80" * 5, cl=9) == crm.ERR_HEADER


# ---- the planted inputs --------------------------------------------------------
@pytest.mark.parametrize("name", list(rc.SLICE))
def test_every_slice_is_the_plain_bytes(name):
    fmt, stream, raw, comp, outp, ranges, out_bytes = rc.slice_case(name)
    assert all(0 <= size <= 300 for _, size in outp)
    got, units = assemble(stream, comp, outp, ranges, out_bytes)
    assert got == rc.expected(raw, ranges, out_bytes)
    # an empty chunk is never a span's first or last unit on a sorted table
    assert all(e[4] != 0 or e[5] == 0 for e in units)
    kinds = set().union(*(crm.classify(outp, r, out_bytes) for r in ranges))
    assert "bad" not in kinds and "refused" not in kinds and "empty" in kinds
    if len([1 for _, size in outp if size]) >= 3 and max(size for _, size in outp) > 1:
        assert {"interior", "both edges", "first edge", "last edge", "single edge", "single whole", "no edge"} <= kinds
    # every residue of the output against the start, for edge units at either end
    for which in (1, 2):
        res = {(ranges[e[2]][2] - ranges[e[2]][0]) % 16 for e in units if e[5] and (e[5] - 1) % 2 + 1 == which}
        assert res == set(range(16)) or (len(outp) == 1 and which == 2) or max(size for _, size in outp) == 1


def test_slice_containers_hold_the_cases():
    by = {name: rc.slice_case(name) for name in rc.SLICE}
    assert sorted(fmt for fmt, *_ in by.values()) == [cm.HADOOP] * 5 + [cm.XERIAL] * 5
    # an empty chunk inside a span, and at a range's start (where the search passes over it)
    for name in ("hadoop: chunks of no bytes inside a block", "xerial: chunks of 200, 0, 1, 16, 33, the header again inside"):
        fmt, stream, raw, comp, outp, ranges, out_bytes = by[name]
        kinds = [crm.classify(outp, r, out_bytes) for r in ranges]
        assert any("empty chunk inside" in k for k in kinds)
        empty_at = {o for o, size in outp if size == 0}
        starts_there = [r for r in ranges if r[0] in empty_at and r[1]]
        assert starts_there and all(outp[crm.span(outp, r, out_bytes)[1]][1] != 0 for r in starts_there)
    # a Hadoop block of several chunks: the walk's open block is carried over them
    fmt, stream, *_ = by["hadoop: one block of five chunks (1, 17, 64, 200, 3)"]
    assert stream[:4] == cm.be32(285) and len(crm.tables(stream, fmt)[0]) == 5
    # a repeated snappy-java header between two chunks of one span
    fmt, stream, raw, comp, outp, ranges, out_bytes = by["xerial: chunks of 200, 0, 1, 16, 33, the header again inside"]
    gap = [comp[u + 1][0] - (comp[u][0] + comp[u][1]) for u in range(len(comp) - 1)]
    assert gap == [4, 4, 20, 4] and stream[comp[3][0] - 20:comp[3][0] - 12] == cm.MAGIC
    assert any(crm.span(outp, r, out_bytes)[1:3] == (2, 3) for r in ranges)
    # copies inside the chunks of the two containers made for them
    for name in ("hadoop: chunks of copies, an empty block between", "xerial: chunks of copies"):
        fmt, stream, raw, comp, outp, *_ = by[name]
        assert any(stream[at + 2 + 0] & 3 == 0 and any(b & 3 == 2 for b in stream[at:at + c]) for at, c in comp)


@pytest.mark.parametrize("fmt", FORMATS)
def test_long_chunks_hold_the_cases(fmt):
    stream, raw = rc.long_case(fmt)
    comp, outp, total = crm.tables(stream, fmt)
    assert [size for _, size in outp] == [300, 65537, 131072, 65536, 196609, 77] and total == len(raw)
    if fmt == cm.HADOOP:
        assert stream[:4] == cm.be32(total)                     # one block of six chunks
    else:
        assert [comp[u + 1][0] - (comp[u][0] + comp[u][1]) for u in range(5)] == [4, 20, 4, 4, 20]
    ranges, out_bytes = rc.lay_out(rc.long_spans(outp))
    got, units = assemble(stream, comp, outp, ranges, out_bytes)
    assert got == rc.expected(raw, ranges, out_bytes)
    for u in (1, 2, 3, 4):
        mine = [e for e in units if e[0] == u]
        size = outp[u][1]
        assert any(e[5] == 0 and (e[3], e[4]) == (0, size) and crm.span(outp, ranges[e[2]], out_bytes)[3] > 1
                   for e in mine)                               # interior
        assert any(e[5] % 2 == 1 and e[3] > 0 and e[4] == size for e in mine)     # a first edge
        assert any(e[5] and e[5] % 2 == 0 and e[3] == 0 and e[4] < size for e in mine)  # a last edge
        assert any(e[5] % 2 == 1 and e[3] > 0 and e[4] < size for e in mine)      # a single edge unit
        assert any(e[5] == 0 and crm.span(outp, ranges[e[2]], out_bytes)[3] == 1 for e in mine)  # single, whole
    # a range ending on a chunk's last byte, and on the next chunk's first
    ends = {r[0] + r[1] for r in ranges}
    assert all(outp[u][0] + outp[u][1] in ends and outp[u][0] + outp[u][1] + 1 in ends for u in (1, 2, 3, 4))
    # the foreign chunk defers in pass 1: its second block copies from its first; no other chunk does
    at, c = comp[2]
    assert crm.defers_in_pass_one(stream[at:at + c])
    assert not any(crm.defers_in_pass_one(stream[a:a + n]) for a, n in comp[:2] + comp[3:])
    assert not crm.defers_in_pass_one(rc.repeated(b"abc", 300))


def test_statuses_of_the_model():
    fmt, stream, raw = rc.SLICE["hadoop: one block of five chunks (1, 17, 64, 200, 3)"]()
    comp, outp, total = crm.tables(stream, fmt)
    ok = lambda payload: 0  # noqa: E731
    whole = (0, total, 0)
    assert crm.range_status(stream, comp, outp, whole, total, ok) == (0, False)
    # a window one byte short at either end, a payload moved, an emptied one, a wrong length
    assert crm.range_status(stream, comp, outp, whole, total, ok, w1=len(stream) - 1) == (crm.ERR_TRUNCATED, True)
    assert crm.range_status(stream, comp, outp, whole, total, ok, w0=comp[0][0] + 1) == (crm.ERR_TRUNCATED, True)
    assert crm.range_status(stream, comp, outp, (1, 10, 0), total, ok, w0=comp[1][0], w1=comp[1][0] + comp[1][1]) == \
        (0, False)
    moved = list(comp)
    moved[2] = (comp[2][0] + 4, comp[2][1])
    assert crm.range_status(stream, moved, outp, whole, total, ok) == (crm.ERR_HEADER, True)
    moved[2] = (comp[2][0], 0)
    assert crm.range_status(stream, moved, outp, whole, total, ok) == (crm.ERR_HEADER, True)
    assert crm.range_status(stream, moved, outp, (0, 18, 0), total, ok) == (0, False)   # chunk 2 is not in the span
    # the lowest failing chunk of the table stage wins; a decode failure comes after every table check
    moved[1] = (len(stream), 1)
    assert crm.range_status(stream, moved, outp, whole, total, ok) == (crm.ERR_TRUNCATED, True)
    bad3 = lambda payload: crm.ERR_OFFSET if len(payload) == comp[3][1] else 0  # noqa: E731
    assert crm.range_status(stream, comp, outp, whole, total, bad3) == (crm.ERR_OFFSET, False)
    assert crm.range_status(stream, comp, outp, (0, 82, 0), total, bad3) == (0, False)
    assert crm.range_status(stream, comp, outp, (total, 1, 0), total + 1, ok) == (crm.ERR_ARG, True)


def test_staging_inputs_reach_more_than_one_group():
    budget = 3 * 65536
    stream, raw = rc.uniform(cm.XERIAL, 8, 4096, 80)
    comp, outp, total = crm.tables(stream, cm.XERIAL)
    ranges, out_bytes = rc.lay_out(rc.staging_spans(total, 40, 3))
    _, units = crm.plan(outp, ranges, out_bytes)
    places, gstart, stage = crm.pack(outp, units, budget)
    assert sum(1 for e in units if e[5]) >= 67 and any(e[5] == 0 and e[4] for e in units)
    assert len(gstart) == 2 and stage == budget                 # 48 chunks of 4,096 fill it exactly
    # a chunk above the budget between short ones: a group of its own
    stream = rc.container(cm.HADOOP, [cc.stored(bytes(n)) for n in (100, 262144, 100)], [100, 262144, 100])
    comp, outp, total = crm.tables(stream, cm.HADOOP)
    ranges, out_bytes = rc.lay_out([(1, 99), (50, 200), (150, 262344 - 50), (262244, 262343)])
    _, units = crm.plan(outp, ranges, out_bytes)
    places, gstart, stage = crm.pack(outp, units, budget)
    assert stage == 262144 and len(gstart) >= 3
    big = [p for p, e in enumerate(units) if e[0] == 1 and e[5]]
    assert all(p in gstart and places[units[p][5]] == 0 for p in big)

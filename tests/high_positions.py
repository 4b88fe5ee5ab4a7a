"""Layouts of tests/test_high_positions.py (no GPU, no torch of their own): the
small planted inputs of the range, record and CRC suites, moved by a constant so
that every position a call is given -- stream positions, the window origin, table
entries, decoded starts, record offsets, output offsets -- lies around 2^32.

The addressing model: positions are offsets into two arenas of ARENA = 2^33 + E
bytes, `src` (filled with 0x5A) and `dst` (0xA5).  `src`'s base is handed to a
call as position 0, `dst` whole as its output, and every object a call touches
lies in [2^32 - E, 2^32 + E) of its arena.  A kernel that drops bit 32 of a
position lands 4 GiB lower, one that wraps a small negative difference in 32 bits
lands 4 GiB higher: both inside the arena, so a wrong kernel shows as wrong bytes
or a disturbed sentinel and not as an unmapped address.  For the same reason no
position here exceeds 2^33; larger ones go to the CPU plan checks (plan cases
below), which run no kernel.

Every builder returns a namespace with the small (unshifted) input beside the
shifted one: the expected bytes are the small input's, by the oracle and the
models of the suites the inputs come from."""
import collections
import functools
import types

import numpy as np

import container_model as cm
import container_ranges_cases as crc_
import container_ranges_model as crm
import datagen
import frame_model as fm
import frame_ranges_cases as fc
import frame_ranges_model as frm
import oracle
import ranges_planted as rp
import record_layouts as rl
import test_container_ranges as tcr
import test_frame as tf
import test_k1r_k2_record_forms as kf
import test_k4_decode as k4
import test_k4_record_forms as rf

P32 = 1 << 32
E = 1 << 25                     # 32 MiB on either side of 2^32
ARENA = 2 * P32 + E
LO, HI = P32 - E, P32 + E
SRC_FILL, DST_FILL = 0x5A, 0xA5
PIECE = 1 << 28                 # the arenas are compared in pieces of 256 MiB
U64 = (1 << 64) - 1
BLOCK = 65536
MASK = rp.MASK
OK, TRUNC, DEP, CHECKSUM, INDEX = 0, -3, -13, -12, -11
SINGLE, STREAMS = 0, 1
STREAMS_FAMILY = "lanes"
PLAN_SHIFTS = [(1 << 40) - (1 << 16), 1 << 62]   # CPU plan checks only


def ns(**k):
    return types.SimpleNamespace(**k)


def centre(total, items, mult=1, res=0, least=2):
    """The shift, = res mod mult, that puts the middle of the item nearest the middle
    of [0, total) at 2^32.  items: [(offset, length)]."""
    a, ln = min((it for it in items if it[1] >= max(least, 2 * mult + 2)),
                key=lambda it: abs(it[0] + it[1] // 2 - total // 2))
    s = P32 - (a + ln // 2)
    s -= (s - res) % mult
    assert a + s < P32 < a + s + ln
    return s


def sides(items):
    """(below, straddling, above) 2^32 of [(position, length)], empty items left out"""
    c = collections.Counter()
    for a, ln in items:
        if ln:
            c["below" if a + ln <= P32 else "above" if a >= P32 else "straddling"] += 1
    return c["below"], c["straddling"], c["above"]


def inside(items):
    return all(LO <= a and a + ln <= HI for a, ln in items)


def move(ranges, d, o):
    return [(a + d, ln, oo + o) for a, ln, oo in ranges]


def translated(units, du, o):
    return [(u + du, (land + o) & U64, i, lo, hi, edge) for u, land, i, lo, hi, edge in units]


def unit_sides(units):
    """{(edge | interior, side of the unit's wanted bytes in dst): count} of plan units"""
    c = collections.Counter()
    for u, land, i, lo, hi, edge in units:
        if hi in (0, frm.BAD):
            continue
        a, b = land + lo, land + hi
        c["edge" if edge else "interior", "below" if b <= P32 else "above" if a >= P32 else "straddling"] += 1
    return dict(sorted(c.items()))


# ---------------------------------------------------------------------------
# A: raw range decode
# ---------------------------------------------------------------------------
def _single_rows(m, n, dep):
    """test_single_independent_blocks' rows: every independent block whole and as
    [b0 + 1, b0 + size - 1), a range inside every dependent block, ranges over two and
    three consecutive blocks -> Packer, the model's statuses"""
    def size(u):
        return min(BLOCK, n - u * BLOCK)
    p, model = rp.Packer(), []
    for u in range(m):
        b0 = u * BLOCK
        if u in dep:
            p.add(b0 + 10 + 97 * u % 5000, 1000, u % 16)
            model.append(DEP)
        else:
            p.add(b0, size(u), u % 16)
            p.add(b0 + 1, size(u) - 2, (u + 7) % 16)
            model += [OK, OK]
    for u in range(m - 1):
        for k in (2, 3):
            if u + k > m:
                continue
            deps = [b in dep for b in range(u, u + k)]
            if any(deps) and (k == 3 or all(deps)):
                continue
            a = u * BLOCK + 1 + 37 * u % 60000
            b = (u + k - 1) * BLOCK + 1 + 53 * u % (size(u + k - 1) - 1)
            p.add(a, b - a, (3 * u + k) % 16)
            model.append(DEP if any(deps) else OK)
    return p, model


def _streams_rows(m, chunk):
    """test_streams_planted_interior's and _staged's rows: runs of 1..3 whole units,
    every unit as an edge unit, ranges from inside unit u to inside u + 2; in a seeded
    order, so that both kinds land on both sides of dst's 2^32"""
    rng = np.random.default_rng(870 + chunk)
    rows, u, i = [], 0, 0
    while u < m:
        run = min(1 + i % 3, m - u)
        rows.append((u * chunk, run * chunk, (i + 5) % 16))
        u, i = u + run, i + 1
    for u in range(m):
        if u % 3 == 0:
            lo, hi = 1, chunk
        elif u % 3 == 1:
            lo, hi = 0, chunk - 1
        else:
            lo = int(rng.integers(1, chunk - 1))
            hi = int(rng.integers(lo + 1, chunk + 1))
        rows.append((u * chunk + lo, hi - lo, (7 * u + 3) % 16))
    for u in range(0, m - 2, 3):
        lo, hi = int(rng.integers(1, chunk)), int(rng.integers(1, chunk))
        rows.append((u * chunk + lo, 2 * chunk - lo + hi, (u + 11) % 16))
    rows.append(((m // 2 - 1) * chunk + 7, 2 * chunk - 20, 6))   # two edge units around unit m // 2's first byte
    p = rp.Packer()
    for k in rng.permutation(len(rows)):
        p.add(*rows[int(k)])
    return p, [OK] * len(p.ranges)


@functools.lru_cache(maxsize=None)
def raw_case(layout, chunk=BLOCK):
    """A small stream of m units as units [K, K + m) of a stream of n bytes whose
    earlier units are not resident and not described: their index entries are filler
    (the first real position).  kr0_range_check and k4_body's RANGE form read entries
    u and u + 1 of planned units only; the GPU test relies on that."""
    if layout == SINGLE:
        stream, index, n_small, _, _ = rp.single_independent_input()
        want, dep = rp.single_independent_want(), set(rp.single_independent_dependent())
        buf, e, unit = stream.tobytes(), [int(x) for x in index], BLOCK
        elements = rp.walk(buf)[1]
        pre = elements[0][0]
        assert e[0] == 0 and 1 <= pre <= 5
        # no planted copy reaches before the stream's first byte: block 0 as unit K != 0
        # (no preamble to parse, back_lim no longer 0) keeps its status
        assert all(pos - off >= 0 for _, pos, t, _, _, off in elements if t != 0)
        m = len(e) - 1
        j = next(j for j in range(m // 2, m - 1) if not {j - 1, j, j + 1} & dep)
    else:
        payload, offs, m, _ = k4.streams_input(STREAMS_FAMILY, chunk)
        want, dep = k4.streams_want(STREAMS_FAMILY, chunk), set()
        buf, e, unit, pre, n_small = payload.tobytes(), [int(x) for x in offs], chunk, 0, m * chunk
        j = m // 2
    K = P32 // unit - j
    assert K * unit < P32 < (K + m) * unit and (K + j) * unit <= P32 < (K + j + 1) * unit
    n = K * unit + n_small
    c0, c1 = rp.block_span(buf, e, j) if layout == SINGLE else (e[j], e[j + 1])
    C = P32 - (c0 + (c1 - c0) // 2)                  # unit K + j's payload straddles 2^32 in src
    assert c0 + C < P32 < c1 + C
    real = [((x & MASK) + C) | (x >> 40 << 40) for x in e]
    if layout == SINGLE:
        real[0] = pre + C                            # behind the preamble: u != 0 parses none
    full = np.full(K + m + 1, real[0], dtype=np.int64)
    full[K:] = real
    p, model = _single_rows(m, n_small, dep) if layout == SINGLE else _streams_rows(m, chunk)
    whole = [(oo, ln) for (a, ln, oo) in p.ranges if a % unit == 0 and ln % unit == 0 and ln]
    O = centre(p.total, whole, 16)
    ranges = move(p.ranges, K * unit, O)
    # the window negatives: a range in the first unit, one in unit j, one in the last unit
    last = (m - 1) * unit
    neg = rp.Packer()
    neg.add(1, unit - 2, 3)
    neg.add(j * unit, unit, 9)
    neg.add(last + 1, n_small - last - 2, 14)
    Oneg = centre(neg.total, [(neg.ranges[1][2], unit)], 16)
    spans = [rp.block_span(buf, e, u) if layout == SINGLE else (e[u], e[u + 1]) for u in range(m)]
    units_comp = [(a + C, b - a) for a, b in spans]
    return ns(layout=layout, unit=unit, m=m, K=K, j=j, n_small=n_small, n=n, C=C, O=O, small=buf, want=want,
              small_index=np.array(e, dtype=np.int64), index=full, w0=pre + C, w1=len(buf) + C, pre=pre,
              small_ranges=p.ranges, small_total=p.total, ranges=ranges, model=model, dep=dep,
              neg_small=neg.ranges, neg_total=neg.total, neg=move(neg.ranges, K * unit, Oneg), Oneg=Oneg,
              neg_short=[OK, OK, TRUNC], neg_late=[TRUNC, OK, OK], units_comp=units_comp)


def raw_writes(c, ranges_small, model, o):
    """dst's expected writes: (offset, bytes) of a range the model calls OK, (offset,
    length) of one that fails while it decodes (its own range is not compared)"""
    w = []
    for (a, ln, oo), st in zip(ranges_small, model):
        if st == OK:
            w.append((oo + o, c.want[a:a + ln]))
        elif st not in rp.EARLY:
            w.append((oo + o, ln))
    return w


# ---------------------------------------------------------------------------
# B: framed range decode
# ---------------------------------------------------------------------------
FRAME_CASES = [("three runs", "header"), ("three runs", "payload"), ("compressed and stored mixed", "payload"),
               ("compressed and stored mixed", "header"), ("stored chunks at the literal-tag edges", "header"),
               ("stored chunks at the literal-tag edges", "payload")]


@functools.lru_cache(maxsize=None)
def _decompress_status(body):
    return 0, oracle.decompress(body)


def frame_statuses(stream, chunks, starts, ranges, out_bytes, w0, w1):
    """frame_ranges_model.range_status of every range -> [(status, early)], each chunk's
    decode and CRC verdict (chunk_decode_status, the model's CRC in Python) taken once"""
    verdict = functools.lru_cache(maxsize=None)(
        lambda u: frm.chunk_decode_status(stream, chunks[u], _decompress_status)[0])
    out = []
    for r in ranges:
        st, u0, u1, k = frm.span(starts, r, out_bytes)
        if st != OK:
            out.append((st, True))
            continue
        us = [e for e in (frm.unit(starts, r, 0, u0, u1, u)[0] for u in range(u0, u0 + k)) if e[4] != 0]
        st = next((s for s in (frm.unit_check(stream, chunks, starts, e[0], e[4], w0, w1) for e in us) if s != OK), OK)
        if st != OK:
            out.append((st, True))
            continue
        out.append((next((s for s in (verdict(e[0]) for e in us) if s != OK), OK), False))
    return out


@functools.lru_cache(maxsize=None)
def _frame_base(name):
    stream, raw = tf.FOREIGN[name]()
    chunks, starts = fc.tables(stream)
    nch = len(chunks) - 1
    spans = [(chunks[u], chunks[u + 1] - chunks[u]) for u in range(nch)]
    a, ln = min((s for s in spans if s[1] >= 48), key=lambda s: abs(s[0] + s[1] // 2 - len(stream) // 2))
    ranges, out_bytes = fc.lay_out(fc.slice_spans(starts))
    w0, w1 = chunks[0], len(stream)
    # (the first rows by the model's own range_status: frame_statuses is the same rule)
    ok = frame_statuses(stream, chunks, starts, ranges, out_bytes, w0, w1)
    assert ok[:8] == [frm.range_status(stream, chunks, starts, r, out_bytes, _decompress_status, w0, w1)
                      for r in ranges[:8]]
    assert all(s == (OK, False) for s in ok)
    # negative 1: the stored CRC of the chunk that straddles 2^32, one bit flipped
    flipped = bytearray(stream)
    flipped[a + 5] ^= 0x10
    flipped = bytes(flipped)
    crc = frame_statuses(flipped, chunks, starts, ranges, out_bytes, w0, w1)
    assert {s for s, _ in crc} == {OK, CHECKSUM} and all(not early for s, early in crc if s)
    # negative 2: the window one byte short
    short = frame_statuses(stream, chunks, starts, ranges, out_bytes, w0, w1 - 1)
    assert {s for s, _ in short} == {OK, TRUNC} and all(early for s, early in short if s)
    return stream, raw, chunks, starts, spans, a, ranges, out_bytes, flipped, crc, short


@functools.lru_cache(maxsize=None)
def frame_case(name, straddle):
    stream, raw, chunks, starts, spans, a, ranges, out_bytes, flipped, crc, short = _frame_base(name)
    nch = len(chunks) - 1
    j = chunks.index(a)
    paylen = (stream[a + 1] | stream[a + 2] << 8 | stream[a + 3] << 16) - 4
    # the chunk's 8 header bytes around 2^32 (3 below: its length field is cut), or its payload
    C = P32 - a - 3 if straddle == "header" else P32 - (a + 8 + paylen // 2)
    jd = max(range(nch), key=lambda u: starts[u + 1] - starts[u])
    D = P32 - (starts[jd] + (starts[jd + 1] - starts[jd]) // 3)
    assert starts[0] + D < P32 < starts[nch] + D
    O = centre(out_bytes, [(oo, ln) for _, ln, oo in ranges], 16)
    return ns(name=name, straddle=straddle, stream=stream, flipped=flipped, raw=raw, chunks=chunks, starts=starts, j=j,
              C=C, D=D, O=O, w0=chunks[0], w1=len(stream), small_ranges=ranges, small_total=out_bytes,
              ranges=move(ranges, D, O), hchunks=[x + C for x in chunks], hstarts=[x + D for x in starts],
              crc=[s for s, _ in crc], short=[s for s, _ in short],
              units_comp=[(x + C, ln) for x, ln in spans], header_at=a + C, payload=(a + 8 + C, paylen))


def slice_writes(raw, ranges_small, statuses, o, partial=()):
    """dst's expected writes of a framed or container call: the slices of the ranges
    with status 0; a range that fails while it decodes (`partial`) is not compared"""
    w = []
    for (a, ln, oo), st in zip(ranges_small, statuses):
        if st == OK:
            w.append((oo + o, np.frombuffer(raw[a:a + ln], dtype=np.uint8)))
        elif st in partial:
            w.append((oo + o, ln))
    return w


# ---------------------------------------------------------------------------
# C: container range decode
# ---------------------------------------------------------------------------
CONTAINER_SLICES = {cm.HADOOP: "hadoop: chunks of copies, an empty block between",
                    cm.XERIAL: "xerial: chunks of copies"}
CONTAINER_CASES = [(fmt, which) for fmt in (cm.HADOOP, cm.XERIAL) for which in ("long", "slice")]


@functools.lru_cache(maxsize=None)
def container_case(fmt, which):
    if which == "long":
        stream, raw, comp, outp = tcr.long_case(fmt)
        ranges, out_bytes = crc_.lay_out(crc_.long_spans(outp))
    else:
        f, stream, raw, comp, outp, ranges, out_bytes = crc_.slice_case(CONTAINER_SLICES[fmt])
        assert f == fmt
    w0, w1 = comp[0][0], comp[-1][0] + comp[-1][1]
    C = centre(len(stream), comp[1:-1] if len(comp) >= 3 else comp)   # a payload between others across 2^32
    j = next(u for u, (a, ln) in enumerate(comp) if a + C < P32 < a + C + ln)
    total = outp[-1][0] + outp[-1][1]
    D = P32 - (outp[j][0] + max(outp[j][1] // 3, 1))
    assert outp[0][0] + D < P32 < total + D
    O = centre(out_bytes, [(oo, ln) for _, ln, oo in ranges], 16, least=40)
    decode_ok = lambda payload: OK  # noqa: E731  (these payloads are sound)
    ok = [crm.range_status(stream, comp, outp, r, out_bytes, decode_ok, w0, w1) for r in ranges]
    assert all(s == (OK, False) for s in ok)
    c = ns(fmt=fmt, which=which, stream=stream, raw=raw, comp=comp, outp=outp, j=j, C=C, D=D, O=O, w0=w0, w1=w1,
           small_ranges=ranges, small_total=out_bytes, ranges=move(ranges, D, O),
           hcomp=[(a + C, ln) for a, ln in comp], houtp=[(a + D, ln) for a, ln in outp])
    if which == "long":
        short = [crm.range_status(stream, comp, outp, r, out_bytes, decode_ok, w0, w1 - 1) for r in ranges]
        assert {s for s, _ in short} == {OK, TRUNC} and all(early for s, early in short if s)
        # a table entry's length raised by 1: the chunk no longer ends where the next begins
        raised = list(outp)
        raised[j] = (outp[j][0], outp[j][1] + 1)
        bad = [crm.range_status(stream, comp, raised, r, out_bytes, decode_ok, w0, w1) for r in ranges]
        assert INDEX in {s for s, _ in bad} and OK in {s for s, _ in bad} and all(early for s, early in bad if s)
        c.short, c.raised, c.bad = [s for s, _ in short], raised, [s for s, _ in bad]
        c.hraised = [(a + D, ln) for a, ln in raised]
    return c


# ---------------------------------------------------------------------------
# D: record batches
# ---------------------------------------------------------------------------
HOSTILE = ["copy-1 offset 0", "copy-2 offset 0", "copy-4 offset 0", "literal 2^32 first", "control",
           "literal 2^24 after"]


@functools.lru_cache(maxsize=None)
def records_case(family="span", chunk=8191):
    """One pass1_layout family's records with a few hostile units between them.
    -> items [(stream, oracle's bytes or None, status: 0, a code, or None = the unshifted call's)]"""
    items = [(s, w.tobytes(), OK) for s, w in rf.unit_records(family, chunk)]
    bodies = k4.hostile_bodies()
    for k, name in enumerate(HOSTILE):
        body, code, _, _ = bodies[name]
        unit = k4.varint(k4.HCHUNK) + body
        got = k4.oracle_accepts(unit, k4.HCHUNK)
        assert (got is None) == (name != "control")
        items.insert(3 + 5 * k, (unit, got, OK if got is not None else code))
    blob, c_descs = rl.pack([[s] for s, _, _ in items], ["kr4"] * len(items), 3100, 1)
    lens = [len(w) if w is not None else k4.HCHUNK for _, w, _ in items]
    o_descs, size = rl.scatter(lens, ["rec"] * len(items), 3101)
    B = centre(len(blob), c_descs, 4, 1)              # (alignments as in the small buffer, 1 byte into a dword)
    O = centre(size, o_descs, 16)
    return ns(items=items, blob=blob, shift=1, c_descs=c_descs, o_descs=o_descs, size=size, lens=lens, B=B, O=O,
              hc=[(a + B, ln) for a, ln in c_descs], ho=[(a + O, ln) for a, ln in o_descs])


@functools.lru_cache(maxsize=None)
def compress_records_case(family="k2"):
    recs, blob, shift, descs = kf.e_batch(family)
    B = centre(len(blob), descs, 4, shift)
    hd = [(a + B, ln) for a, ln in descs]
    for side in (lambda a, ln: a + ln <= P32, lambda a, ln: a >= P32):
        assert {kf.cls(r[1]) for r, (a, ln) in zip(recs, hd) if side(a, ln)} == {"k1r", "k1r64"}
    return ns(records=[r[1] for r in recs], blob=blob, shift=shift, descs=descs, B=B, hd=hd)


# ---------------------------------------------------------------------------
# E: long records
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def long_case():
    """short, the SINGLE stream of test_k4_decode as one long record, empty, short"""
    stream, index, n, _, _ = k4.single_input()
    shorts = rf.unit_records("span", 8191)[:2]
    items = [(shorts[0][0], shorts[0][1].tobytes(), [0, len(shorts[0][0])]),
             (stream.tobytes(), k4.single_want().tobytes(), index.tolist()),
             (b"\x00", b"", [0]),
             (shorts[1][0], shorts[1][1].tobytes(), [0, len(shorts[1][0])])]
    classes = ["short", "long", "empty", "short"]
    # (the first seed that leaves a short record on either side of the long one in memory: k4_long_unit and
    # kr5_index_lrecords then see a record offset with bit 32 clear and one with it set)
    for seed in range(3200, 3300):
        blob, c_descs = rl.pack([[it[0]] for it in items], classes, seed, 2)
        B = centre(len(blob), c_descs, 4, 2)
        below, across, above = sides([(a + B, ln) for (a, ln), cls in zip(c_descs, classes) if cls != "empty"])
        if below and above:
            break
    o_descs, size = rl.scatter([len(it[1]) for it in items], classes, 3201)
    O = centre(size, o_descs, 16)
    assert c_descs[1][0] + B < P32 < c_descs[1][0] + B + c_descs[1][1]
    assert o_descs[1][0] + O < P32 < o_descs[1][0] + O + o_descs[1][1]
    return ns(items=items, blob=blob, c_descs=c_descs, o_descs=o_descs, size=size, B=B, O=O,
              tables=[e for it in items for e in it[2]],
              hc=[(a + B, ln) for a, ln in c_descs], ho=[(a + O, ln) for a, ln in o_descs])


LONG_SOURCE = 3 * BLOCK + 61001


@functools.lru_cache(maxsize=None)
def compress_long_case():
    """A record of 65,537 bytes below 2^32, one of LONG_SOURCE bytes whose second block
    holds src's 2^32, one of 100 bytes above"""
    a = datagen.make("T", 65537 + LONG_SOURCE + 100, 3300).tobytes()
    recs = [a[:65537], a[65537:65537 + LONG_SOURCE], a[65537 + LONG_SOURCE:]]
    at = P32 - 100001
    descs = [(at - 65537 - 7, 65537), (at, LONG_SOURCE), (at + LONG_SOURCE + 5, 100)]
    assert BLOCK < P32 - at < 2 * BLOCK
    return ns(records=recs, descs=descs)


# ---------------------------------------------------------------------------
# F: CRC-32C
# ---------------------------------------------------------------------------
CRC_LENGTHS = [3, 4, 257, 4097, 65536]


@functools.lru_cache(maxsize=None)
def crc_case():
    """Entries of every length ending 0..3 bytes past 2^32 (k = 0 abuts it from below)
    and starting 0..3 bytes past it, and one cut in its middle, over random bytes"""
    r0 = P32 - BLOCK - 64
    data = datagen.make("R", 2 * BLOCK + 128, 3400).tobytes()
    ents = []
    for ln in CRC_LENGTHS:
        ents += [(P32 - ln + k, ln) for k in range(4)] + [(P32 + k, ln) for k in range(4)] + [(P32 - ln // 2, ln)]
    want = [fm.crc32c(data[a - r0:a - r0 + ln]) for a, ln in ents]
    return ns(at=r0, data=data, entries=ents, want=want)


# ---------------------------------------------------------------------------
# the plan cases of the three CPU plan checks: the arena's shifts and two no GPU test uses
# ---------------------------------------------------------------------------
def raw_plan_cases():
    """[(n, out_bytes, unit, ranges)] for tests/test_ranges_plan_check.py"""
    out = []
    for layout, chunk in ((SINGLE, BLOCK), (STREAMS, 8191), (STREAMS, BLOCK)):
        c = raw_case(layout, chunk)
        out.append((c.n, ARENA, c.unit, c.ranges))
        for s in PLAN_SHIFTS:
            k = s // c.unit
            out.append((k * c.unit + c.n_small, s + c.small_total + 16, c.unit, move(c.small_ranges, k * c.unit, s)))
    return out


def frame_plan_cases():
    """[(out_bytes, starts, ranges)] for tests/test_frame_ranges_plan_check.py"""
    out = []
    for name in sorted({n for n, _ in FRAME_CASES}):
        c = frame_case(name, "payload")
        out.append((ARENA, c.hstarts, c.ranges))
        for s in PLAN_SHIFTS:
            out.append((s + c.small_total + 16, [x + s + 1 for x in c.starts], move(c.small_ranges, s + 1, s)))
    return out


def container_plan_cases():
    """[(out_bytes, outp, ranges)] for tests/test_container_ranges_plan_check.py"""
    out = []
    for fmt, which in CONTAINER_CASES:
        c = container_case(fmt, which)
        out.append((ARENA, c.houtp, c.ranges))
        if which == "long":
            out.append((ARENA, c.hraised, c.ranges))
            for s in PLAN_SHIFTS:
                out.append((s + c.small_total + 16, [(a + s + 1, ln) for a, ln in c.outp],
                            move(c.small_ranges, s + 1, s)))
    return out


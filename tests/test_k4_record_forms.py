"""k4_body's other instantiations on the planted inputs of test_k4_decode.py:
kr4_decode_records (REC), kr4_decode_lunits / kr4_back_lunits (LONG) with
kr5_index_lrecords, and kr4_decode_frame_units (REC inside the framed range
decode) next to the framed whole decode.  The inputs, the element model and the
proof of what the inputs reach are test_k4_decode's; this module only lays the
same bytes out as records, long records and framing chunks (record_layouts.py)
and compares whole sentinel-filled output buffers bit for bit.

A. test_records_planted: every STREAMS unit of a family (preamble included) is one
   record of one decompress_records_device call; the expected bytes are
   streams_want's.  One family per chunk is decoded again with d_status NULL.
B. test_hostile_records: every unit of hostile_bodies() and streams_only_bodies()
   stands between two good records in memory and in the batch.  The record behind
   a unit whose last element is cut short begins with the byte that would complete
   it (a preamble of 100 or 228, or the empty record 00), so a decoder bounded by
   the batch's end instead of the record's would accept the unit.  A status is 0
   exactly when the oracle accepts the unit; otherwise it is what a one-unit
   STREAMS decode of the same bytes reports.
C. test_long_*: single_input() as a long record -- alone with its host-built table
   at four (source alignment, output residue) pairs, without a table (the device
   walk must return the host-built entries), twice in one batch with the 8,191-byte
   span and lanes units and two empty records (two records in pass 2 at once, each
   on its own ticket counter, short records' one-unit slices next to them), and
   that batch with the second copy's table damaged three ways.
D. test_frame_*: planted units wrapped as type-00 chunks behind the identifier
   (all of span and lanes, the 24-unit picks of test_streams_planted_alignment of
   the other families, long's sweeps, both chunk sizes; a padding chunk where it is
   needed to cycle the payload's alignment).  Decoded whole, as one range at out_offset
   0..15 (every unit interior), and as ranges that begin and end 1 byte and
   chunk - 1 bytes inside each run's first and last chunk (staged edge units).  The
   chunk table and the seek table are the model's; the device walk and
   frame_seek_tensor must return them.

test_layouts_have_their_properties (no GPU) asserts what the layouts claim and
runs k4_model over the frame subset in its record form (c_end the payload's end,
the payload at its address in the frame).  Measured there:
* A: 1,215 records per chunk (overlap 278, ring 124, long 750, span 30, lanes 33),
  every source alignment and every destination residue in each of the ten batches,
  buffer bases at all four residues.
  test_records_reach_the_edges_at_their_own_alignments runs k4_model over every
  record where it lies and lands (chunk 8192 / 8191): batches starting at o = 255 |
  256: 26 | 35 and 36 | 27, at 511 | 512: 5 | 7 and 9 | 8; hpos 440 | 441: 19 | 21 and
  30 | 35; e_lsrc + e_len 508 | 509: 66 | 67 and 74 | 61; batch output 1023 / 1024 /
  1025: 22 / 75 / 19 and 22 / 72 / 19; first source byte at lo - 1 / lo / lo + 1: 570 /
  568 / 487 and 570 / 569 / 484; all 9,520 overlap triples at their phases; ring
  flushes at each of the 16 destination residues 312-328 and 316-329 times (the
  STREAMS suites see dst & 15 = 0 only at chunk 8192).
* B: 45 hostile units, 135 records, 41 of the units refused by the oracle; 6 units
  end in a cut element and are followed by a completing record (oracle: the unit
  alone refused, with that byte accepted).
* C: the SINGLE stream is 5,761,995 bytes in 88 blocks; the batch holds 67 records
  (2 long, 63 short, 2 empty) and 241 units.
* D: 708 chunks (span 30, lanes 33, 24 each of overlap and ring, 243 of long, at
  both chunk sizes), 5,799,582 bytes.  With long's 24-unit pick alone the subset
  had 1 | 12 batches starting at o = 255 | 256 and none at 511 | 512, so long's
  sweeps (its last 219 units) are framed too.  Then: batches starting at o = 255 |
  256: 21 | 20, at 511 | 512: 17 | 12; hpos 440 | 441: 25 | 11; e_lsrc + e_len 508 |
  509: 56 | 75; batch output 1023 / 1024 / 1025 at an element end: 20 / 136 / 24;
  first source byte at lo - 1 / lo / lo + 1: 562 / 564 / 482; all 16 k4_literal_hbm
  (dst & 3, src & 3) pairs; the 20 edge ranges stage 40 units, 1,376 go straight
  to the output.
"""
import collections
import functools

import numpy as np
import pytest

import frame_model as fm
import frame_ranges_model as frm
import oracle
import record_layouts as rl
import snappy_amd
import test_k4_decode as k4
from golden_inputs import varint
from test_long_records import decode_call as long_decode_call, index_call, walk_table
from test_records import streams_status

CHUNKS, FAMILIES, HCHUNK, BLOCK = k4.CHUNKS, k4.FAMILIES, k4.HCHUNK, k4.BLOCK
NULL_STATUS = {8192: "long", 8191: "ring"}  # decoded a second time with d_status NULL
SINGLE_PAIRS = [(0, 0), (1, 5), (2, 10), (3, 15)]  # (s_in, s_out)
DAMAGE = ["last", "moved", "beyond"]


def unit_records(family: str, chunk: int, pick=None):
    """[(a unit's stream, its decoded bytes)] of a STREAMS input (of the units in pick)."""
    payload, offs, units, _ = k4.streams_input(family, chunk)
    want = k4.streams_want(family, chunk)
    p = payload.tobytes()
    return [(p[int(offs[u]):int(offs[u + 1])], want[u * chunk:(u + 1) * chunk])
            for u in (range(units) if pick is None else pick)]


# ---- A ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def pass1_layout(family: str, chunk: int):
    recs = unit_records(family, chunk)
    seed = 1100 + 10 * FAMILIES.index(family) + chunk % 2
    shift = (FAMILIES.index(family) + chunk) % 4
    blob, c_descs = rl.pack([[s] for s, _ in recs], ["kr4"] * len(recs), seed, shift)
    o_descs, size = rl.scatter([chunk] * len(recs), [family] * len(recs), seed + 1)
    return blob, shift, c_descs, o_descs, size, [w for _, w in recs]


@pytest.mark.gpu
@pytest.mark.parametrize("chunk", CHUNKS)
@pytest.mark.parametrize("family", FAMILIES)
def test_records_planted(codec, family, chunk):
    """A: kr4_decode_records, one record per planted unit, one call per family."""
    blob, shift, c_descs, o_descs, size, wants = pass1_layout(family, chunk)
    comp = rl.to_device(blob, shift)
    img, care = rl.image(size, o_descs, wants)
    for with_status in (True, False) if NULL_STATUS[chunk] == family else (True,):
        out = rl.sentinel_buffer(size)
        rc, status = rl.decode_records_call(codec, comp, c_descs, out, o_descs, with_status)
        assert rc == snappy_amd.OK
        assert (status == (0 if with_status else 77)).all(), np.flatnonzero(status)[:8]
        rl.assert_image(out.cpu().numpy(), img, care, o_descs, (family, chunk, with_status))


# ---- B ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def hostile_batch():
    """-> cases [(name, code or None, good record, (unit, oracle's bytes or None), record behind it)]
    with records as (stream, decoded bytes), blob, shift, c_descs, o_descs, size."""
    bodies = {**k4.hostile_bodies(), **k4.streams_only_bodies()}
    tape = k4.Tape(1992, 2 << 20)
    rng = np.random.default_rng(1993)

    def good(n: int):
        if n == 0:
            return b"\x00", b""
        s = varint(n) + k4.encode(k4.filler(rng, n), tape)[0]
        return s, oracle.decompress(s)

    cases = []
    for name, (body, code, at, lane0) in bodies.items():
        unit = varint(HCHUNK) + body
        n_next = HCHUNK
        if "cut short" in name:
            # the first byte of the record behind it completes the element: a preamble of 228
            # (e4 01), of 100 (64), or the empty record (00)
            for b in (0xE4, 0x64, 0x00) if "width 4" in name else (0x64, 0x00, 0xE4):
                if k4.oracle_accepts(unit + bytes([b]), HCHUNK) is not None:
                    break
            else:
                raise AssertionError(name)
            n_next = {0xE4: 228, 0x64: 100, 0x00: 0}[b]
        cases.append((name, code, good(HCHUNK), (unit, k4.oracle_accepts(unit, HCHUNK)), good(n_next)))
    groups = [[before[0], unit, after[0]] for _, _, before, (unit, _), after in cases]
    blob, c_descs = rl.pack(groups, ["kr4"] * len(groups), 1994, 1)
    lens = [n for _, _, before, _, after in cases for n in (len(before[1]), HCHUNK, len(after[1]))]
    o_descs, size = rl.scatter(lens, ["hostile"] * len(lens), 1995)
    return cases, blob, 1, c_descs, o_descs, size


@pytest.mark.gpu
def test_hostile_records(codec):
    """B: hostile lengths, offsets and cut elements as records between good records."""
    cases, blob, shift, c_descs, o_descs, size = hostile_batch()
    expect, wants = [], []
    for name, code, before, (unit, want), after in cases:
        st = 0
        if want is None:
            st = streams_status(codec, unit, HCHUNK)
            assert st < 0, (name, st)
            if code is not None:
                assert st == code, (name, st)
        print(f"{name}: oracle {'accepts' if want is not None else 'refuses'}, one-unit STREAMS status {st}")
        expect += [0, st, 0]
        wants += [before[1], want, after[1]]
    comp = rl.to_device(blob, shift)
    img, care = rl.image(size, o_descs, wants)
    first = next(s for s in expect if s)
    for with_status in (True, False):
        out = rl.sentinel_buffer(size)
        rc, status = rl.decode_records_call(codec, comp, c_descs, out, o_descs, with_status)
        if with_status:
            bad = [(cases[i // 3][0], i % 3, int(status[i]), expect[i]) for i in range(len(expect))
                   if status[i] != expect[i]]
            assert not bad, bad[:6]
        assert rc == first
        rl.assert_image(out.cpu().numpy(), img, care, o_descs, ("hostile", with_status))


# ---- C ---------------------------------------------------------------------------
def single_alone(s_in: int, s_out: int):
    """The SINGLE stream as the only record -> blob, shift, c_descs, o_descs, size."""
    stream, index, n, _, _ = k4.single_input()
    shift = (3 * s_in + 1) % 4
    pad = (s_in - shift) % 4 + 4
    blob = bytes([rl.FILL]) * pad + stream.tobytes() + bytes([rl.FILL]) * 5
    return blob, shift, [(pad, stream.size)], [(16 + s_out, n)], 16 + s_out + n + 23


@pytest.mark.gpu
@pytest.mark.parametrize("s_in,s_out", SINGLE_PAIRS)
def test_long_single_with_its_table(codec, s_in, s_out):
    """C1: kr4_decode_lunits and kr4_back_lunits, 87 of 88 blocks through pass 2."""
    stream, index, n, _, _ = k4.single_input()
    blob, shift, c_descs, o_descs, size = single_alone(s_in, s_out)
    out = rl.sentinel_buffer(size)
    rc, status = long_decode_call(codec, rl.to_device(blob, shift), c_descs, out, o_descs, index=index.tolist())
    assert rc == snappy_amd.OK and status.tolist() == [0]
    img, care = rl.image(size, o_descs, [k4.single_want()])
    rl.assert_image(out.cpu().numpy(), img, care, o_descs, ("single", s_in, s_out))


@pytest.mark.gpu
def test_long_single_without_a_table(codec):
    """C2: kr5_index_lrecords walks the stream from an unaligned start."""
    stream, index, n, _, _ = k4.single_input()
    blob, shift, c_descs, o_descs, size = single_alone(3, 7)
    comp = rl.to_device(blob, shift)
    rc, table, status = index_call(codec, comp, c_descs, [n])
    assert rc == snappy_amd.OK and status.tolist() == [0]
    assert table[:index.size].tolist() == index.tolist() and (table[index.size:] == -7).all()
    assert table[index.size - 1] == stream.size
    out = rl.sentinel_buffer(size)
    rc, status = long_decode_call(codec, comp, c_descs, out, o_descs, index=None)
    assert rc == snappy_amd.OK and status.tolist() == [0]
    img, care = rl.image(size, o_descs, [k4.single_want()])
    rl.assert_image(out.cpu().numpy(), img, care, o_descs, "single without a table")


@functools.lru_cache(maxsize=None)
def long_batch():
    """empty, SINGLE, the span units, empty, the lanes units, SINGLE ->
    blob, shift, c_descs, o_descs, size, wants, tables, classes, positions of the two SINGLE records."""
    stream, index, n, _, _ = k4.single_input()
    single = (stream.tobytes(), k4.single_want(), index.tolist(), "long")
    empty = (b"\x00", b"", [0], "empty")
    short = {f: [(s, w, [0, len(s)], "short") for s, w in unit_records(f, 8191)] for f in ("span", "lanes")}
    items = [empty, single] + short["span"] + [empty] + short["lanes"] + [single]
    at = [i for i, it in enumerate(items) if it[3] == "long"]
    classes = [it[3] for it in items]
    blob, c_descs = rl.pack([[it[0]] for it in items], classes, 1996, 2)
    o_descs, size = rl.scatter([len(it[1]) for it in items], classes, 1997)
    return blob, 2, c_descs, o_descs, size, [it[1] for it in items], [it[2] for it in items], classes, at


@pytest.mark.gpu
@pytest.mark.parametrize("table", [True, False])
def test_long_batch_two_records_in_pass_2(codec, table):
    """C3: two records running pass 2 at the same time among one-unit records."""
    blob, shift, c_descs, o_descs, size, wants, tables, _, _ = long_batch()
    comp = rl.to_device(blob, shift)
    flat = [e for t in tables for e in t]
    if not table:
        rc, built, status = index_call(codec, comp, c_descs, [ln for _, ln in o_descs])
        assert rc == snappy_amd.OK and not status.any()
        assert built[:len(flat)].tolist() == flat and (built[len(flat):] == -7).all()
    out = rl.sentinel_buffer(size)
    rc, status = long_decode_call(codec, comp, c_descs, out, o_descs, index=flat if table else None)
    assert rc == snappy_amd.OK and not status.any()
    img, care = rl.image(size, o_descs, wants)
    rl.assert_image(out.cpu().numpy(), img, care, o_descs, ("long batch", table))


def damaged(tables, at, how: str):
    """The batch's tables with record `at`'s damaged as test_hostile_tables damages one."""
    t = list(tables[at])
    if how == "last":      # the last entry is not the compressed length
        t[-1] -= 1
    elif how == "moved":   # an entry one byte off its element's start
        t[1] += 1
    else:                  # an entry beyond the record's compressed range
        t[2] = t[-1] + 1
    return tables[:at] + [t] + tables[at + 1:]


@pytest.mark.gpu
@pytest.mark.parametrize("how", DAMAGE)
def test_long_batch_damaged_table(codec, how):
    """C4: the second SINGLE record's table damaged: ERR_INDEX for it alone.  With a
    wrong last entry no unit of it loads a byte, so its range keeps the sentinel;
    with the other two its remaining blocks decode (a partial write of its own
    range, which the contract allows) and its range is not compared."""
    blob, shift, c_descs, o_descs, size, wants, tables, _, at = long_batch()
    bad = at[1]
    flat = [e for t in damaged(tables, bad, how) for e in t]
    wants = list(wants)
    wants[bad] = np.full(len(wants[bad]), rl.SENT, dtype=np.uint8) if how == "last" else None
    out = rl.sentinel_buffer(size)
    rc, status = long_decode_call(codec, rl.to_device(blob, shift), c_descs, out, o_descs, index=flat)
    assert status.tolist() == [snappy_amd.ERR_INDEX if i == bad else 0 for i in range(len(wants))]
    assert rc == snappy_amd.ERR_INDEX
    img, care = rl.image(size, o_descs, wants)
    rl.assert_image(out.cpu().numpy(), img, care, o_descs, ("damaged table", how))


# ---- D ---------------------------------------------------------------------------
LONG_SWEEPS = 25 * 7 + 22 * 2  # long_cases()' last cases: the sweeps of e_lsrc + e_len and of the batch-start o


def frame_pick(family: str, units: int):
    """The units framed: all of span and lanes, test_streams_planted_alignment's picks
    of the others, and the sweeps of long: without them the subset has no batch
    starting at o = 511 | 512 and one at 255 (test_layouts_have_their_properties)."""
    if family in ("span", "lanes"):
        return list(range(units))
    pick = min(units, 24)
    if family != "long":
        return list(range(pick))
    first = (units - pick) // 2
    assert first + pick <= units - LONG_SWEEPS
    return list(range(first, first + pick)) + list(range(units - LONG_SWEEPS, units))


@functools.lru_cache(maxsize=None)
def frame_input():
    """-> the framed stream, its decoded bytes, the runs as (family, chunk, first
    chunk, chunks, decoded start), every chunk's decoded size."""
    stream, raw, runs, sizes = bytearray(fm.IDENTIFIER), bytearray(), [], []
    for chunk in CHUNKS:
        for family in FAMILIES:
            pick = frame_pick(family, k4.streams_input(family, chunk)[2])
            runs.append((family, chunk, len(sizes), len(pick), len(raw)))
            for s, w in unit_records(family, chunk, pick):
                k = len(sizes)
                if (len(stream) + 8) % 4 != k % 4:  # the payload's alignment cycles
                    stream += fm.padding((k - (len(stream) + 4 + 8)) % 4)
                assert (len(stream) + 8) % 4 == k % 4
                stream += fm.compressed(w.tobytes(), s)
                raw += w.tobytes()
                sizes.append(chunk)
    return bytes(stream), bytes(raw), runs, sizes


@functools.lru_cache(maxsize=None)
def frame_tables():
    """The model's chunk table and seek table."""
    stream, raw, runs, sizes = frame_input()
    st, chunks, total = fm.chunk_table(stream)
    assert st == fm.OK and total == len(raw) and len(chunks) == len(sizes) + 1
    starts = [0] + np.cumsum(sizes).tolist()
    return chunks, starts


def frame_edge_ranges():
    """Per run, a range 1 byte and one chunk - 1 bytes inside its first and last chunk
    -> ([(start, length, out_offset)], out_bytes)."""
    stream, raw, runs, sizes = frame_input()
    spans = []
    for family, chunk, c0, count, r0 in runs:
        ln = count * chunk
        spans += [(r0 + 1, ln - 2, chunk), (r0 + chunk - 1, ln - 2 * (chunk - 1), chunk)]
    o_descs, size = rl.scatter([ln for _, ln, _ in spans], [c for _, _, c in spans], 1998)
    return [(a, ln, o) for (a, ln, _), (o, _) in zip(spans, o_descs)], size


def i64(values):
    import torch
    return torch.tensor(list(values), dtype=torch.int64, device="cuda")


@pytest.mark.gpu
def test_frame_whole_decode_and_tables(codec):
    """D: the device walk and seek table are the model's; the whole decode at four
    (stream alignment, output residue) pairs."""
    stream, raw, runs, sizes = frame_input()
    chunks, starts = frame_tables()
    want = np.frombuffer(raw, dtype=np.uint8)
    for shift, s_out in SINGLE_PAIRS:
        frame = rl.to_device(stream, shift)
        n, table = codec.frame_index_tensor(frame)
        assert n == len(raw) and table.cpu().tolist() == chunks
        n2, seek = codec.frame_seek_tensor(frame, table.contiguous())
        assert n2 == len(raw) and seek.cpu().tolist() == starts
        size = 64 + s_out + len(raw) + 37
        buf = rl.sentinel_buffer(size)
        out = buf[64 + s_out:64 + s_out + len(raw)]
        got = codec.decompress_frame_tensor(frame, table, len(raw), out=out)
        assert got.data_ptr() == out.data_ptr() and got.numel() == len(raw)
        o_descs = [(64 + s_out, len(raw))]
        img, care = rl.image(size, o_descs, [want])
        rl.assert_image(buf.cpu().numpy(), img, care, o_descs, ("frame", shift, s_out))


def frame_ranges_check(codec, shift, ranges, out_bytes, what):
    stream, raw, runs, sizes = frame_input()
    chunks, starts = frame_tables()
    buf = rl.sentinel_buffer(out_bytes)
    _, st = codec.decompress_frame_ranges_tensor(rl.to_device(stream, shift), 0, i64(chunks), i64(starts), ranges,
                                                 out=buf)
    assert codec.last_ranges_status == snappy_amd.OK and not st.cpu().numpy().any(), what
    o_descs = [(o, ln) for _, ln, o in ranges]
    img, care = rl.image(out_bytes, o_descs, [np.frombuffer(raw[a:a + ln], dtype=np.uint8) for a, ln, _ in ranges])
    rl.assert_image(buf.cpu().numpy(), img, care, o_descs, what)


@pytest.mark.gpu
@pytest.mark.parametrize("quarter", range(4))
def test_frame_one_range_over_everything(codec, quarter):
    """D: kr4_decode_frame_units, every unit interior and decoded straight into the
    output, at out_offset 0..15 (four per case)."""
    n = len(frame_input()[1])
    for oo in range(4 * quarter, 4 * quarter + 4):
        frame_ranges_check(codec, (oo + quarter) % 4, [(0, n, oo)], oo + n + 1 + oo % 7, ("one range", oo))


@pytest.mark.gpu
def test_frame_edge_ranges(codec):
    """D: ranges beginning and ending inside each run's first and last chunk: those
    two units are staged, the ones between them go straight to the output."""
    ranges, out_bytes = frame_edge_ranges()
    frame_ranges_check(codec, 3, ranges, out_bytes, "edge ranges")


# ---- G: what the layouts claim (no GPU) ----------------------------------------------
def frame_stats(shift: int = 0):
    """k4_model over every chunk of the frame as the record kr4_decode_frame_units
    makes of it -> Stats merged over the subset."""
    stream, raw, runs, sizes = frame_input()
    chunks, starts = frame_tables()
    buf = bytes(shift) + stream
    S = k4.Stats()
    for u, pos in enumerate(chunks[:-1]):
        ln = stream[pos + 1] | stream[pos + 2] << 8 | stream[pos + 3] << 16
        c0 = shift + pos + 8
        assert k4.k4_model(buf, c0, c0 + ln - 4, c0 + ln - 4, sizes[u], 0, sizes[u], 0, 0, False,
                           starts[u] & 15, S) == "ok"
    return S


def test_records_reach_the_edges_at_their_own_alignments():
    """No GPU: the window positions depend on where a record lies (o counts from the
    aligned dword below its first byte) and the flushes on where its output lies, so
    k4_model runs over every record of A as kr4_decode_records sees it -- c_end its
    own end, its address in the shifted buffer, its output offset -- and
    test_k4_decode's conditions must hold for the five batches of a chunk merged,
    flushes at all 16 destination residues at either chunk."""
    for chunk in CHUNKS:
        per = []
        for family in FAMILIES:
            blob, shift, c_descs, o_descs, size, wants = pass1_layout(family, chunk)
            buf = bytes(shift) + blob
            S = k4.Stats()
            for (o, ln), (oo, _) in zip(c_descs, o_descs):
                c0 = shift + o
                assert k4.k4_model(buf, c0, c0 + ln, c0 + ln, chunk, 0, chunk, 0, 0, False, oo & 15, S) == "ok"
            per.append(S)
        k4.check_conditions(k4.merged(per), f"records / {chunk}", range(16))


def test_image_comparison_catches_a_changed_byte():
    """No GPU: the whole-buffer check itself."""
    o_descs = [(3, 5), (20, 0), (21, 4)]
    img, care = rl.image(30, o_descs, [b"abcde", b"", None])
    good = img.copy()
    good[22] ^= 1  # inside the range that is not compared
    rl.assert_image(good, img, care, o_descs, "control")
    for at in (0, 2, 3, 7, 8, 20, 25, 29):  # sentinels on every side of the ranges, a record's first and last byte
        bad = img.copy()
        bad[at] ^= 0x10
        with pytest.raises(AssertionError):
            rl.assert_image(bad, img, care, o_descs, at)


def check_layout(what, descs, classes, shift, o_descs, families, size, full=True):
    al = rl.source_alignments(descs, classes, shift)
    res = rl.dest_residues(o_descs, families)
    gaps = rl.gaps_of(o_descs, size)
    print(f"{what}: {len(descs)} records, base {shift} bytes into a dword, alignments "
          f"{ {k: sorted(v) for k, v in al.items()} }, residues { {k: len(v) for k, v in res.items()} }, "
          f"gaps {min(gaps)}..{max(gaps)}")
    assert rl.shuffled_against_addresses(descs) and rl.shuffled_against_addresses(o_descs), what
    assert min(gaps) >= 1 and max(gaps) <= 40, (what, min(gaps), max(gaps))
    if full:
        assert all(v == {0, 1, 2, 3} for v in al.values()), (what, al)
        assert all(len(v) == 16 for v in res.values()), (what, res)
    return al, res


def test_layouts_have_their_properties():
    """No GPU: alignment and residue coverage of every batch, B's completing
    neighbours, C's tables, and the edges the frame subset of D still reaches."""
    # A
    shifts, total = set(), collections.Counter()
    for chunk in CHUNKS:
        for family in FAMILIES:
            blob, shift, c_descs, o_descs, size, wants = pass1_layout(family, chunk)
            check_layout(f"A {family} {chunk}", c_descs, ["kr4"] * len(c_descs), shift, o_descs,
                         [family] * len(o_descs), size)
            shifts.add(shift)
            total[chunk] += len(c_descs)
            for (o, ln), (s, _) in zip(c_descs[:5], unit_records(family, chunk)):
                assert blob[o:o + ln] == s
    print("A: records per chunk", dict(total))
    assert shifts == {0, 1, 2, 3} and all(v == 1215 for v in total.values())
    # B
    cases, blob, shift, c_descs, o_descs, size = hostile_batch()
    check_layout("B", c_descs, ["kr4"] * len(c_descs), shift, o_descs, ["hostile"] * len(o_descs), size)
    cut = 0
    for i, (name, code, before, (unit, want), after) in enumerate(cases):
        o, ln = c_descs[3 * i + 1]
        assert blob[o:o + ln] == unit and c_descs[3 * i] == (o - len(before[0]), len(before[0]))
        assert c_descs[3 * i + 2] == (o + ln, len(after[0])), "the record behind it follows it directly"
        assert k4.oracle_accepts(before[0], len(before[1])) == before[1]
        assert after[0] == b"\x00" or k4.oracle_accepts(after[0], len(after[1])) == after[1]
        if "cut short" in name:
            cut += 1
            assert want is None, name
            assert k4.oracle_accepts(unit + blob[o + ln:o + ln + 1], HCHUNK) is not None, name
    refused = sum(1 for c in cases if c[3][1] is None)
    print(f"B: {len(cases)} hostile units, {len(c_descs)} records, {refused} refused by the oracle, "
          f"{cut} followed by a completing record")
    assert cut == 6 and refused >= 30 and len(cases) - refused >= 4
    # C
    stream, index, n, _, _ = k4.single_input()
    assert walk_table(stream.tobytes(), n) == index.tolist() and index[-1] == stream.size
    res = set()
    for s_in, s_out in SINGLE_PAIRS:
        blob, shift, c_descs, o_descs, size = single_alone(s_in, s_out)
        assert (shift + c_descs[0][0]) % 4 == s_in and blob[c_descs[0][0]:][:stream.size] == stream.tobytes()
        res.add(o_descs[0][0] & 15)
    assert res == {0, 5, 10, 15}
    blob, shift, c_descs, o_descs, size, wants, tables, classes, at = long_batch()
    al, rs = check_layout("C batch", c_descs, classes, shift, o_descs, classes, size, full=False)
    a, b = at
    assert (shift + c_descs[a][0]) % 4 != (shift + c_descs[b][0]) % 4 and o_descs[a][0] % 16 != o_descs[b][0] % 16
    assert al["short"] == {0, 1, 2, 3} and len(rs["short"]) == 16
    units = sum(max(1, (ln + BLOCK - 1) // BLOCK) for _, ln in o_descs)
    print(f"C: SINGLE {n} bytes in {index.size - 1} blocks; the batch holds {len(c_descs)} records "
          f"({dict(collections.Counter(classes))}), {units} units")
    assert collections.Counter(classes) == {"long": 2, "short": 63, "empty": 2}
    for t, (o, ln), (_, n_out) in zip(tables, c_descs, o_descs):
        assert t[-1] == (ln if n_out else 0) and len(t) == (n_out + BLOCK - 1) // BLOCK + 1
    for how in DAMAGE:
        assert damaged(tables, b, how)[b] != tables[b] and damaged(tables, b, how)[:b] == tables[:b]
    # D
    stream, raw, runs, sizes = frame_input()
    chunks, starts = frame_tables()
    assert fm.read(stream[:chunks[3]], oracle.decompress) == raw[:starts[3]]
    assert {(p + 8) % 4 for p in chunks[:-1]} == {0, 1, 2, 3}
    print(f"D: {len(sizes)} chunks, {len(raw)} bytes decoded, {len(stream)} framed;", {
        (f, c): k for f, c, _, k, _ in runs})
    S = frame_stats()
    both = {"o at a batch start 255 | 256": (S.o_pre, (255, 256)), "o at a batch start 511 | 512": (S.o_pre, (511, 512)),
            "hpos 440 | 441": (S.hpos, (440, 441)), "e_lsrc + e_len 508 | 509": (S.lsum, (508, 509)),
            "batch output 1023 / 1024 / 1025": (S.span_end, (1023, 1024, 1025)),
            "copy source lo - 1 / lo / lo + 1": (S.src_lo, (-1, 0, 1))}
    for name, (c, keys) in both.items():
        print(f"  D: {name}:", " | ".join(str(c[k]) for k in keys))
        assert all(c[k] >= 1 for k in keys), name
    print(f"  D: k4_literal_hbm (dst & 3, src & 3) pairs: {len(S.hbm_pairs)}")
    assert len(S.hbm_pairs) == 16
    ranges, out_bytes = frame_edge_ranges()
    st, units = frm.plan(starts, ranges, out_bytes)
    edge = sum(1 for u in units if u[5])
    print(f"  D: edge ranges: {len(ranges)}, staged units {edge}, interior units {len(units) - edge}, "
          f"out_offset residues {sorted({o % 16 for _, _, o in ranges})}")
    assert st == [0] * len(ranges) and edge == 2 * len(ranges) and len(units) > 4 * edge

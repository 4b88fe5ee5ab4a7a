"""Translation invariance of the range, record and CRC calls at positions across
2^32: a call's output and statuses must not change when every
position it is given -- stream positions, the window origin, table entries,
decoded starts, record offsets, output offsets -- is moved by a constant.  The
other suites of these calls work below 1 MiB; here the same small planted inputs
(imported from them, high_positions.py lays them out) stand around 2^32 of two
arenas of 2^33 + 32 MiB: `src` (0x5A), whose base a call gets as position 0, and
`dst` (0xA5), passed whole as the output.  Every object lies in [2^32 - 32 MiB,
2^32 + 32 MiB), so a kernel that drops bit 32 of a position or wraps a small
negative difference in 32 bits still lands inside an arena, 4 GiB away: wrong
bytes or a disturbed sentinel, never an unmapped address.  No position above
2^33 reaches the GPU; those go to the three CPU plan checks.

After each call all of `dst` is compared on the device with its image -- the
expected slices where they belong, 0xA5 everywhere else -- in pieces of 256 MiB;
a range or record that failed while decoding has only its own range left out.
The expected bytes are the oracle's and the CPU models' of the small input, never
a GPU run's; for A-C the same call is made unshifted as well and must give the
same statuses and bytes (wrong at high positions, not wrong input).  `src` is
compared with a copy around every call and summed at setup and teardown.

A raw ranges relies on kr0_range_check and k4_body's RANGE form reading index
entries u and u + 1 of planned units only: the entries below unit K are filler.

Which case reaches which kernel with bit 32 set on one side and clear on the
other (a 32-bit cast of pos / land / co, or an rfl64 without its high half, then
moves a load or store by 4 GiB into 0x5A / 0xA5 fill: a byte mismatch, a wrong
status or a disturbed sentinel):
* kr0_range_check: A, entries o0 / o1 and w0 / w1 on both sides, `o1 - w0` across
  (test_raw_ranges; the windows cut by one byte move w0 / w1 alone).
* kr4_decode_range_units: A, land below and above for interior units, one
  straddling; `dst - u * unit` with u * unit > 2^32 (8191: no shift); comp_at + c0
  on both sides, one unit's payload across; edge units on both sides.
* kr6_clip: A and B, land + lo below, across and above.
* kh2_headers / kh3_entries: B, chunks[] and starts[] on both sides, a header cut
  by 2^32 ("header") and the window's w0 / w1 on both sides.
* kr4_decode_frame_units: B, pos + 8 + bias and land on both sides, a payload
  across ("payload"), `ustatus + 4 p - 4 (u + 1)` unchanged by the shift (checked
  by the statuses).
* kh4_copy_stored: B, the stored chunks of "mixed" and "literal-tag edges".
* kf1_crc32c (both passes, entry form) and kh5_verify: B, every chunk's CRC is
  taken where it was decoded, both sides; the flipped CRC is found in the chunk at
  2^32; F reads entries ending and starting 0..3 bytes around 2^32.
* kq3_tables / kq4_derive / kq6_clip: C, comp and outp pairs on both sides, a
  payload and a chunk's output across; the long-record walk, both K4 passes
  (lunits forms, kr5_index_lrecords) under it on the derived batch.
* kr4_decode_records / kr5_record_lengths: D, record offsets and out offsets on
  both sides, one each across.
* kr1_match_records* / kr2_emit_records: D compress, sources of both classes on
  both sides, one across.
* lunits forms, kr5_index_lrecords: E, a record of 88 blocks across src's and
  dst's 2^32 with and without its table; the compress side on a source record
  whose second block holds 2^32.

Measured (test_layouts_have_their_properties prints them):
* A SINGLE: units [65,487, 65,586) of a stream of 4.3 GB; decoded units below / across
  / above 2^32: 49 / 0 / 50 (2^32 is a block edge), compressed 48 / 3 / 48; 285 ranges,
  30 of them ERR_DEPENDENT; plan units edge 97 / 0 / 236, interior 67 / 1 / 32.
* A STREAMS (lanes), chunk 8191 | 65,536: K 524,336 | 65,520, 33 units, decoded 16 / 1 /
  16 | 16 / 0 / 17, compressed 16 / 1 / 16; 62 ranges; edge units 34 / 0 / 23 | 31 / 0 / 26,
  interior 21 / 1 / 22 | 19 / 1 / 24.
* B three runs | mixed | literal-tag edges: chunks 2 / 1 / 3 | 1 / 1 / 2 | 6 / 1 / 1; 141 | 82
  | 308 ranges; edge units 63 / 0 / 97 | 29 / 1 / 66 | 256 / 1 / 127, interior 127 / 1 / 102 |
  34 / 0 / 42 | 569 / 0 / 111; ERR_CHECKSUM 88 | 52 | 124, ERR_TRUNCATED 46 | 34 | 70 ranges.
* C long (both formats): payloads and decoded chunks 3 / 1 / 2, 33 ranges, edge units 31
  / 0 / 16, interior 11 / 1 / 8; ERR_TRUNCATED 4; the raised entry gives ERR_INDEX and
  ERR_HEADER; slices: 17,207 | 21,947 ranges, payloads 1 / 1 / 1.
* D decode: 36 records (6 hostile), compressed and outputs 17 / 1 / 18; D compress:
  106 records, K1r sources 34 / 0 / 56, K1r64 8 / 1 / 7.
* E: the long record's 2^32 is its compressed byte 2,148,110 of 4,296,215 and its
  output byte 2,880,999 of 5,761,995; a short record on either side of it in src.
* F: 45 entries, 5 / 19 / 21.
* every case but C long (15) has ranges at all 16 dst residues mod 16.
* on the MI355X the GPU tests take 0.03 to 1.7 s each, the module 13 s.

Eight deliberate 32-bit truncations, built as two scratch libraries and run against
this module on the MI355X (none committed; each only moves a load or store by
4 GiB inside an arena):
* kr4_decode_range_units, `land` cast to 32 bits: all six test_raw_ranges (a sentinel
  disturbed 4 GiB below its range, the range itself left 0xA5).
* kr4_decode_frame_units, `pos` cast to 32 bits: the four test_frame_ranges on streams
  with compressed chunks (ERR_HEADER for the ranges touching a chunk above 2^32);
  the stream of stored chunks only does not reach this kernel and passes.
* kq3_tables, `co` cast to 32 bits where the payload's preamble is read: all six
  test_container_ranges (ERR_HEADER).
* kr4_decode_records, `co` cast to 32 bits in rec.c0: test_records_decode_and_lengths.
* kr1_record, the high half of the source offset's rfl64 dropped: test_records_compress
  (sizes and bytes of the records above 2^32).
* k4_long_unit, `co` cast to 32 bits in `(bias + co) & ~3`: test_long_records_decode (a
  first layout with every record starting below 2^32 passed it: a short record now
  stands on either side of the long one).
* kf1_crc32c's entry form, `off` cast to 32 bits: test_crc32c_entries and all six
  test_frame_ranges (ERR_CHECKSUM).
* kr0_range_check, `o1` cast to 32 bits: all six test_raw_ranges (ERR_TRUNCATED for the
  units above 2^32).
  The tests of calls the broken kernel is not part of passed in each run.
"""
import contextlib

import numpy as np
import pytest
import torch

import container_ranges_model as crm
import frame_model as fm
import frame_ranges_model as frm
import high_positions as hp
import ranges_model as rm
import record_layouts as rl
import snappy_amd
import test_k1r_k2_record_forms as kf
import test_long_records as lr
from high_positions import ARENA, BLOCK, E, HI, LO, OK, P32, PIECE, SINGLE, STREAMS

SENT = hp.DST_FILL


# ---------------------------------------------------------------------------
# the arenas
# ---------------------------------------------------------------------------
def pieces(a, b):
    return [(p, min(p + PIECE, b)) for p in range(a, b, PIECE)]


def arena_sum(t):
    return sum(int(t[a:b].sum(dtype=torch.int64).item()) for a, b in pieces(0, ARENA))


def dev(b):
    a = np.frombuffer(bytes(b), dtype=np.uint8).copy() if not isinstance(b, np.ndarray) else np.array(b)
    return torch.from_numpy(a).cuda() if a.size else torch.empty(0, dtype=torch.uint8, device="cuda")


def i64(v):
    return torch.tensor([x - (1 << 64) if x >= 1 << 63 else x for x in v], dtype=torch.int64, device="cuda")


def flat(p):
    return i64([x for q in p for x in q])


class Arena:
    def __init__(self):
        self.src = torch.full((ARENA,), hp.SRC_FILL, dtype=torch.uint8, device="cuda")
        self.dst = torch.full((ARENA,), hp.DST_FILL, dtype=torch.uint8, device="cuda")
        assert self.src.data_ptr() % 16 == 0 and self.dst.data_ptr() % 16 == 0
        assert self.src.numel() == self.dst.numel() == ARENA

    @contextlib.contextmanager
    def placed(self, objects):
        """objects [(offset, bytes)] in src for the calls made inside; no call may change src"""
        try:
            for at, data in objects:
                assert LO <= at and at + len(data) <= HI
                self.src[at:at + len(data)] = dev(data)
            before = self.src[LO:HI].clone()
            yield
            assert torch.equal(self.src[LO:HI], before), "a call wrote into src"
        except BaseException:
            self.dst.fill_(SENT)   # (a failure before check(): the next test starts from the sentinel)
            raise
        finally:
            self.src[LO:HI].fill_(hp.SRC_FILL)

    def window(self):
        return self.dst[LO:HI].cpu().numpy()

    def check(self, writes, what, fetch=False):
        """All of dst against its image: writes = [(offset, bytes)] and [(offset, length)]
        (a range that is not compared); 0xA5 everywhere else.  dst is the sentinel again
        afterwards.  -> dst[LO:HI] on the host (fetch), as the call left it"""
        img = np.full(HI - LO, SENT, dtype=np.uint8)
        care = np.ones(HI - LO, dtype=bool)
        for at, w in writes:
            ln = w if isinstance(w, int) else len(w)
            assert LO <= at and at + ln <= HI, (what, at, ln)
            if isinstance(w, int):
                care[at - LO:at - LO + ln] = False
            else:
                img[at - LO:at - LO + ln] = w if isinstance(w, np.ndarray) else np.frombuffer(bytes(w), dtype=np.uint8)
        d_img, d_care = torch.from_numpy(img).cuda(), torch.from_numpy(care).cuda()
        got = self.window() if fetch else None
        bad = []
        for a, b in pieces(0, LO) + pieces(HI, ARENA):
            if not bool((self.dst[a:b] == SENT).all()):
                at = a + int((self.dst[a:b] != SENT).to(torch.uint8).argmax().item())
                bad.append(f"sentinel disturbed at dst byte {at} = 2^32 {at - P32:+d}: {int(self.dst[at].item()):#x}")
                self.dst[a:b].fill_(SENT)
        diff = (self.dst[LO:HI] != d_img) & d_care
        if bool(diff.any()):
            k = int(diff.to(torch.uint8).argmax().item())
            at = LO + k
            own = [i for i, (o, w) in enumerate(writes) if o <= at < o + (w if isinstance(w, int) else len(w))]
            where = f"byte {at - writes[own[0]][0]} of write {own[0]}" if own else "a sentinel byte"
            bad.append(f"{int(diff.sum().item())} bytes differ, the first at dst byte {at} = 2^32 {at - P32:+d}: "
                       f"{where}, "
                       f"{int(self.dst[at].item()):#x} for {int(img[k]):#x}")
        self.dst[LO:HI].fill_(SENT)
        assert not bad, (what, bad)
        return got


@pytest.fixture(scope="module")
def arena():
    a = Arena()
    before = arena_sum(a.src)
    assert before == hp.SRC_FILL * ARENA
    yield a
    after = arena_sum(a.src)
    clean = all(bool((a.dst[p:q] == SENT).all()) for p, q in pieces(0, ARENA))
    del a.src, a.dst
    torch.cuda.empty_cache()
    assert after == before, "src changed"
    assert clean, "dst was left disturbed"


def same_as_unshifted(got, small_out, o, small_ranges=(), skip=()):
    """dst[o, o + size) as the call left it is the unshifted call's whole buffer, but
    for the own ranges of the ranges in `skip` (they failed while decoding)"""
    mine = got[o - LO:o - LO + small_out.size]
    ne = mine != small_out
    for i in skip:
        _, ln, oo = small_ranges[i]
        ne[oo:oo + ln] = False
    assert not ne.any(), f"differs from the unshifted call at its output byte {int(np.flatnonzero(ne)[0])}"


def first_failure(st):
    return next((s for s in st if s != 0), 0)


def sentinel(size):
    return torch.full((max(size, 1),), SENT, dtype=torch.uint8, device="cuda")


def slots_env(monkeypatch, slots):
    if slots:
        monkeypatch.setenv("SNAPPY_AMD_RANGE_SLOTS", str(slots))
    else:
        monkeypatch.delenv("SNAPPY_AMD_RANGE_SLOTS", raising=False)


# ---------------------------------------------------------------------------
# A: raw range decode
# ---------------------------------------------------------------------------
RAW = [(SINGLE, BLOCK), (STREAMS, 8191), (STREAMS, BLOCK)]


def raw_call(codec, c, comp, origin, offs, n, ranges, out):
    _, st = codec.decompress_ranges_tensor(comp, offs, n, ranges, out=out, chunk=c.unit, layout=c.layout,
                                           comp_origin=origin)
    st = [int(x) for x in st.cpu().numpy()]
    assert codec.last_ranges_status == first_failure(st)
    return st


@pytest.mark.gpu
@pytest.mark.parametrize("slots", [0, 3])
@pytest.mark.parametrize("layout,chunk", RAW, ids=["single", "streams-8191", "streams-65536"])
def test_raw_ranges(codec, arena, monkeypatch, layout, chunk, slots):
    """A: kr0_range_check, kr4_decode_range_units and kr6_clip on units [K, K + m) of a
    stream of more than 4 GiB; with 3 staging slots they are reused by every launch group."""
    slots_env(monkeypatch, slots)
    c = hp.raw_case(layout, chunk)
    offs, small_offs, small = dev(c.index), dev(c.small_index), dev(np.frombuffer(c.small, dtype=np.uint8))
    with arena.placed([(c.C, c.small)]):
        st = raw_call(codec, c, arena.src[c.w0:c.w1], c.w0, offs, c.n, c.ranges, arena.dst)
        assert st == c.model, [(i, c.ranges[i], s, m) for i, (s, m) in enumerate(zip(st, c.model)) if s != m][:6]
        got = arena.check(hp.raw_writes(c, c.small_ranges, c.model, c.O), ("raw", layout, chunk), fetch=True)
        out = sentinel(c.small_total)
        assert raw_call(codec, c, small, 0, small_offs, c.n_small, c.small_ranges, out) == st
        same_as_unshifted(got, out.cpu().numpy(), c.O, c.small_ranges,
                          [i for i, m in enumerate(c.model) if m != OK and m not in hp.rp.EARLY])
        # the window one byte short (the last unit's bytes end at w1) and one byte late
        for cut0, cut1, model in ((0, 1, c.neg_short), (1, 0, c.neg_late)):
            w0, w1 = c.w0 + cut0, c.w1 - cut1
            st = raw_call(codec, c, arena.src[w0:w1], w0, offs, c.n, c.neg, arena.dst)
            assert st == model, (cut0, cut1, st)
            got = arena.check(hp.raw_writes(c, c.neg_small, model, c.Oneg), ("raw window", cut0, cut1), fetch=True)
            out = sentinel(c.neg_total)
            assert raw_call(codec, c, small[cut0:small.numel() - cut1], cut0, small_offs, c.n_small,
                            c.neg_small, out) == model
            same_as_unshifted(got, out.cpu().numpy(), c.Oneg)


# ---------------------------------------------------------------------------
# B: framed range decode
# ---------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name,straddle", hp.FRAME_CASES)
def test_frame_ranges(codec, arena, name, straddle):
    """B: kh2_headers, kh3_entries, kr4_decode_frame_units, kh4_copy_stored, both
    kf1_crc32c passes, kh5_verify and kr6_clip through sub-tables with absolute
    positions; then a flipped stored CRC in the chunk at 2^32 and the window one byte short."""
    c = hp.frame_case(name, straddle)
    hchunks, hstarts, chunks, starts = i64(c.hchunks), i64(c.hstarts), i64(c.chunks), i64(c.starts)
    for stream, model, cut in ((c.stream, [OK] * len(c.ranges), 0), (c.flipped, c.crc, 0), (c.stream, c.short, 1)):
        partial = [i for i, s in enumerate(model) if s == hp.CHECKSUM]
        with arena.placed([(c.C + c.w0, stream[c.w0:c.w1])]):
            win = arena.src[c.C + c.w0:c.C + c.w1 - cut]
            _, st = codec.decompress_frame_ranges_tensor(win, c.C + c.w0, hchunks, hstarts, c.ranges, out=arena.dst)
            st = st.cpu().tolist()
            assert st == model, [(i, c.ranges[i], s, m) for i, (s, m) in enumerate(zip(st, model)) if s != m][:6]
            assert codec.last_ranges_status == first_failure(model)
            got = arena.check(hp.slice_writes(c.raw, c.small_ranges, model, c.O, (hp.CHECKSUM,)), (name, straddle, cut),
                              fetch=True)
        out = sentinel(c.small_total)
        _, st2 = codec.decompress_frame_ranges_tensor(dev(stream[c.w0:c.w1 - cut]), c.w0, chunks, starts,
                                                      c.small_ranges, out=out)
        assert st2.cpu().tolist() == st
        same_as_unshifted(got, out.cpu().numpy(), c.O, c.small_ranges, partial)


# ---------------------------------------------------------------------------
# C: container range decode
# ---------------------------------------------------------------------------
CONTAINER = [(f, w, 0) for f, w in hp.CONTAINER_CASES] + [(hp.cm.XERIAL, "long", 3), (hp.cm.HADOOP, "long", 3)]


@pytest.mark.gpu
@pytest.mark.parametrize("fmt,which,slots", CONTAINER)
def test_container_ranges(codec, arena, monkeypatch, fmt, which, slots):
    """C: kq3_tables, kq4_derive, the long-record decode of the derived batch (the
    per-record walk, both K4 passes) and kq6_clip; with a staging area of 3 blocks the
    long chunks run in several launch groups.  Then the window one byte short and a
    table entry's length raised by 1."""
    slots_env(monkeypatch, slots)
    c = hp.container_case(fmt, which)
    rows = [(c.houtp, c.outp, [OK] * len(c.ranges), 0)]
    if which == "long":
        rows += [(c.houtp, c.outp, c.short, 1), (c.hraised, c.raised, c.bad, 0)]
    for houtp, outp, model, cut in rows:
        with arena.placed([(c.C + c.w0, c.stream[c.w0:c.w1])]):
            win = arena.src[c.C + c.w0:c.C + c.w1 - cut]
            _, st = codec.decompress_container_ranges_tensor(win, c.C + c.w0, flat(c.hcomp), flat(houtp), c.ranges,
                                                             out=arena.dst)
            st = st.cpu().tolist()
            assert st == model, [(i, c.ranges[i], s, m) for i, (s, m) in enumerate(zip(st, model)) if s != m][:6]
            assert codec.last_ranges_status == first_failure(model)
            got = arena.check(hp.slice_writes(c.raw, c.small_ranges, model, c.O), (fmt, which, slots, cut), fetch=True)
        out = sentinel(c.small_total)
        _, st2 = codec.decompress_container_ranges_tensor(dev(c.stream[c.w0:c.w1 - cut]), c.w0, flat(c.comp),
                                                          flat(outp), c.small_ranges, out=out)
        assert st2.cpu().tolist() == st
        same_as_unshifted(got, out.cpu().numpy(), c.O)


# ---------------------------------------------------------------------------
# D: record batches
# ---------------------------------------------------------------------------
@pytest.mark.gpu
def test_records_decode_and_lengths(codec, arena):
    """D: kr4_decode_records and kr5_record_lengths, the blob in src and the outputs in
    dst on both sides of 2^32 and across it, hostile records between the good ones."""
    c = hp.records_case()
    out = rl.sentinel_buffer(c.size)
    rc0, small_st = rl.decode_records_call(codec, rl.to_device(c.blob, c.shift), c.c_descs, out, c.o_descs)
    want, writes = [], []
    for (s, w, code), (oo, ln), st0 in zip(c.items, c.ho, small_st.tolist()):
        if code is None:                      # the oracle refuses it, with no code of its own
            assert st0 < 0
            code = st0
        want.append(code)
        writes.append((oo, w if code == OK else ln))
    with arena.placed([(c.B, c.blob)]):
        st = codec.decompress_records_tensor(arena.src, flat(c.hc), arena.dst, flat(c.ho)).cpu().tolist()
        assert st == want and small_st.tolist() == want
        assert codec.last_records_status == rc0 == first_failure(want)
        arena.check(writes, "records")
        lens, lst = codec.records_length_tensor(arena.src, flat(c.hc))
        assert lens.cpu().tolist() == c.lens and not lst.cpu().numpy().any()
        arena.check([], "record lengths")


@pytest.mark.gpu
def test_records_compress(codec, arena):
    """D: kr1_match_records, kr1_match_records64 and kr2_emit_records on sources on
    both sides of src's 2^32; the output's offsets are the call's own prefix sums."""
    c = hp.compress_records_case()
    cap = snappy_amd.max_records_output(sum(len(r) for r in c.records), len(c.records))
    buf = sentinel(cap + 64)
    with arena.placed([(c.B, c.blob)]):
        payload, offs, status = codec.compress_records_tensor(arena.src, flat(c.hd), out=buf[:cap])
        arena.check([], "compress records")
    want = [kf.expected_stream(r) for r in c.records]
    sizes = [len(w) for w in want]
    assert not status.cpu().numpy().any() and codec.last_records_status == OK
    assert offs.cpu().tolist() == [0] + np.cumsum(sizes).tolist() and payload.numel() == sum(sizes)
    got = buf.cpu().numpy()
    bad = [i for i, w in enumerate(want) if got[sum(sizes[:i]):sum(sizes[:i + 1])].tobytes() != w]
    assert not bad, [(i, c.hd[i]) for i in bad[:6]]
    assert (got[sum(sizes):] == SENT).all(), "bytes written past the total"


# ---------------------------------------------------------------------------
# E: long records
# ---------------------------------------------------------------------------
@pytest.mark.gpu
def test_long_records_decode(codec, arena):
    """E: kr4_decode_lunits / kr4_back_lunits with the host-built table and without
    (kr5_index_lrecords must return the same entries), the long record across src's and
    dst's 2^32."""
    c = hp.long_case()
    writes = [(oo, it[1]) for it, (oo, _) in zip(c.items, c.ho)]
    with arena.placed([(c.B, c.blob)]):
        index, st = codec.records_index_tensor(arena.src, flat(c.hc), flat(c.ho))
        assert not st.cpu().numpy().any() and index[:len(c.tables)].cpu().tolist() == c.tables
        for table in (i64(c.tables), None):
            st = codec.decompress_long_records_tensor(arena.src, flat(c.hc), arena.dst, flat(c.ho), index=table)
            assert not st.cpu().numpy().any() and codec.last_records_status == OK
            arena.check(writes, ("long records", table is not None))


@pytest.mark.gpu
def test_long_records_compress(codec, arena):
    """E: the long-record compress on a source record whose second block holds 2^32."""
    c = hp.compress_long_case()
    want = [lr.expected_stream(r) for r in c.records]
    tables = [e for w, r in zip(want, c.records) for e in lr.walk_table(w, len(r))]
    total = sum(len(r) for r in c.records)
    cap = snappy_amd.max_long_records_output(total, len(c.records))
    buf = sentinel(cap + 64)
    with arena.placed([(o, r) for (o, _), r in zip(c.descs, c.records)]):
        payload, offs, status, index = codec.compress_long_records_tensor(arena.src, flat(c.descs), out=buf[:cap])
        arena.check([], "compress long records")
    sizes = [len(w) for w in want]
    assert not status.cpu().numpy().any() and offs.cpu().tolist() == [0] + np.cumsum(sizes).tolist()
    got = buf.cpu().numpy()
    assert got[:sum(sizes)].tobytes() == b"".join(want) and (got[sum(sizes):] == SENT).all()
    assert index[:len(tables)].cpu().tolist() == tables


# ---------------------------------------------------------------------------
# F: CRC-32C
# ---------------------------------------------------------------------------
@pytest.mark.gpu
def test_crc32c_entries(codec, arena):
    """F: kf1_crc32c's entry form on entries ending and starting 0..3 bytes around 2^32."""
    c = hp.crc_case()
    with arena.placed([(c.at, c.data)]):
        ol = flat(c.entries)
        raw = codec.crc32c_tensor(arena.src, ol, masked=False).cpu().numpy().view(np.uint32).tolist()
        msk = codec.crc32c_tensor(arena.src, ol, masked=True).cpu().numpy().view(np.uint32).tolist()
    for (a, ln), r, m, w in zip(c.entries, raw, msk, c.want):
        assert r == w and m == fm.mask(w), (a - P32, ln, hex(r), hex(w))


# ---------------------------------------------------------------------------
# the layouts (no GPU)
# ---------------------------------------------------------------------------
def test_layouts_have_their_properties():
    """No GPU: every object lies in [2^32 - E, 2^32 + E) of an arena of [0, 2^33 + E),
    every case crosses or abuts 2^32 as it claims, and each CPU model's plan of the
    shifted tables is the unshifted plan translated."""
    assert ARENA == 2 * P32 + E and E <= 64 << 20 and (LO, HI) == (P32 - E, P32 + E) and 0 < LO and HI < ARENA
    assert PIECE <= 256 << 20

    def dst_items(ranges):
        return [(oo, ln) for _, ln, oo in ranges]

    def residues(ranges):
        return sorted({oo % 16 for _, ln, oo in ranges if ln})

    # A
    for layout, chunk in RAW:
        c = hp.raw_case(layout, chunk)
        what = f"A {'SINGLE' if layout == SINGLE else 'STREAMS'} {chunk}"
        assert hp.inside([(c.C, len(c.small)), (c.w0, c.w1 - c.w0)] + c.units_comp + dst_items(c.ranges + c.neg))
        assert c.K * c.unit < P32 < (c.K + c.m) * c.unit and c.n < ARENA and c.index.size == c.K + c.m + 1
        assert (c.index[:c.K] == c.index[c.K]).all() and c.index[-1] & hp.MASK == c.w1
        assert c.index.nbytes <= 5 << 20 and (chunk == BLOCK or (c.K * c.unit) % 65536)
        st_s, units_s = rm.plan(c.n_small, c.unit, c.small_ranges, c.small_total)
        st_h, units_h = rm.plan(c.n, c.unit, c.ranges, ARENA)
        assert st_h == st_s == [OK] * len(c.ranges) and units_h == hp.translated(units_s, c.K, c.O)
        below, across, above = hp.sides(c.units_comp)
        us = hp.unit_sides(units_h)
        decoded = hp.sides([(u * c.unit, c.unit) for u in range(c.K, c.K + c.m)])
        print(f"{what}: K {c.K}, {c.m} units, decoded below / across / above 2^32: {decoded}, compressed {below} / "
              f"{across} / {above}; {len(c.ranges)} ranges, plan units {us}, dst residues {residues(c.ranges)}")
        assert below >= 5 and across >= 1 and above >= 5
        assert all(us.get((kind, side), 0) >= 1 for kind in ("edge", "interior") for side in ("below", "above"))
        assert us.get(("interior", "straddling"), 0) >= 1
        # a range whose first and last units are edge units on either side of 2^32
        across = [(a, ln) for a, ln, _ in c.ranges if a < P32 < a + ln and a % c.unit and (a + ln) % c.unit]
        assert any((a + ln - 1) // c.unit > a // c.unit for a, ln in across)
        if chunk == BLOCK:
            assert any((a + ln - 1) // c.unit - a // c.unit == 1 for a, ln in across)
        if layout == SINGLE:
            assert c.model.count(hp.DEP) >= 30 and c.index[c.K] & hp.MASK == c.C + c.pre
        # the window negatives: a range in the first unit (its entry is w0), one in unit K + j, one in the last
        # unit (its end is w1)
        assert [(a // c.unit, (a + ln - 1) // c.unit) for a, ln, _ in c.neg] == \
            [(c.K + u, c.K + u) for u in (0, c.j, c.m - 1)]
        assert (c.neg_short, c.neg_late) == ([OK, OK, hp.TRUNC], [hp.TRUNC, OK, OK])
        assert c.index[c.K] & hp.MASK == c.w0 and c.units_comp[0][0] + c.units_comp[0][1] < c.w1 - 1
        assert c.units_comp[-1][0] > c.w0 + 1
    # B
    types = set()
    for name, straddle in hp.FRAME_CASES:
        c = hp.frame_case(name, straddle)
        assert hp.inside([(c.C + c.w0, c.w1 - c.w0)] + c.units_comp + dst_items(c.ranges))
        assert c.hstarts[0] < P32 < c.hstarts[-1] < ARENA and c.hchunks[-1] < ARENA
        cut = c.header_at < P32 < c.header_at + 8 if straddle == "header" else c.payload[0] < P32 < sum(c.payload)
        assert cut and c.header_at == c.hchunks[c.j]
        st_s, units_s = frm.plan(c.starts, c.small_ranges, c.small_total)
        st_h, units_h = frm.plan(c.hstarts, c.ranges, ARENA)
        assert st_h == st_s == [OK] * len(c.ranges) and units_h == hp.translated(units_s, 0, c.O)
        us = hp.unit_sides(units_h)
        kinds = sorted({c.stream[p] for p in c.chunks[:-1]})
        types |= set(kinds)
        print(f"B {name} ({straddle} across): chunks below / across / above 2^32: {hp.sides(c.units_comp)}, "
              f"types {kinds}; "
              f"{len(c.ranges)} ranges, plan units {us}, dst residues {residues(c.ranges)}; "
              f"ERR_CHECKSUM {c.crc.count(hp.CHECKSUM)}, ERR_TRUNCATED {c.short.count(hp.TRUNC)}")
        assert all(us.get((kind, side), 0) >= 1 for kind in ("edge", "interior") for side in ("below", "above"))
        assert hp.sides(dst_items(c.ranges))[1] >= 1
    assert types == {0, 1}
    # C
    for fmt, which in hp.CONTAINER_CASES:
        c = hp.container_case(fmt, which)
        assert hp.inside([(c.C + c.w0, c.w1 - c.w0)] + c.hcomp + dst_items(c.ranges))
        assert c.houtp[0][0] < P32 < sum(c.houtp[-1]) < ARENA and hp.sides(c.hcomp)[1] == 1
        tabs = [(c.outp, c.houtp)] + ([(c.raised, c.hraised)] if which == "long" else [])
        for outp, houtp in tabs:
            st_s, units_s = crm.plan(outp, c.small_ranges, c.small_total)
            st_h, units_h = crm.plan(houtp, c.ranges, ARENA)
            assert st_h == st_s and units_h == hp.translated(units_s, 0, c.O)
        us = hp.unit_sides(crm.plan(c.houtp, c.ranges, ARENA)[1])
        print(f"C format {fmt} {which}: payloads below / across / above 2^32: {hp.sides(c.hcomp)}, decoded "
              f"{hp.sides(c.houtp)}; {len(c.ranges)} ranges, plan units {us}, dst residues {residues(c.ranges)}"
              + (f"; ERR_TRUNCATED {c.short.count(hp.TRUNC)}, raised entry {sorted(set(c.bad))}" if which == "long"
                 else ""))
        assert sum(v for (kind, side), v in us.items() if side == "straddling") >= 1
        assert any(side == "below" for _, side in us) and any(side == "above" for _, side in us)
        if which == "long":
            assert max(ln for _, ln in c.outp) > BLOCK
    # D
    c = hp.records_case()
    assert hp.inside([(c.B, len(c.blob))] + c.hc + c.ho) and c.B % 4 == c.shift and c.O % 16 == 0
    assert all(c.blob[a:a + ln] == s for (a, ln), (s, _, _) in zip(c.c_descs, c.items))
    print(f"D decode: {len(c.items)} records ({len(hp.HOSTILE)} hostile), compressed below / across / above 2^32: "
          f"{hp.sides(c.hc)}, outputs {hp.sides(c.ho)}, dst residues {sorted({o % 16 for o, _ in c.ho})}")
    assert min(hp.sides(c.hc)) >= 1 and min(hp.sides(c.ho)) >= 1
    c = hp.compress_records_case()
    assert hp.inside([(c.B, len(c.blob))] + c.hd) and c.B % 4 == c.shift
    by = {k: hp.sides([d for d, r in zip(c.hd, c.records) if kf.cls(r) == k]) for k in ("k1r", "k1r64")}
    print(f"D compress: {len(c.records)} records, sources below / across / above 2^32 per class: {by}")
    assert all(v[0] >= 1 and v[2] >= 1 for v in by.values()) and hp.sides(c.hd)[1] == 1
    # E
    c = hp.long_case()
    assert hp.inside([(c.B, len(c.blob))] + c.hc + c.ho)
    assert hp.sides(c.hc[1:2]) == hp.sides(c.ho[1:2]) == (0, 1, 0) and len(c.tables) == 2 + 89 + 1 + 2
    assert hp.sides([d for d, it in zip(c.hc, c.items) if it[1]]) == (1, 1, 1)
    print(f"E decode: records' compressed bytes below / across / above 2^32: {hp.sides(c.hc)}, "
          f"outputs {hp.sides(c.ho)}; "
          f"the long record's 2^32 is its compressed byte {P32 - c.hc[1][0]} of {c.hc[1][1]}, output byte "
          f"{P32 - c.ho[1][0]} of {c.ho[1][1]}")
    c = hp.compress_long_case()
    assert hp.inside(c.descs) and hp.sides(c.descs) == (1, 1, 1) and c.descs[1][1] == 3 * BLOCK + 61001
    # F
    c = hp.crc_case()
    assert hp.inside(c.entries + [(c.at, len(c.data))])
    assert sorted({ln for _, ln in c.entries}) == hp.CRC_LENGTHS
    for ln in hp.CRC_LENGTHS:
        assert {a - P32 for a, n in c.entries if n == ln} == {k - ln for k in range(4)} | set(range(4)) | {-(ln // 2)}
    print(f"F: {len(c.entries)} entries, below / across / above 2^32: {hp.sides(c.entries)}")

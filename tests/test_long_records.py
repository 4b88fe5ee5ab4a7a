"""Long records: record batches whose records hold 0..2^30
decoded bytes, each one raw Snappy stream of ceil(L / 65536) blocks with one
preamble, compressed, indexed and decoded in one call each.

The checker of every compressed record is oracle.compress(record) (the empty
record's expectation is the format's byte 00); the expected decoded bytes are
the input, or oracle.decompress for streams of other writers.  The expected
block table of a record is a Python walk of its stream: entry k is where the
element holding output byte 65536 k starts, counted from the record's first
byte, with the bytes of that element before the block in bits 40..63; the last
entry is the compressed length.  Decode statuses of foreign and hostile
records are compared with snappy_amd_index_device followed by a SINGLE-layout
decode of that record alone.

Shapes: lengths one byte around every block edge and around the K1r / K1r64
class edge of a record's last block (32,768 / 32,769 bytes past a block edge),
mixed with short records; 8,193+ units in one call (past the one-wave scan) with
records' first units on both sides of 64- and 256-thread boundaries; batches of
a few MB at most.
"""
import ctypes
import functools
import random

import numpy as np
import pytest

import datagen
import oracle
import snappy_amd
from golden_inputs import build_stream, random_ops

gpu = pytest.mark.gpu

SENT = 0xA5
BLOCK = 65536
LONG = [65537, 98304, 98305, 131072, 131073, 3 * 65536 + 1, 5 * 65536 + 17]
SHORT = [0, 1, 100, 32768, 32769, 65536]


def torch_():
    import torch
    return torch


def varint(n: int) -> bytes:
    out = bytearray()
    while n >= 0x80:
        out.append((n & 0x7F) | 0x80)
        n >>= 7
    out.append(n)
    return bytes(out)


def enc_literal(data: bytes) -> bytes:
    n = len(data) - 1
    if n < 60:
        return bytes([n << 2]) + data
    k = (n.bit_length() + 7) // 8
    return bytes([(59 + k) << 2]) + n.to_bytes(k, "little") + data


def enc_copy2(length: int, offset: int) -> bytes:
    assert 1 <= length <= 64 and 0 <= offset < 65536
    return bytes([((length - 1) << 2) | 2]) + offset.to_bytes(2, "little")


@functools.lru_cache(maxsize=None)
def expected_stream(record: bytes) -> bytes:
    return oracle.compress(record) if record else b"\x00"


def nblk_of(n: int) -> int:
    return (n + BLOCK - 1) // BLOCK


def walk_table(stream: bytes, n: int) -> list:
    """The block table of one record's stream of n decoded bytes."""
    if n == 0:
        return [0]
    ip = 0
    while stream[ip] & 0x80:
        ip += 1
    ip += 1
    entries, op, unit = [0], 0, 1
    while op < n:
        x, tag = ip, stream[ip]
        kind = tag & 3
        if kind == 0:
            ln = (tag >> 2) + 1
            ip += 1
            if ln > 60:
                k = ln - 60
                ln = int.from_bytes(stream[ip:ip + k], "little") + 1
                ip += k
            ip += ln
        elif kind == 1:
            ln, ip = ((tag >> 2) & 7) + 4, ip + 2
        elif kind == 2:
            ln, ip = (tag >> 2) + 1, ip + 3
        else:
            ln, ip = (tag >> 2) + 1, ip + 5
        while unit * BLOCK < op + ln and unit * BLOCK < n:
            entries.append(x | ((unit * BLOCK - op) << 40))
            unit += 1
        op += ln
        if op == unit * BLOCK and op < n:
            entries.append(ip)
            unit += 1
    entries.append(len(stream))
    assert len(entries) == nblk_of(n) + 1
    return entries


def content(kind: str, n: int, seed: int) -> bytes:
    return datagen.make(kind, n, seed).tobytes()


def dev_i64(values):
    torch = torch_()
    return torch.tensor(list(values), dtype=torch.int64, device="cuda")


def dev_u8(data: bytes):
    torch = torch_()
    a = np.frombuffer(bytes(data), dtype=np.uint8).copy()
    return torch.from_numpy(a).cuda() if a.size else torch.empty(0, dtype=torch.uint8, device="cuda")


def compress_call(codec, base, descs, out_cap=None, index_cap=None, in_bytes=None, with_index=True):
    """The C call on sentinel-filled buffers.  descs: [(offset, length)].
    -> rc, out (whole buffer), offsets, status, out_len, index (whole buffer; -7 where unwritten)"""
    torch = torch_()
    count = len(descs)
    total = sum(ln for _, ln in descs if ln <= snappy_amd.LONG_RECORD_MAX)
    cap = snappy_amd.max_long_records_output(total, count) if out_cap is None else out_cap
    icap = snappy_amd.max_records_index(total, count) if index_cap is None else index_cap
    out = torch.full((cap + 64,), SENT, dtype=torch.uint8, device="cuda")
    offs = torch.full((count + 1,), -7, dtype=torch.int64, device="cuda")
    index = torch.full((icap + 8,), -7, dtype=torch.int64, device="cuda")
    status = torch.full((max(count, 1),), 77, dtype=torch.int32, device="cuda")
    ol = dev_i64(v for d in descs for v in d)
    got = ctypes.c_size_t(12345)
    codec._bind_stream()
    rc = snappy_amd.lib().snappy_amd_compress_long_records_device(
        codec._h, ctypes.c_void_p(base.data_ptr()), base.numel() if in_bytes is None else in_bytes,
        ctypes.c_void_p(ol.data_ptr()), count, ctypes.c_void_p(out.data_ptr()), cap, ctypes.c_void_p(offs.data_ptr()),
        ctypes.c_void_p(index.data_ptr()) if with_index else None, icap, ctypes.c_void_p(status.data_ptr()),
        ctypes.byref(got))
    torch.cuda.synchronize()
    return rc, out.cpu().numpy(), offs.cpu().numpy(), status.cpu().numpy()[:count], got.value, index.cpu().numpy()


def check_batch(codec, blob: bytes, descs, refused=None):
    """compress descs of blob: every accepted record bit-exact against the oracle,
    d_offsets the prefix sum, every table entry the Python walk's, nothing written
    past the total or past the tables.  -> (payload bytes, offsets, table list)"""
    refused = refused or {}
    rc, out, offs, status, out_len, index = compress_call(codec, dev_u8(blob), descs)
    want = [b"" if i in refused else expected_stream(blob[o:o + ln]) for i, (o, ln) in enumerate(descs)]
    assert rc == (refused[min(refused)] if refused else snappy_amd.OK)
    sizes = [len(w) for w in want]
    assert offs.tolist() == [0] + np.cumsum(sizes).tolist(), "d_offsets is not the prefix sum of the oracle's sizes"
    assert out_len == sum(sizes)
    flat = out.tobytes()
    for i, w in enumerate(want):
        assert flat[offs[i]:offs[i + 1]] == w, f"record {i} {descs[i]} differs from the oracle"
    assert (out[out_len:] == SENT).all(), "bytes written past the total"
    assert status.tolist() == [refused.get(i, 0) for i in range(len(descs))]
    table = []
    for i, (o, ln) in enumerate(descs):
        table += [0] if i in refused else walk_table(want[i], ln)
    assert index[:len(table)].tolist() == table, "block tables differ from the walk of the oracle's streams"
    assert (index[len(table):] == -7).all(), "entries written past the tables"
    return flat[:out_len], offs, table


def decode_call(codec, comp, c_descs, out, o_descs, index=None, comp_bytes=None, out_bytes=None, with_status=True):
    """The C decode call with sync = 1 -> rc, status (numpy)"""
    torch = torch_()
    count = len(c_descs)
    status = torch.full((max(count, 1),), 77, dtype=torch.int32, device="cuda")
    c_ol, o_ol = dev_i64(v for d in c_descs for v in d), dev_i64(v for d in o_descs for v in d)
    idx = None if index is None else dev_i64(index)
    codec._bind_stream()
    rc = snappy_amd.lib().snappy_amd_decompress_long_records_device(
        codec._h, ctypes.c_void_p(comp.data_ptr()), comp.numel() if comp_bytes is None else comp_bytes,
        ctypes.c_void_p(c_ol.data_ptr()), count, ctypes.c_void_p(out.data_ptr()),
        out.numel() if out_bytes is None else out_bytes, ctypes.c_void_p(o_ol.data_ptr()),
        ctypes.c_void_p(idx.data_ptr()) if idx is not None else None,
        ctypes.c_void_p(status.data_ptr()) if with_status else None, 1)
    torch.cuda.synchronize()
    return rc, status.cpu().numpy()[:count]


def index_call(codec, comp, c_descs, lens, index_cap=None):
    """records_index_device -> rc, tables (numpy, -7 where unwritten), status"""
    torch = torch_()
    count = len(c_descs)
    cap = sum(nblk_of(n) + 1 for n in lens) if index_cap is None else index_cap
    index = torch.full((cap + 8,), -7, dtype=torch.int64, device="cuda")
    status = torch.full((max(count, 1),), 77, dtype=torch.int32, device="cuda")
    c_ol, o_ol = dev_i64(v for d in c_descs for v in d), dev_i64(v for n in lens for v in (0, n))
    codec._bind_stream()
    rc = snappy_amd.lib().snappy_amd_records_index_device(
        codec._h, ctypes.c_void_p(comp.data_ptr()), comp.numel(), ctypes.c_void_p(c_ol.data_ptr()), count,
        ctypes.c_void_p(o_ol.data_ptr()), ctypes.c_void_p(index.data_ptr()), cap, ctypes.c_void_p(status.data_ptr()))
    torch.cuda.synchronize()
    return rc, index.cpu().numpy(), status.cpu().numpy()[:count]


def single_reference(codec, stream: bytes, n: int):
    """snappy_amd_index_device + a SINGLE-layout decode of one stream alone ->
    (status, decoded bytes or None): what every record of a batch must report"""
    torch = torch_()
    d = dev_u8(stream)
    offs = torch.zeros(nblk_of(max(n, 1)) + 4, dtype=torch.int64, device="cuda")
    got = ctypes.c_size_t(0)
    codec._bind_stream()
    rc = snappy_amd.lib().snappy_amd_index_device(codec._h, ctypes.c_void_p(d.data_ptr()), len(stream),
                                                  ctypes.c_void_p(offs.data_ptr()), offs.numel(), ctypes.byref(got))
    if rc == snappy_amd.OK and got.value != n:
        rc = snappy_amd.ERR_HEADER
    if rc != snappy_amd.OK:
        return rc, None
    out = torch.zeros(max(n, 1), dtype=torch.uint8, device="cuda")
    rc = snappy_amd.lib().snappy_amd_decompress_device(codec._h, ctypes.c_void_p(d.data_ptr()),
                                                       ctypes.c_void_p(offs.data_ptr()), n, BLOCK, snappy_amd.SINGLE,
                                                       ctypes.c_void_p(out.data_ptr()))
    return rc, out.cpu().numpy().tobytes()[:n]


def scatter(lens, rng, gap_lo=1, gap_hi=40):
    """output ranges for records of these decoded lengths, in shuffled address
    order with gaps -> (o_descs, buffer size)"""
    order = list(range(len(lens)))
    rng.shuffle(order)
    at, descs = rng.randrange(gap_lo, gap_hi), [None] * len(lens)
    for i in order:
        descs[i] = (at, lens[i])
        at += lens[i] + rng.randrange(gap_lo, gap_hi)
    return descs, at


def check_decode(codec, streams, lens, want, index, rng, expect_status=None):
    """decode a batch into scattered ranges of a 0xA5-filled buffer: the records'
    bytes, their statuses, the canaries between the ranges"""
    torch = torch_()
    c_descs, blob = [], bytearray(b"\x5a" * 3)
    for s in streams:
        c_descs.append((len(blob), len(s)))
        blob += s + b"\x5a" * rng.randrange(0, 5)
    o_descs, size = scatter(lens, rng)
    out = torch.full((size,), SENT, dtype=torch.uint8, device="cuda")
    rc, status = decode_call(codec, dev_u8(bytes(blob)), c_descs, out, o_descs, index=index)
    expect_status = expect_status or [0] * len(streams)
    assert status.tolist() == expect_status
    bad = [s for s in expect_status if s]
    assert rc == (bad[0] if bad else snappy_amd.OK)
    got = out.cpu().numpy()
    canary = np.ones(size, dtype=bool)
    for i, (o, n) in enumerate(o_descs):
        canary[o:o + n] = False
        if expect_status[i] == 0:
            assert got[o:o + n].tobytes() == want[i], f"record {i} decoded wrong"
    assert (got[canary] == SENT).all(), "a byte outside the records' output ranges was written"


# ---- 1: block and class edges ----------------------------------------------------
@functools.lru_cache(maxsize=None)
def edge_batch():
    """(blob, descs): the long and the short lengths, kinds T, R, Z and P, laid out
    with gaps of 0..7 bytes so that the offsets cover every class mod 4, the
    descriptors shuffled against the address order"""
    rng = random.Random(41)
    recs = [(ln, "TRZP"[k % 4], k) for k, ln in enumerate(LONG + SHORT + LONG[:4])]
    blob, descs = bytearray(), []
    for k, (ln, kind, seed) in enumerate(recs):
        blob += bytes(rng.randrange(0, 8))
        while len(blob) % 4 != k % 4:
            blob += b"\x00"
        descs.append((len(blob), ln))
        blob += content(kind, ln, seed)
    assert {o % 4 for o, ln in descs if ln > BLOCK} == {0, 1, 2, 3}
    rng.shuffle(descs)
    return bytes(blob), descs


@gpu
def test_block_and_class_edges(codec):
    blob, descs = edge_batch()
    check_batch(codec, blob, descs)


# ---- 2: against the existing calls -----------------------------------------------
@gpu
def test_long_record_alone_is_the_single_stream_and_short_records_the_short_call(codec):
    torch = torch_()
    data = content("T", 5 * BLOCK + 17, 3)
    payload, offs, table = check_batch(codec, b"ab" + data, [(2, len(data))])
    comp, soffs = codec.compress_tensor(dev_u8(data), layout=snappy_amd.SINGLE)
    assert comp.cpu().numpy().tobytes() == payload
    assert soffs.cpu().numpy().tolist() == table
    # short records through the long call: the short call's bytes and offsets
    blob, descs = edge_batch()
    short = [d for d in descs if d[1] <= BLOCK]
    base = dev_u8(blob)
    ol = dev_i64(v for d in short for v in d)
    p_long, o_long, st, _ = codec.compress_long_records_tensor(base, ol)
    p_short, o_short, _ = codec.compress_records_tensor(base, ol)
    assert torch.equal(p_long, p_short) and torch.equal(o_long, o_short) and int(st.abs().sum()) == 0
    # and the short call still refuses what the long one takes
    with pytest.raises(snappy_amd.SnappyError):
        codec.compress_records([bytes(65537)])
    assert codec.compress_long_records([bytes(65537)]) == [oracle.compress(bytes(65537))]


# ---- 3: unit mapping and both scans ------------------------------------------------
@functools.lru_cache(maxsize=None)
def many_units_batch():
    """(blob, descs): 150 records of alternately 1 and 3 blocks of zeros among
    64-byte text records, placed so that the long records' first units have the
    residues 63, 0, 1 and 62 mod 64 in turn; 8,193+ units in all"""
    zeros, text = bytes(2 * BLOCK + 100), content("T", 64 * 1024, 9)
    blob = zeros + text
    descs, u, j = [], 0, 0
    first_units = []

    def filler():
        nonlocal u, j
        descs.append((len(zeros) + 64 * (j % 1024), 64))
        u, j = u + 1, j + 1

    for i in range(150):
        while u % 64 != (63, 0, 1, 62)[i % 4]:
            filler()
        first_units.append(u)
        ln = BLOCK if i % 2 == 0 else 2 * BLOCK + 100
        descs.append((0, ln))
        u += nblk_of(ln)
    while u < 8193 + 70:
        filler()
    assert u > 8192 and len(descs) > 64
    assert {f % 64 for f in first_units} == {63, 0, 1, 62}
    assert {255, 0, 1} <= {f % 256 for f in first_units}
    return blob, descs


@gpu
def test_unit_mapping_and_scans_past_one_wave(codec):
    blob, descs = many_units_batch()
    payload, offs, table = check_batch(codec, blob, descs)
    # the same units through the decode's plan, expansion and status fold
    rng = random.Random(5)
    streams = [payload[offs[i]:offs[i + 1]] for i in range(len(descs))]
    lens = [ln for _, ln in descs]
    want = [blob[o:o + ln] for o, ln in descs]
    check_decode(codec, streams, lens, want, table, rng)
    check_decode(codec, streams, lens, want, None, rng)


# ---- 4: refusals ---------------------------------------------------------------------
@gpu
def test_refusals_and_capacities(codec):
    data = content("T", 2 * BLOCK + 500, 7)
    n = len(data)
    descs = [(0, 70000), (0, (1 << 30) + 1), (100, n - 100), (n - 10, 11), (5, 0), (1000, 3 * 1000)]
    refused = {1: snappy_amd.ERR_UNSUPPORTED, 3: snappy_amd.ERR_ARG}
    check_batch(codec, data, descs, refused)
    # one short of either capacity: ERR_CAPACITY, nothing written
    good = [d for i, d in enumerate(descs) if i not in refused]
    total = sum(ln for _, ln in good)
    cap = snappy_amd.max_long_records_output(total, len(good))
    assert cap == total + total // 32 + 32 * (len(good) + total // BLOCK) + 16
    entries = sum(nblk_of(ln) + 1 for _, ln in good)
    assert entries <= snappy_amd.max_records_index(total, len(good))
    base = dev_u8(data)
    for kw in ({"out_cap": cap - 1}, {"index_cap": entries - 1}):
        rc, out, offs, status, out_len, index = compress_call(codec, base, good, **kw)
        assert rc == snappy_amd.ERR_CAPACITY
        assert (out == SENT).all() and (offs == -7).all() and (index == -7).all()
    rc, out, offs, status, out_len, index = compress_call(codec, base, good, out_cap=cap, index_cap=entries)
    assert rc == snappy_amd.OK and (index[:entries] != -7).all() and (index[entries:] == -7).all()
    # no table asked for: the same bytes
    rc2, out2, offs2, _, len2, index2 = compress_call(codec, base, good, with_index=False)
    assert rc2 == snappy_amd.OK and len2 == out_len and (out2[:len2] == out[:len2]).all() and (index2 == -7).all()


# ---- 5: round trip -------------------------------------------------------------------
@gpu
def test_round_trip_into_scattered_ranges(codec):
    blob, descs = edge_batch()
    payload, offs, table = check_batch(codec, blob, descs)
    streams = [payload[offs[i]:offs[i + 1]] for i in range(len(descs))]
    lens = [ln for _, ln in descs]
    want = [blob[o:o + ln] for o, ln in descs]
    rng = random.Random(8)
    check_decode(codec, streams, lens, want, table, rng)
    check_decode(codec, streams, lens, want, None, rng)
    # records_index_device reproduces compress's tables entry for entry (the records packed as compress left them)
    c_descs = [(int(offs[i]), int(offs[i + 1] - offs[i])) for i in range(len(descs))]
    rc, index, status = index_call(codec, dev_u8(payload), c_descs, lens)
    assert rc == snappy_amd.OK and status.tolist() == [0] * len(descs)
    assert index[:len(table)].tolist() == table and (index[len(table):] == -7).all()
    rc, index, _ = index_call(codec, dev_u8(payload), c_descs, lens, index_cap=len(table) - 1)
    assert rc == snappy_amd.ERR_CAPACITY and (index == -7).all()
    # the tensor forms and the conveniences
    recs = [want[i] for i in (0, 5, len(want) - 1)] + [b"", b"x"]
    comp = codec.compress_long_records(recs)
    assert comp == [expected_stream(r) for r in recs]
    assert codec.decompress_long_records(comp) == recs
    assert snappy_amd.decompress_long_records(snappy_amd.compress_long_records(recs[:2])) == recs[:2]


# ---- 6: streams of other writers -----------------------------------------------------
@gpu
def test_foreign_streams_among_ordinary_records(codec, golden):
    rng = random.Random(6)
    ordinary = [content("T", 70000, 1), content("R", 300, 2), b""]
    ord_streams = [expected_stream(r) for r in ordinary]
    group, size = [], 0
    vectors = list(golden["xblock_vectors"])
    for k, v in enumerate(vectors):
        stream = build_stream(random_ops(v["random"]["seed"], v["random"]["n_out"], v["random"]["max_off"])
                              if "random" in v else v["ops"])
        group.append((v, stream))
        size += len(stream)
        if size < (2 << 20) and k + 1 < len(vectors):
            continue
        streams, lens, want, expect = [ord_streams[0]], [len(ordinary[0])], [ordinary[0]], [0]
        for j, (w, s) in enumerate(group):
            ref_rc, ref_out = single_reference(codec, s, w["out_len"])
            dec = oracle.decompress(s)
            assert ref_rc == snappy_amd.OK and ref_out == dec and len(dec) == w["out_len"], w["name"]
            q = 1 + j % 2  # an ordinary record after every foreign one
            streams += [s, ord_streams[q]]
            lens += [w["out_len"], len(ordinary[q])]
            want += [dec, ordinary[q]]
            expect += [ref_rc, 0]
        check_decode(codec, streams, lens, want, None, rng, expect)
        table = [e for s, n in zip(streams, lens) for e in walk_table(s, n)]
        c_descs, blob = [], bytearray()
        for s in streams:
            c_descs.append((len(blob), len(s)))
            blob += s
        rc, index, status = index_call(codec, dev_u8(bytes(blob)), c_descs, lens)
        assert rc == snappy_amd.OK and status.tolist() == [0] * len(streams)
        assert index[:len(table)].tolist() == table, "the built tables differ from the Python walk"
        check_decode(codec, streams, lens, want, table, rng, expect)
        group, size = [], 0


# ---- 7: hostile records among good ones ------------------------------------------------
def hostile_parts():
    good = [content("T", 2 * BLOCK + 77, 11), content("T", 900, 12), content("Z", BLOCK + 1, 0)]
    return good, [expected_stream(g) for g in good]


@gpu
def test_hostile_streams_without_a_table(codec):
    torch = torch_()
    good, gs = hostile_parts()
    n0 = len(good[0])
    cut = gs[0][:len(gs[0]) * 3 // 5]                       # a stream cut mid-block
    # its first copy reaches one byte before the record's own first output byte
    body = bytes(range(10))
    reach = varint(70000) + enc_literal(body) + enc_copy2(4, 11) + enc_literal(content("R", 70000 - 14, 4))
    streams = [gs[0], cut, gs[1], gs[0], gs[2], reach, gs[1]]
    lens = [n0, n0, len(good[1]), n0 + 1, len(good[2]), 70000, len(good[1])]
    want = [good[0], None, good[1], None, good[2], None, good[1]]
    expect = [0, snappy_amd.ERR_TRUNCATED, 0, snappy_amd.ERR_HEADER, 0, snappy_amd.ERR_OFFSET, 0]
    for i in (1, 3, 5):
        assert single_reference(codec, streams[i], lens[i])[0] == expect[i], i
    # the records' outputs back to back: record 5's copy would read record 4's last byte
    c_descs, blob = [], bytearray()
    for s in streams:
        c_descs.append((len(blob), len(s)))
        blob += s
    o_descs, at = [], 16
    for n in lens:
        o_descs.append((at, n))
        at += n
    out = torch.full((at + 16,), SENT, dtype=torch.uint8, device="cuda")
    rc, status = decode_call(codec, dev_u8(bytes(blob)), c_descs, out, o_descs)
    assert status.tolist() == expect and rc == snappy_amd.ERR_TRUNCATED
    got = out.cpu().numpy()
    for i, (o, n) in enumerate(o_descs):
        if expect[i] == 0:
            assert got[o:o + n].tobytes() == want[i], i
    assert (got[:16] == SENT).all() and (got[at:] == SENT).all()
    assert (got[o_descs[1][0]:o_descs[1][0] + n0] == SENT).all(), "a record the index failed was decoded"
    assert (got[o_descs[3][0]:o_descs[3][0] + n0 + 1] == SENT).all(), "a record with a wrong preamble was decoded"
    # without status words the call still returns the first failure
    rc, _ = decode_call(codec, dev_u8(bytes(blob)), c_descs, out, o_descs, with_status=False)
    assert rc == snappy_amd.ERR_TRUNCATED


@gpu
def test_hostile_tables(codec):
    rng = random.Random(12)
    good, gs = hostile_parts()
    streams = [gs[0], gs[1], gs[0], gs[2], gs[0], gs[1], gs[0]]
    lens = [len(good[k]) for k in (0, 1, 0, 2, 0, 1, 0)]
    want = [good[k] for k in (0, 1, 0, 2, 0, 1, 0)]
    tables = [walk_table(s, n) for s, n in zip(streams, lens)]
    assert len(tables[0]) == 4
    tables[0][-1] -= 1             # the last entry is not the compressed length
    tables[2][1] += 1              # an entry one byte off its element's start
    tables[4][2] = len(gs[0]) + 1  # an entry beyond the record's compressed range
    expect = [snappy_amd.ERR_INDEX, 0, snappy_amd.ERR_INDEX, 0, snappy_amd.ERR_INDEX, 0, 0]
    check_decode(codec, streams, lens, want, [e for t in tables for e in t], rng, expect)


@gpu
def test_range_checks_come_before_any_access(codec):
    torch = torch_()
    good, gs = hostile_parts()
    blob = gs[0] + gs[1]
    comp = dev_u8(blob + bytes(64))
    a, b = len(gs[0]), len(gs[1])
    n0, n1 = len(good[0]), len(good[1])
    out = torch.full((n0 + n1 + 64,), SENT, dtype=torch.uint8, device="cuda")
    c_descs = [(0, a), (0, a), (a, b + 1), (a, b), (a, 0), (a, b)]
    o_descs = [(8, n0), (0, (1 << 30) + 1), (8, n1), (n0 + 8 + 40, n1), (8, n1), (n0 + 8, n1)]
    expect = [0, snappy_amd.ERR_UNSUPPORTED, snappy_amd.ERR_TRUNCATED, snappy_amd.ERR_CAPACITY, snappy_amd.ERR_HEADER, 0]
    # the call is told the buffers end where the good records end
    rc, status = decode_call(codec, comp, c_descs, out, o_descs, comp_bytes=a + b, out_bytes=n0 + 8 + n1 + 39)
    assert status.tolist() == expect and rc == snappy_amd.ERR_UNSUPPORTED
    got = out.cpu().numpy()
    assert got[8:8 + n0].tobytes() == good[0] and got[8 + n0:8 + n0 + n1].tobytes() == good[1]
    assert (got[:8] == SENT).all() and (got[8 + n0 + n1:] == SENT).all()


# ---- 8: scratch ----------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("shape", ["many_small", "one_long"])
def test_scratch_stays_under_its_bound(codec, shape):
    torch = torch_()
    if shape == "many_small":
        count, ln = 65536, 64
    else:
        count, ln = 1, 4 << 20
    data = content("T", count * ln, 21)
    base = dev_u8(data)
    off_len = dev_i64(v for i in range(count) for v in (i * ln, ln))
    codec.trim()
    payload, offs, status, index = codec.compress_long_records_tensor(base, off_len)
    bound = snappy_amd.max_long_records_scratch(count * ln, count)
    assert codec.device_bytes() <= bound
    assert int(status.abs().sum()) == 0
    o = offs.cpu().numpy()
    assert payload.cpu().numpy().tobytes()[:int(o[1])] == expected_stream(data[:ln])
    c_ol = torch.stack([offs[:-1], offs[1:] - offs[:-1]], dim=1).reshape(-1).contiguous()
    for idx in (index, None):
        out = torch.zeros(count * ln, dtype=torch.uint8, device="cuda")
        st = codec.decompress_long_records_tensor(payload, c_ol, out, off_len, index=idx)
        assert int(st.abs().sum()) == 0 and torch.equal(out, base)
        assert codec.device_bytes() <= bound
    codec.trim()


# ---- 9: CPU --------------------------------------------------------------------------
def test_scratch_bound_is_linear():
    for t in (0, 1, 64, 65536, 65537, 1 << 20, (1 << 30), 3 << 30, 1 << 36):
        for c in (0, 1, 2, 1000, 65536, 1 << 24, (1 << 31) - 1):
            assert snappy_amd.max_long_records_scratch(t, c) <= 2.5 * t + 256 * c + 65536, (t, c)


def test_size_functions_and_argument_handling():
    for t in (0, 1, 65536, 65537, 1 << 30):
        for c in (1, 3):
            assert snappy_amd.max_long_records_output(t, c) == t + t // 32 + 32 * (c + t // BLOCK) + 16
            assert snappy_amd.max_records_index(t, c) == t // BLOCK + 2 * c
            # every record's table fits, however the bytes are split among the records
            assert nblk_of(t) + 1 + 1 * (c - 1) <= snappy_amd.max_records_index(t, c)
            assert snappy_amd.max_long_records_scratch(t, c) >= 2 * t
        # a record of 0..65,536 bytes needs no more output room here than in the short call
        if t <= BLOCK:
            assert snappy_amd.max_long_records_output(t, 1) - snappy_amd.max_records_output(t, 1) in (0, 32)
    assert snappy_amd.LONG_RECORD_MAX == 1 << 30
    assert snappy_amd.records_table_bases([0, 1, 65536, 65537, 1 << 30]) == [0, 1, 3, 5, 8, 8 + 16385]
    # an empty batch needs no device; a record that is not bytes-like is refused before one is touched
    assert snappy_amd.compress_long_records([]) == [] and snappy_amd.decompress_long_records([]) == []
    with pytest.raises(TypeError):
        snappy_amd.compress_long_records([3.5])
    with pytest.raises(snappy_amd.SnappyError) as e:
        snappy_amd.decompress_long_records([b"\x00", b""])
    assert e.value.code == snappy_amd.ERR_HEADER

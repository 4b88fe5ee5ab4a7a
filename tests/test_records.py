"""Record batches: `count` independent raw Snappy streams of
0..65,536 bytes at (offset, length) pairs, compressed, measured and decoded in
one call each.

The checker of every compressed record is oracle.compress(record); the empty
record's expectation is the format's (the one byte 00: the oracle writes
nothing for empty input, which no decoder accepts).  Decode statuses are
compared with what a one-unit SNAPPY_AMD_STREAMS decode of the same bytes
reports where such a launch can express the case.

Shapes: the lengths are the edges of the code paths -- 0 (no match finder), 1..5
and 15..18 (below the first probe and around is_block_end's 16), 59..61 and
255..257 (literal header sizes), 4,095..4,097 (hash table size steps),
32,767..32,769 (K1r against K1r64) and 65,535 / 65,536 (the ring's last
segment, the largest record).  The whole file runs in a few seconds.
"""
import ctypes
import functools
import random

import numpy as np
import pytest

import datagen
import oracle
import snappy_amd

pytestmark = pytest.mark.gpu

SENT = 0xA5
LENGTHS = ([0, 1, 2, 3, 4, 5] + [15, 16, 17, 18] + [59, 60, 61] + [255, 256, 257] + [4095, 4096, 4097] +
           [32767, 32768, 32769] + [65535, 65536])


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


# ---- a small encoder for hand-built streams -----------------------------------
def enc_literal(data: bytes, declared: int = None) -> bytes:
    n = (len(data) if declared is None else declared) - 1
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


def content(kind: int, n: int, seed: int) -> bytes:
    """text, noise, or a short-period repeat"""
    if kind % 3 == 0:
        return datagen.make("T", n, seed).tobytes()
    if kind % 3 == 1:
        return datagen.make("R", n, seed).tobytes()
    return datagen.make("K", n, seed, period=7 + seed % 23).tobytes()


def dev_i64(values):
    torch = torch_()
    return torch.tensor(list(values), dtype=torch.int64, device="cuda")


def dev_u8(data: bytes, pad: int = 0):
    torch = torch_()
    a = np.frombuffer(bytes(data) + bytes(pad), dtype=np.uint8).copy()
    return torch.from_numpy(a).cuda() if a.size else torch.empty(0, dtype=torch.uint8, device="cuda")


def compress_call(codec, base, descs, out_cap=None, with_status=True, in_bytes=None):
    """The C call on a sentinel-filled output.  descs: [(offset, length)].
    -> rc, out (whole buffer, numpy), offsets (numpy, count + 1; sentinel-filled before), status, out_len"""
    torch = torch_()
    count = len(descs)
    total = sum(min(ln, 65536) for _, ln in descs)
    cap = snappy_amd.max_records_output(total, count) if out_cap is None else out_cap
    out = torch.full((cap + 64,), SENT, dtype=torch.uint8, device="cuda")
    offs = torch.full((count + 1,), -7, dtype=torch.int64, device="cuda")
    status = torch.full((max(count, 1),), 77, dtype=torch.int32, device="cuda")
    ol = dev_i64(v for d in descs for v in d)
    got = ctypes.c_size_t(12345)
    codec._bind_stream()
    rc = snappy_amd.lib().snappy_amd_compress_records_device(
        codec._h, ctypes.c_void_p(base.data_ptr()), base.numel() if in_bytes is None else in_bytes,
        ctypes.c_void_p(ol.data_ptr()), count, ctypes.c_void_p(out.data_ptr()), cap, ctypes.c_void_p(offs.data_ptr()),
        ctypes.c_void_p(status.data_ptr()) if with_status else None, ctypes.byref(got))
    torch.cuda.synchronize()
    return rc, out.cpu().numpy(), offs.cpu().numpy(), status.cpu().numpy()[:count], got.value


def check_batch(codec, blob: bytes, descs, refused=None, with_status=True):
    """compress descs of blob; every accepted record bit-exact against the oracle,
    the offsets their prefix sum, the sentinel untouched past the total"""
    refused = refused or {}
    base = dev_u8(blob)
    rc, out, offs, status, out_len = compress_call(codec, base, descs, with_status=with_status)
    want = [b"" if i in refused else expected_stream(blob[o:o + ln]) for i, (o, ln) in enumerate(descs)]
    first = min(refused) if refused else None
    assert rc == (refused[first] if refused else snappy_amd.OK)
    sizes = [len(w) for w in want]
    assert offs.tolist() == [0] + np.cumsum(sizes).tolist(), "d_offsets is not the prefix sum of the oracle's sizes"
    assert out_len == sum(sizes)
    flat = out.tobytes()
    for i, w in enumerate(want):
        assert flat[offs[i]:offs[i + 1]] == w, f"record {i} {descs[i]} differs from the oracle"
    assert (out[out_len:] == SENT).all(), "bytes written past the total"
    if with_status:
        assert status.tolist() == [refused.get(i, 0) for i in range(len(descs))]
    else:
        assert (status == 77).all() or len(descs) == 0
    return flat[:out_len], offs


# ---- batch 1: every length class, shuffled, every alignment ---------------------
@pytest.fixture(scope="module")
def batch1():
    """(blob, descs in batch order): 21 records of up to 32,768 bytes and 6 longer
    ones (the three long lengths twice, other contents) laid out with gaps of 0..7
    bytes so that each class sees every source alignment mod 4"""
    rng = random.Random(20)
    recs = [(ln, k) for k, ln in enumerate(LENGTHS)] + [(ln, k + 1) for k, ln in enumerate((32769, 65535, 65536))]
    rng.shuffle(recs)
    blob = bytearray()
    descs, seen = [], {False: 0, True: 0}
    for ln, k in recs:
        big = ln > 32768
        want_al = seen[big] % 4
        seen[big] += 1
        gap = (want_al - len(blob)) % 4 + (4 if rng.random() < 0.5 else 0)  # 0..7
        blob += bytes([0x5A]) * gap
        descs.append((len(blob), ln))
        blob += content(k, ln, 100 + k)
    blob += bytes(5)
    order = list(range(len(descs)))
    rng.shuffle(order)  # the batch lists the records in another order than they lie in memory
    descs = [descs[i] for i in order]
    for cls in (False, True):
        als = {o % 4 for o, ln in descs if (ln > 32768) == cls and ln}
        assert als == {0, 1, 2, 3}, (cls, als)
    return bytes(blob), descs


@pytest.fixture(scope="module")
def batch1_out(codec, batch1):
    blob, descs = batch1
    return check_batch(codec, blob, descs)


def test_length_classes_one_batch(batch1_out):
    """1: every length class in one shuffled batch, bit-exact (the fixture asserts)"""
    payload, offs = batch1_out
    assert len(offs) == len(LENGTHS) + 3 + 1


@pytest.mark.parametrize("case", ["small", "big", "empty", "one_each", "twice", "none"])
def test_plan_class_edges(codec, case):
    """2: batches holding one class only, one record of each class, a repeated
    descriptor, no record at all -- each its own call"""
    blob = content(0, 70000, 7)
    descs, refused = {
        "small": ([(3, 100), (200, 32768), (40000, 1), (33001, 4097)], {}),
        "big": ([(1, 65536), (2, 32769), (4467, 65533)], {}),
        "empty": ([(0, 0), (70000, 0), (17, 0)], {}),
        "one_each": ([(5, 0), (6, 5000), (7, 40000), (8, 65537)], {3: snappy_amd.ERR_UNSUPPORTED}),
        "twice": ([(1001, 3000), (9, 50000), (1001, 3000), (9, 50000)], {}),
        "none": ([], {}),
    }[case]
    payload, offs = check_batch(codec, blob, descs, refused)
    if case == "twice":
        assert payload[offs[0]:offs[1]] == payload[offs[2]:offs[3]] and payload[offs[1]:offs[2]] == payload[offs[3]:offs[4]]
    if case == "none":
        assert offs.tolist() == [0] and payload == b""


@pytest.mark.parametrize("chunk", [100, 4096, 32768, 65536])
def test_equals_the_fixed_layout(codec, chunk):
    """3: uniform descriptors give the bytes and offsets of compress_tensor(STREAMS)"""
    torch = torch_()
    n = 3 * chunk + chunk // 3 + 1 if chunk > 100 else 10 * chunk + 37
    x = torch.from_numpy(datagen.make("T", n, 31)).cuda()
    want, want_offs = codec.compress_tensor(x, chunk=chunk, layout=snappy_amd.STREAMS)
    descs = [(o, min(chunk, n - o)) for o in range(0, n, chunk)]
    payload, offs, status = codec.compress_records_tensor(x, dev_i64(v for d in descs for v in d))
    assert torch.equal(offs, want_offs)
    assert torch.equal(payload, want)
    assert not status.any()


def test_refusals(codec):
    """4: a 65,537-byte record and a range one byte past in_bytes among good
    neighbours; the first refusal is returned with and without d_status; a
    short out_cap fails before anything is written"""
    blob = content(0, 70000, 11)
    descs = [(10, 300), (100, 65537), (50000, 2000), (70000 - 99, 100), (3, 33000)]
    refused = {1: snappy_amd.ERR_UNSUPPORTED, 3: snappy_amd.ERR_ARG}
    check_batch(codec, blob, descs, refused)
    check_batch(codec, blob, descs, refused, with_status=False)
    check_batch(codec, blob, [descs[3], descs[0], descs[1]], {0: snappy_amd.ERR_ARG, 2: snappy_amd.ERR_UNSUPPORTED},
                with_status=False)
    good = [descs[0], descs[2], descs[4]]
    need = snappy_amd.max_records_output(sum(ln for _, ln in good), len(good))
    assert need == 35300 + 35300 // 32 + 32 * 3 + 16
    rc, out, offs, status, out_len = compress_call(codec, dev_u8(blob), good, out_cap=need - 1)
    assert rc == snappy_amd.ERR_CAPACITY
    assert (out == SENT).all() and (offs == -7).all() and (status == 77).all()
    rc, out, offs, status, out_len = compress_call(codec, dev_u8(blob), good, out_cap=need)
    assert rc == snappy_amd.OK and out_len == offs[-1] > 0


def test_scratch_is_linear_in_the_batch():
    """5: 65,536 records of 64 bytes on a fresh context: the scratch stays within
    the header's formula and far below a per-record 65,536-byte layout"""
    torch = torch_()
    count, ln = 65536, 64
    total = count * ln
    a = datagen.make("T", total, 5)
    x = torch.from_numpy(a).cuda()
    off_len = torch.stack([torch.arange(count, dtype=torch.int64) * ln, torch.full((count,), ln, dtype=torch.int64)],
                          dim=1).reshape(-1).cuda()
    c = snappy_amd.Codec(0)
    try:
        payload, offs, status = c.compress_records_tensor(x, off_len)
        held = c.device_bytes()
    finally:
        c.close()
    s = 2 * total + total // 128 + 64 * count + 256  # the formula of include/snappy_amd.h, restated
    bound = s + s // 8 + 16512
    print(f"device_bytes {held} (bound {bound}; a 65,536-byte token layout per record: {count * 131088})")
    assert bound == snappy_amd.max_records_scratch(total, count)
    assert held <= bound
    assert held < 256 << 20
    assert not status.any()
    o, p = offs.cpu().numpy(), payload.cpu().numpy().tobytes()
    for i in (0, 1, 4097, count - 1):
        assert p[o[i]:o[i + 1]] == expected_stream(a[i * ln:(i + 1) * ln].tobytes())


# ---- decode -------------------------------------------------------------------
def decode_call(codec, comp: bytes, c_descs, o_descs, out_bytes, with_status=True, comp_bytes=None, sync=1):
    """The C call on a sentinel-filled output -> rc, out (numpy), status"""
    torch = torch_()
    count = len(c_descs)
    d_comp = dev_u8(comp)
    out = torch.full((out_bytes + 16,), SENT, dtype=torch.uint8, device="cuda")
    status = torch.full((max(count, 1),), 77, dtype=torch.int32, device="cuda")
    c_ol, o_ol = dev_i64(v for d in c_descs for v in d), dev_i64(v for d in o_descs for v in d)
    codec._bind_stream()
    rc = snappy_amd.lib().snappy_amd_decompress_records_device(
        codec._h, ctypes.c_void_p(d_comp.data_ptr()), len(comp) if comp_bytes is None else comp_bytes,
        ctypes.c_void_p(c_ol.data_ptr()), count, ctypes.c_void_p(out.data_ptr()), out_bytes,
        ctypes.c_void_p(o_ol.data_ptr()), ctypes.c_void_p(status.data_ptr()) if with_status else None, sync)
    torch.cuda.synchronize()
    return rc, out.cpu().numpy(), status.cpu().numpy()[:count]


def scatter_layout(lengths, rng, align_classes=None):
    """output ranges with sentinel gaps of 0..7 bytes -> [(offset, length)], total"""
    pos, descs = 0, []
    for k, ln in enumerate(lengths):
        pos += (k % 4 - pos) % 4 + (4 if rng.random() < 0.5 else 0)
        descs.append((pos, ln))
        pos += ln
    return descs, pos + 3


def test_round_trip_into_scattered_ranges(codec, batch1, batch1_out):
    """6: batch 1's compressed records, decoded in another order into ranges
    separated by sentinel gaps; every source and destination alignment occurs"""
    blob, descs = batch1
    payload, offs = batch1_out
    rng = random.Random(6)
    order = list(range(len(descs)))
    rng.shuffle(order)
    c_descs = [(int(offs[i]), int(offs[i + 1] - offs[i])) for i in order]
    o_descs, out_bytes = scatter_layout([descs[i][1] for i in order], rng)
    assert {o % 4 for o, _ in c_descs} == {0, 1, 2, 3} and {o % 4 for o, ln in o_descs if ln} == {0, 1, 2, 3}
    for with_status in (True, False):
        rc, out, status = decode_call(codec, payload, c_descs, o_descs, out_bytes, with_status=with_status)
        assert rc == snappy_amd.OK
        image = np.full(out.size, SENT, dtype=np.uint8)
        for i, (o, ln) in zip(order, o_descs):
            image[o:o + ln] = np.frombuffer(blob[descs[i][0]:descs[i][0] + ln], dtype=np.uint8)
        bad = np.nonzero(out != image)[0]
        assert bad.size == 0, f"first differing output byte {bad[0]}"
        assert (status == (0 if with_status else 77)).all()


def lay_out(streams, rng=None):
    pos, descs = 0, []
    for s in streams:
        pos += 0 if rng is None else rng.randrange(4)
        descs.append((pos, len(s)))
        pos += len(s)
    comp = bytearray(pos)
    for (o, ln), s in zip(descs, streams):
        comp[o:o + ln] = s
    return bytes(comp), descs


def test_foreign_streams(codec, golden):
    """7: streams of other writers in one batch: all four tag types, 3- and 4-byte
    literal lengths, an RLE copy, a 65,536-byte literal, maximal-length copies"""
    cases = [(bytes.fromhex(v["stream_hex"]), bytes.fromhex(v["out_hex"])) for v in golden["decoder_vectors"]]
    assert len(cases) == 5
    lit = datagen.make("R", 65536, 3).tobytes()
    cases.append((varint(65536) + enc_literal(lit), lit))
    head = datagen.make("R", 64, 4).tobytes()
    cases.append((varint(65536) + enc_literal(head) + enc_copy2(64, 64) * 1023, head * 1024))
    cases.append((b"\x00", b""))
    rng = random.Random(7)
    comp, c_descs = lay_out([s for s, _ in cases], rng)
    o_descs, out_bytes = scatter_layout([len(w) for _, w in cases], rng)
    rc, out, status = decode_call(codec, comp, c_descs, o_descs, out_bytes)
    assert rc == snappy_amd.OK and not status.any()
    image = np.full(out.size, SENT, dtype=np.uint8)
    for (o, ln), (_, w) in zip(o_descs, cases):
        image[o:o + ln] = np.frombuffer(w, dtype=np.uint8)
    assert (out == image).all()


def streams_status(codec, stream: bytes, out_len: int) -> int:
    """what a one-unit SNAPPY_AMD_STREAMS decode of these bytes reports today"""
    torch = torch_()
    d = dev_u8(stream, pad=8)
    offs = dev_i64([0, len(stream)])
    out = torch.empty(out_len + 16, dtype=torch.uint8, device="cuda")
    codec._bind_stream()
    return snappy_amd.lib().snappy_amd_decompress_device(codec._h, ctypes.c_void_p(d.data_ptr()),
                                                         ctypes.c_void_p(offs.data_ptr()), out_len, out_len,
                                                         snappy_amd.STREAMS, ctypes.c_void_p(out.data_ptr()))


N_H = 300  # decoded length of the hostile records


def hostile_streams():
    body = datagen.make("T", N_H, 8).tobytes()
    good = expected_stream(body)
    E = snappy_amd
    return body, good, [
        # name, stream, expected status (checked against the one-unit STREAMS decode too)
        ("preamble + 1", varint(N_H + 1) + good[2:], E.ERR_HEADER),
        ("preamble - 1", varint(N_H - 1) + good[2:], E.ERR_HEADER),
        ("cut varint", b"\xac", E.ERR_HEADER),
        ("truncated literal", varint(N_H) + enc_literal(body[:100], declared=N_H), E.ERR_TRUNCATED),
        ("copy offset 0", varint(N_H) + enc_literal(body[:8]) + enc_copy2(8, 0) + enc_literal(body[16:]), E.ERR_OFFSET),
        ("copy before the start", varint(N_H) + enc_literal(body[:4]) + enc_copy2(8, 5) + enc_literal(body[12:]),
         E.ERR_OFFSET),
        ("element overruns", varint(N_H) + enc_literal(body[:296]) + enc_literal(body[:8]), E.ERR_OVERRUN),
    ]


def test_hostile_records_among_good_ones(codec):
    """8: each hostile record between two good ones; statuses as the one-unit
    STREAMS decode reports them, never positive; neighbours bit-exact; the
    sentinel around every failing record's range intact"""
    E = snappy_amd
    body, good, hostile = hostile_streams()
    assert good[:2] == varint(N_H)
    for name, s, want in hostile:
        assert streams_status(codec, s, N_H) == want, name
    streams, want_status = [good], [0]
    for name, s, want in hostile:
        streams += [s, good]
        want_status += [want, 0]
    comp, c_descs = lay_out(streams, random.Random(8))
    comp += bytes(16)
    comp_bytes = len(comp) - 16  # the call's comp_bytes: the last 16 bytes exist but are outside
    o_descs, out_bytes = scatter_layout([N_H] * len(streams), random.Random(9))
    # one more good record, listed last, at the very end of the output
    last = (out_bytes, N_H)
    out_bytes += N_H
    # the range cases: (compressed range, output range, status); none may load or store
    c_descs += [(comp_bytes - 5, 10), c_descs[0], c_descs[0], (c_descs[0][0], 0), (comp_bytes + 1, 0), c_descs[0]]
    o_descs += [(0, 0), (out_bytes - 10, N_H), (0, 65537), (0, 0), (0, 0), last]
    want_status += [E.ERR_TRUNCATED, E.ERR_CAPACITY, E.ERR_UNSUPPORTED, E.ERR_HEADER, E.ERR_TRUNCATED, 0]
    first = next(s for s in want_status if s)
    for with_status in (True, False):
        rc, out, status = decode_call(codec, comp, c_descs, o_descs, out_bytes, with_status=with_status,
                                      comp_bytes=comp_bytes)
        assert rc == first
        if with_status:
            assert status.tolist() == want_status
            assert (status <= 0).all()
        image = np.full(out.size, SENT, dtype=np.uint8)
        care = np.ones(out.size, dtype=bool)
        for (o, ln), st in zip(o_descs, want_status):
            if st == 0:
                image[o:o + ln] = np.frombuffer(body, dtype=np.uint8)
            elif st in (E.ERR_HEADER, E.ERR_TRUNCATED, E.ERR_OFFSET, E.ERR_OVERRUN) and ln == N_H:
                care[o:o + ln] = False  # a failing record may leave a prefix of its own range written
        bad = np.nonzero((out != image) & care)[0]
        assert bad.size == 0, f"byte {bad[0]} outside every failing record's range changed"
    # asynchronous form: OK now, the statuses in d_status
    rc, out, status = decode_call(codec, comp, c_descs, o_descs, out_bytes, comp_bytes=comp_bytes, sync=0)
    assert rc == E.OK and status.tolist() == want_status


def test_records_length(codec, batch1, batch1_out):
    """9: the preambles of batch 1, a 5-byte varint above 2^32, a 10-byte varint
    that never ends, a range cut inside the varint, a range outside the buffer"""
    E = snappy_amd
    blob, descs = batch1
    payload, offs = batch1_out
    big = (1 << 32) + 5
    extra = [varint(big) + b"\x00", b"\xff" * 10 + b"\x01", varint(65536) + b"\x00"]
    assert len(extra[0]) == 6
    comp, x_descs = lay_out(extra)
    x_descs[2] = (x_descs[2][0], 2)  # 80 80 04 cut after two bytes
    n1 = len(payload)
    c_descs = [(int(offs[i]), int(offs[i + 1] - offs[i])) for i in range(len(descs))]
    c_descs += [(n1 + o, ln) for o, ln in x_descs] + [(n1 + len(comp) - 1, 2), (n1 + len(comp), 0)]
    lens, status = codec.records_length_tensor(dev_u8(payload + comp), dev_i64(v for d in c_descs for v in d))
    assert lens.tolist() == [ln for _, ln in descs] + [big, 0, 0, 0, 0]
    assert status.tolist() == [0] * len(descs) + [0, E.ERR_HEADER, E.ERR_HEADER, E.ERR_TRUNCATED, E.ERR_HEADER]


def test_host_conveniences(codec):
    """10: lists of bytes in, lists of bytes out; a corrupt entry raises its code"""
    xs = [b"", b"a", content(0, 5000, 1), b"", content(2, 65536, 2), content(1, 33, 3)]
    comp = codec.compress_records(xs)
    assert comp == [expected_stream(x) for x in xs]
    assert codec.decompress_records(comp) == xs
    assert snappy_amd.decompress_records(snappy_amd.compress_records(xs[:3])) == xs[:3]
    assert codec.compress_records([]) == [] and codec.decompress_records([]) == []
    _, _, hostile = hostile_streams()
    for name, s, want in hostile[2:]:
        with pytest.raises(snappy_amd.SnappyError) as e:
            codec.decompress_records([comp[2], s, comp[1]])
        assert e.value.code == want, name
    with pytest.raises(snappy_amd.SnappyError) as e:
        codec.compress_records([b"x" * 65537])
    assert e.value.code == snappy_amd.ERR_UNSUPPORTED

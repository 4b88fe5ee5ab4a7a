"""Planted inputs of the container range decode tests, shared by
the CPU model test, the plan check and the GPU tests: which containers, which
ranges, where they land.  Every payload is written by hand as literal and copy
elements (container_cases' builders and the ones below), so nothing but the
models is needed to build them; the plain bytes are the reference."""
import random

import container_cases as cc
import container_model as cm
import container_ranges_model as crm

SENT = 0xA5
BLOCK = 65536


def copy2(length, offset):
    """one copy element with a two-byte offset (length 1..64, offset 1..65,535)"""
    assert 1 <= length <= 64 and 1 <= offset <= 65535
    return bytes([((length - 1) << 2) | 2]) + offset.to_bytes(2, "little")


def decode(payload):
    """the bytes of one raw stream of literals and copies (no checks: the tests' own streams)"""
    p, n, shift = 0, 0, 0
    while True:
        b = payload[p]
        p += 1
        n |= (b & 0x7F) << shift
        shift += 7
        if not b & 0x80:
            break
    out = bytearray()
    while p < len(payload):
        tag = payload[p]
        t = tag & 3
        if t == 0:
            m = tag >> 2
            k = m - 59 if m >= 60 else 0
            ln = (int.from_bytes(payload[p + 1:p + 1 + k], "little") if k else m) + 1
            out += payload[p + 1 + k:p + 1 + k + ln]
            p += 1 + k + ln
            continue
        if t == 1:
            ln, off, p = 4 + ((tag >> 2) & 7), ((tag >> 5) << 8) | payload[p + 1], p + 2
        elif t == 2:
            ln, off, p = (tag >> 2) + 1, int.from_bytes(payload[p + 1:p + 3], "little"), p + 3
        else:
            ln, off, p = (tag >> 2) + 1, int.from_bytes(payload[p + 1:p + 5], "little"), p + 5
        for _ in range(ln):
            out.append(out[-off])
    assert len(out) == n
    return bytes(out)


def repeated(pattern, total):
    """the raw stream of `pattern` repeated to `total` bytes: one literal, then copies"""
    assert total > len(pattern)
    s, left = cm.varint(total) + cc.literal(pattern), total - len(pattern)
    while left:
        k = min(left, 64)
        s += copy2(k, len(pattern))
        left -= k
    return s


def back_copy_chunk(seed):
    """a raw stream of 131,072 bytes whose second block is all copies that reach into
    its first: 65,536 literal bytes, then 1,024 copies of 64 bytes at offset 65,535"""
    return cm.varint(2 * BLOCK) + cc.literal(cc.content(BLOCK, seed)) + copy2(64, 65535) * 1024


def container(fmt, payloads, lens, header_before=()):
    """one Hadoop block of all the chunks, or a snappy-java stream with the header again
    in front of the chunks named in header_before"""
    if fmt == cm.HADOOP:
        return cm.hadoop_block(sum(lens), payloads)
    s = cm.header()
    for i, p in enumerate(payloads):
        if i in header_before:
            s += cm.header()
        s += cm.chunk(p)
    return s


def _own_hadoop_five():
    p = [cc.content(n, 40 + n) for n in (1, 17, 64, 200, 3)]
    return cm.HADOOP, container(cm.HADOOP, [cc.stored(x) for x in p], [len(x) for x in p]), b"".join(p)


def _own_hadoop_copies():
    streams = [repeated(b"abcdefg", 120), cc.stored(cc.content(5, 51)), repeated(b"xy", 60)]
    raws = [decode(s) for s in streams]
    s = cm.hadoop_block(125, streams[:2]) + cm.be32(0) + cm.hadoop_block(60, streams[2:])
    return cm.HADOOP, s, b"".join(raws)


def _own_xerial_five():
    p = [cc.content(n, 60 + n) for n in (200, 0, 1, 16, 33)]
    return cm.XERIAL, container(cm.XERIAL, [cc.stored(x) for x in p], [len(x) for x in p], header_before=(3,)), \
        b"".join(p)


def _own_xerial_copies():
    streams = [repeated(b"0123456789abcdef", 130), repeated(b"q", 70), cc.stored(cc.content(9, 52))]
    return cm.XERIAL, container(cm.XERIAL, streams, None), b"".join(decode(s) for s in streams)


def _abc(fmt):
    return lambda: (fmt, cc.abc_hadoop() if fmt == cm.HADOOP else cc.abc_xerial(), b"abc")


# name -> (format, container, plain bytes): five small containers per format, chunks of 0 to 300 bytes
SLICE = {
    "hadoop: raw_len 0 blocks at the start, in the middle and at the end": cc.FOREIGN[
        "hadoop: raw_len 0 blocks at the start, in the middle and at the end"],
    "hadoop: chunks of no bytes inside a block": cc.FOREIGN["hadoop: chunks of no bytes inside a block"],
    "hadoop: three chunks of one byte in two blocks": _abc(cm.HADOOP),
    "hadoop: one block of five chunks (1, 17, 64, 200, 3)": _own_hadoop_five,
    "hadoop: chunks of copies, an empty block between": _own_hadoop_copies,
    "xerial: the header again mid-stream and at the end": cc.FOREIGN["xerial: the header again mid-stream and at the end"],
    "xerial: version 2, compatible_version 1": cc.FOREIGN["xerial: version 2, compatible_version 1"],
    "xerial: three chunks of one byte": _abc(cm.XERIAL),
    "xerial: chunks of 200, 0, 1, 16, 33, the header again inside": _own_xerial_five,
    "xerial: chunks of copies": _own_xerial_copies,
}

LONG_SIZES = [300, 65537, 131072, 65536, 196609, 77]   # chunk 2 is back_copy_chunk


def long_case(fmt, compress=cc.stored, content=cc.content):
    """(container, plain bytes): chunks of LONG_SIZES bytes, chunk 2 the foreign one whose
    second block copies from its first; in Hadoop one block of six chunks, in snappy-java
    the header again in front of chunks 2 and 5.  content(n, seed) -> the plain bytes of
    a chunk, compress(raw) -> its raw stream."""
    raws, streams = [], []
    for k, n in enumerate(LONG_SIZES):
        if k == 2:
            s = back_copy_chunk(70)
            raws.append(decode(s))
        else:
            raws.append(content(n, 70 + k))
            s = compress(raws[-1])
        streams.append(s)
    return container(fmt, streams, LONG_SIZES, header_before=(2, 5)), b"".join(raws)


def long_spans(outp):
    """every long chunk as an interior, first-edge, last-edge, single-edge and
    single-whole unit; ends on a chunk's last byte and on the next chunk's first"""
    spans = []
    for u in (1, 2, 3, 4):
        b0, size = outp[u]
        b1 = b0 + size
        spans += [(b0 - 1, b1 + 1), (b0 + 1, b1 + 1), (b0 - 1, b1 - 1), (b0 + size // 3, b1 - size // 4), (b0, b1),
                  (b0 - 5, b1), (b0 - 5, b1 + 1), (b0 + BLOCK - 1, b0 + BLOCK + 1)]
    spans.append((1, outp[-1][0] + outp[-1][1] - 1))
    return spans


def lay_out(spans):
    """[(start, length, out_offset)] back to back with gaps of 1..16 sentinel bytes, range
    k at out_offset = start + k (mod 16): every residue of the output against the start.
    -> (ranges, out_bytes)"""
    ranges, oo = [], 3
    for k, (a, b) in enumerate(spans):
        oo += 1 + (a + k - (oo + 1)) % 16
        ranges.append((a, b - a, oo))
        oo += b - a
    return ranges, oo + 5


def every_slice(n):
    """every (start, length) of n decoded bytes, length 0 at both ends included"""
    return [(a, b) for a in range(n + 1) for b in range(a, n + 1) if b > a or a in (0, n)]


def slice_case(name):
    fmt, stream, raw = SLICE[name]()
    comp, outp, total = crm.tables(stream, fmt)
    assert total == len(raw)
    ranges, out_bytes = lay_out(every_slice(total))
    return fmt, stream, raw, comp, outp, ranges, out_bytes


def expected(raw, ranges, out_bytes, accepted=None):
    """the output buffer: the accepted ranges' slices of raw, the sentinel elsewhere"""
    buf = bytearray([SENT]) * max(out_bytes, 1)
    for i, (a, ln, oo) in enumerate(ranges):
        if accepted is None or i in accepted:
            buf[oo:oo + ln] = raw[a:a + ln]
    return bytes(buf)


def planned(stream, comp, outp, ranges, out_bytes, accepted):
    """the output buffer by the tables as they are given, right or not: every unit of an
    accepted range puts bytes [lo, hi) of what its table entry's payload decodes to at
    land + [lo, hi); the sentinel elsewhere"""
    buf = bytearray([SENT]) * max(out_bytes, 1)
    _, units = crm.plan(outp, ranges, out_bytes)
    for u, land, i, lo, hi, edge in units:
        if i in accepted and hi not in (0, crm.BAD):
            at, c = comp[u]
            buf[land + lo:land + hi] = decode(stream[at:at + c])[lo:hi]
    return bytes(buf)


def uniform(fmt, count, size, seed):
    """count stored chunks of `size` bytes -> (container, plain bytes)"""
    p = [cc.content(size, seed + i) for i in range(count)]
    return container(fmt, [cc.stored(x) for x in p], [size] * count), b"".join(p)


def staging_spans(total, count, seed):
    """`count` seeded ranges inside [1, total - 1) of a container of 4,096-byte chunks:
    inside one chunk, or across one to three boundaries"""
    rnd = random.Random(seed)
    spans = []
    for _ in range(count):
        a = rnd.randrange(1, total - 2)
        spans.append((a, min(a + rnd.choice([1, 100, 4096, 5000, 9000, 13000]), total - 1)))
    return spans

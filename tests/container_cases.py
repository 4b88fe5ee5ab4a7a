"""Hand-built container streams shared by test_container_model.py (CPU: the
model's tables and statuses, asserted literally), test_container_walk_check.py
(CPU: the C walk rule under a sanitizer) and test_container.py (GPU).  Every
payload here is written by hand as literal elements, so nothing but the model
is needed to build them."""
import random

import container_model as cm


def content(n: int, seed: int) -> bytes:
    return random.Random(seed).randbytes(n)


def literal(raw: bytes) -> bytes:
    """One literal element holding raw (len >= 1)."""
    k = len(raw) - 1
    if k < 60:
        return bytes([k << 2]) + raw
    for extra in (1, 2, 3, 4):
        if k < 1 << (8 * extra):
            return bytes([(59 + extra) << 2]) + k.to_bytes(extra, "little") + raw
    raise ValueError(len(raw))


def stored(raw: bytes) -> bytes:
    """The raw stream of raw as one long literal (00 for no bytes)."""
    return cm.varint(len(raw)) + (literal(raw) if raw else b"")


HELLO = bytes.fromhex("05 10 68 65 6c 6c 6f")  # the raw stream of b"hello"
HELLO_HADOOP = bytes.fromhex("00 00 00 05 00 00 00 07 05 10 68 65 6c 6c 6f")
HELLO_XERIAL = bytes.fromhex("82 53 4e 41 50 50 59 00 00 00 00 01 00 00 00 01 00 00 00 07 05 10 68 65 6c 6c 6f")


def _three_chunks():
    p = [content(1, 1), content(65537, 2), content(300000, 3)]
    return cm.HADOOP, cm.hadoop_block(365538, [stored(x) for x in p]), b"".join(p)


def _empty_blocks():
    p = [content(100, 4), content(50, 5)]
    s = cm.be32(0) + cm.hadoop_block(100, [stored(p[0])]) + cm.be32(0) + cm.be32(0) + \
        cm.hadoop_block(50, [stored(p[1])]) + cm.be32(0)
    return cm.HADOOP, s, b"".join(p)


def _zero_chunks():
    p = [content(10, 6), content(20, 7)]
    return cm.HADOOP, cm.hadoop_block(30, [stored(b""), stored(p[0]), stored(b""), stored(p[1])]), b"".join(p)


def _repeated_header():
    p = [content(70, 8), content(300, 9)]
    s = cm.header() + cm.chunk(stored(p[0])) + cm.header() + cm.chunk(stored(p[1])) + cm.header()
    return cm.XERIAL, s, b"".join(p)


def _version_two():
    p = content(40, 10)
    return cm.XERIAL, cm.header(2, 1) + cm.chunk(stored(p)), p


def _stored_hadoop():
    p = content(100000, 11)
    return cm.HADOOP, cm.hadoop_block(100000, [stored(p)]), p


def _stored_xerial():
    p = content(100000, 12)
    return cm.XERIAL, cm.header() + cm.chunk(stored(p)) + cm.chunk(stored(b"")), p


# name -> (format, stream, decoded bytes)
FOREIGN = {
    "hadoop: a block of three chunks (1; 65,537; 300,000)": _three_chunks,
    "hadoop: raw_len 0 blocks at the start, in the middle and at the end": _empty_blocks,
    "hadoop: chunks of no bytes inside a block": _zero_chunks,
    "xerial: the header again mid-stream and at the end": _repeated_header,
    "xerial: version 2, compatible_version 1": _version_two,
    "hadoop: a stored-only chunk": _stored_hadoop,
    "xerial: a stored-only chunk and an empty one": _stored_xerial,
}

# the tables the walk must give, worked out by hand from the layouts above:
# name -> ([(payload offset, comp_len) ...], [(output offset, length) ...])
#   stored(1) = 01 00 xx: 3 bytes; stored(65,537) = 3 + 4 + 65,537; stored(300,000) = 3 + 4 + 300,000
FOREIGN_TABLES = {
    "hadoop: a block of three chunks (1; 65,537; 300,000)": (
        [(8, 3), (15, 65544), (65563, 300007)], [(0, 1), (1, 65537), (65538, 300000)]),
    #   00000000 | 00000064 00000066 (01 + 60<<2,63 + 100) | 0 | 0 | 00000032 00000034 (01 + 49<<2 + 50) | 0
    "hadoop: raw_len 0 blocks at the start, in the middle and at the end": (
        [(12, 103), (131, 52)], [(0, 100), (100, 50)]),
    #   0000001e | 00000001 00 | 0000000c (0a 24 + 10) | 00000001 00 | 00000016 (14 4c + 20)
    "hadoop: chunks of no bytes inside a block": (
        [(8, 1), (13, 12), (29, 1), (34, 22)], [(0, 0), (0, 10), (10, 0), (10, 20)]),
    #   header | 00000049 (46 f0 45 + 70) | header | 00000130 (ac 02 f4 2b 01 + 300) | header
    "xerial: the header again mid-stream and at the end": (
        [(20, 73), (113, 305)], [(0, 70), (70, 300)]),
    "xerial: version 2, compatible_version 1": ([(20, 42)], [(0, 40)]),
    #   stored(100,000) = 3 (a0 8d 06) + 4 (f8 9f 86 01) + 100,000
    "hadoop: a stored-only chunk": ([(8, 100007)], [(0, 100000)]),
    "xerial: a stored-only chunk and an empty one": ([(20, 100007), (100031, 1)], [(0, 100000), (100000, 0)]),
}


def abc_hadoop() -> bytes:
    """Three chunks of one byte each, two blocks: the container whose prefixes the error tests walk."""
    return cm.hadoop_block(2, [stored(b"a"), stored(b"b")]) + cm.hadoop_block(1, [stored(b"c")])


def abc_xerial() -> bytes:
    return cm.header() + b"".join(cm.chunk(stored(x)) for x in (b"a", b"b", b"c"))


def two_byte_varint() -> bytes:
    """An empty block, then a chunk whose preamble has two bytes."""
    return cm.be32(0) + cm.hadoop_block(130, [stored(content(130, 13))])


def walk_error_cases():
    """name -> (format, stream, status): one case per line of the walk rule."""
    a, x = abc_hadoop(), abc_xerial()
    big = cm.varint((1 << 30) + 1)
    return {
        "hadoop: comp_len 0": (cm.HADOOP, cm.be32(5) + cm.be32(0) + b"\x00", cm.ERR_HEADER),
        "xerial: comp_len 0": (cm.XERIAL, x + cm.be32(0), cm.ERR_HEADER),
        "hadoop: a chunk one byte past the end": (cm.HADOOP, a[:-1], cm.ERR_TRUNCATED),
        "xerial: a chunk 2^32 - 1 past the end": (cm.XERIAL, x + b"\xff\xff\xff\xff\x01", cm.ERR_TRUNCATED),
        "hadoop: a varint cut by its chunk": (cm.HADOOP, cm.be32(200) + cm.chunk(b"\xc8"), cm.ERR_HEADER),
        "xerial: a varint of six bytes": (cm.XERIAL, x + cm.chunk(b"\x80\x80\x80\x80\x80\x00"), cm.ERR_HEADER),
        "hadoop: a preamble of 2^30 + 1": (cm.HADOOP, cm.be32(0xFFFFFFFF) + cm.chunk(big + b"\x00"), cm.ERR_UNSUPPORTED),
        "xerial: a preamble of 2^30 + 1": (cm.XERIAL, x + cm.chunk(big + b"\x00"), cm.ERR_UNSUPPORTED),
        "hadoop: a chunk longer than its block has left": (
            cm.HADOOP, cm.hadoop_block(3, [stored(b"ab"), stored(b"cd")]), cm.ERR_OVERRUN),
        "hadoop: the input ends inside a block": (cm.HADOOP, cm.hadoop_block(3, [stored(b"ab")]), cm.ERR_TRUNCATED),
        "hadoop: three bytes where a block begins": (cm.HADOOP, a + b"\x00\x00\x00", cm.ERR_TRUNCATED),
        "xerial: wrong magic": (cm.XERIAL, x[:6] + b"\x58" + x[7:], cm.ERR_HEADER),
        "xerial: no bytes at all": (cm.XERIAL, b"", cm.ERR_HEADER),
        "xerial: compatible_version 2": (cm.XERIAL, cm.header(1, 2) + x[16:], cm.ERR_UNSUPPORTED),
        "xerial: a header of 15 bytes": (cm.XERIAL, x[:15], cm.ERR_TRUNCATED),
        "xerial: a second header with a wrong byte": (cm.XERIAL, x + cm.MAGIC[:5] + b"\x00" * 11, cm.ERR_HEADER),
        "xerial: a second header cut short": (cm.XERIAL, x + cm.header()[:9], cm.ERR_TRUNCATED),
    }

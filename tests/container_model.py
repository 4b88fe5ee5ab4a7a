"""A Python model of the two length-prefixed Snappy containers, kept with the
tests: the block stream of Hadoop's SnappyCodec and the chunk stream of
snappy-java's SnappyOutputStream.  Written from the description of the formats
in DESIGN.md 7.5 (neither implementation is at hand); it knows nothing of the
library.  test_container_model.py pins it to hand-written vectors.

All integers are big-endian u32.  A raw stream is varint(L) followed by
elements.

  Hadoop       blocks: BE32 raw_len, then chunks BE32 comp_len | raw stream until
               the chunks' decoded lengths add up to raw_len (0: no chunk)
  snappy-java  82 53 4e 41 50 50 59 00, BE32 version, BE32 compatible_version,
               then chunks BE32 comp_len | raw stream; the header may stand
               again at any chunk boundary
"""
import struct

HADOOP, XERIAL = 0, 1
MAGIC = bytes.fromhex("82534e4150505900")
CHUNK_MAX = 1 << 30

OK, ERR_HEADER, ERR_TRUNCATED, ERR_OVERRUN, ERR_UNSUPPORTED = 0, -2, -3, -5, -9


def be32(v: int) -> bytes:
    return struct.pack(">I", v)


def varint(n: int) -> bytes:
    out = bytearray()
    while n >= 128:
        out.append((n & 0x7F) | 0x80)
        n >>= 7
    out.append(n)
    return bytes(out)


def header(version: int = 1, compatible: int = 1) -> bytes:
    return MAGIC + be32(version) + be32(compatible)


def chunk(payload: bytes) -> bytes:
    return be32(len(payload)) + bytes(payload)


def hadoop_block(raw_len: int, payloads) -> bytes:
    """One block holding the given raw streams as its chunks."""
    return be32(raw_len) + b"".join(chunk(p) for p in payloads)


def wrap(pieces, payloads, format, with_header=True) -> bytes:
    """The container a compressor writes for `pieces` (the input cut into
    blocks) whose raw streams are `payloads`: one chunk per piece, in Hadoop
    one block per chunk."""
    assert len(pieces) == len(payloads)
    if format == HADOOP:
        return b"".join(hadoop_block(len(r), [p]) for r, p in zip(pieces, payloads))
    return (header() if with_header else b"") + b"".join(chunk(p) for p in payloads)


def _chunk(data, p, end, left):
    """The chunk rule at p: (status, payload offset, comp_len, decoded length)."""
    if end - p < 4:
        return ERR_TRUNCATED, 0, 0, 0
    c, = struct.unpack_from(">I", data, p)
    if c == 0:
        return ERR_HEADER, 0, 0, 0
    if p + 4 + c > end:
        return ERR_TRUNCATED, 0, 0, 0
    length, shift, done = 0, 0, False
    for b in data[p + 4:p + 4 + min(c, 5)]:
        length |= (b & 0x7F) << shift
        shift += 7
        if not b & 0x80:
            done = True
            break
    if not done:
        return ERR_HEADER, 0, 0, 0
    if length > CHUNK_MAX:
        return ERR_UNSUPPORTED, 0, 0, 0
    if left is not None and length > left:
        return ERR_OVERRUN, 0, 0, 0
    return OK, p + 4, c, length


def walk(data: bytes, format):
    """(status, [(payload offset, comp_len) ...], [(output offset, length) ...],
    decoded bytes): the strict walk; the tables and the count hold the chunks
    in front of the first failure."""
    data = bytes(data)
    end, p, o = len(data), 0, 0
    comp, outp = [], []
    if format == HADOOP:
        left = 0
        while p < end:
            if left == 0:
                if end - p < 4:
                    return ERR_TRUNCATED, comp, outp, o
                left, = struct.unpack_from(">I", data, p)
                p += 4
                continue
            st, at, c, length = _chunk(data, p, end, left)
            if st != OK:
                return st, comp, outp, o
            comp.append((at, c))
            outp.append((o, length))
            o += length
            left -= length
            p = at + c
        return (ERR_TRUNCATED if left else OK), comp, outp, o
    first = True
    while first or p < end:
        if first or data[p:p + 4] == MAGIC[:4]:
            have = data[p:p + 8]
            if not have or have != MAGIC[:len(have)]:
                return ERR_HEADER, comp, outp, o
            if end - p < 16:
                return ERR_TRUNCATED, comp, outp, o
            if struct.unpack_from(">I", data, p + 12)[0] > 1:
                return ERR_UNSUPPORTED, comp, outp, o
            p += 16
            first = False
            continue
        st, at, c, length = _chunk(data, p, end, None)
        if st != OK:
            return st, comp, outp, o
        comp.append((at, c))
        outp.append((o, length))
        o += length
        p = at + c
    return OK, comp, outp, o


def unwrap(data: bytes, format, decompress) -> bytes:
    """Strict reader: decompress(raw stream) -> bytes for every chunk.  Raises
    ValueError(status) on a malformed container."""
    st, comp, outp, n = walk(data, format)
    if st != OK:
        raise ValueError(st)
    out = bytearray()
    for (at, c), (o, length) in zip(comp, outp):
        raw = decompress(bytes(data[at:at + c])) if length else b""
        if len(raw) != length or o != len(out):
            raise ValueError(ERR_HEADER)
        out += raw
    assert len(out) == n
    return bytes(out)

"""A Python model of the Snappy framing format (framing_format.txt of
google/snappy), kept with the tests: a table CRC-32C, the mask, a writer that
can emit every chunk type from given payloads, and a strict reader.  It knows
nothing of the library; test_frame_model.py pins it to published values."""
import struct

IDENTIFIER = bytes.fromhex("ff060000734e61507059")
CHUNK_MAX = 65536

OK, ERR_HEADER, ERR_TRUNCATED, ERR_OVERRUN, ERR_UNSUPPORTED, ERR_CHECKSUM = 0, -2, -3, -5, -9, -12

_POLY = 0x82F63B78
_TABLE = []
for _i in range(256):
    _c = _i
    for _ in range(8):
        _c = (_c >> 1) ^ (_POLY if _c & 1 else 0)
    _TABLE.append(_c)


def crc32c(data: bytes) -> int:
    c = 0xFFFFFFFF
    for b in bytes(data):
        c = _TABLE[(c ^ b) & 0xFF] ^ (c >> 8)
    return c ^ 0xFFFFFFFF


def mask(c: int) -> int:
    return (((c >> 15) | (c << 17)) + 0xA282EAD8) & 0xFFFFFFFF


def varint(n: int) -> bytes:
    out = bytearray()
    while n >= 128:
        out.append((n & 0x7F) | 0x80)
        n >>= 7
    out.append(n)
    return bytes(out)


def chunk(kind: int, body: bytes) -> bytes:
    assert len(body) < 1 << 24
    return bytes([kind]) + struct.pack("<I", len(body))[:3] + body


def compressed(raw: bytes, payload: bytes, crc=None) -> bytes:
    """A type-00 chunk: payload = a raw Snappy stream of raw."""
    c = mask(crc32c(raw)) if crc is None else crc
    return chunk(0x00, struct.pack("<I", c) + payload)


def stored(raw: bytes, crc=None) -> bytes:
    """A type-01 chunk."""
    c = mask(crc32c(raw)) if crc is None else crc
    return chunk(0x01, struct.pack("<I", c) + raw)


def padding(n: int) -> bytes:
    return chunk(0xFE, bytes(n))


def skippable(kind: int, body: bytes) -> bytes:
    assert 0x80 <= kind <= 0xFD
    return chunk(kind, body)


def frame_streams(a: bytes, payload: bytes, offs, identifier=True) -> bytes:
    """The framing of a's 65,536-byte pieces whose raw streams lie in payload
    at offs (oracle.compress_streams(a, 65536)): compressed chunks only."""
    out = bytearray(IDENTIFIER if identifier else b"")
    for u in range(len(offs) - 1):
        out += compressed(a[u * CHUNK_MAX:(u + 1) * CHUNK_MAX], bytes(payload[int(offs[u]):int(offs[u + 1])]))
    return bytes(out)


def chunk_table(stream: bytes):
    """(status, [positions of the data chunk headers ..., len(stream)], decoded
    bytes): the strict walk, by the rules of the format."""
    pos, table, total, first = 0, [], 0, True
    n = len(stream)
    while pos < n:
        if n - pos < 4:
            return ERR_TRUNCATED, table, total
        kind = stream[pos]
        ln = stream[pos + 1] | stream[pos + 2] << 8 | stream[pos + 3] << 16
        if first and kind != 0xFF:
            return ERR_HEADER, table, total
        first = False
        if kind == 0xFF:
            if ln != 6:
                return ERR_HEADER, table, total
            if n - pos < 10:
                return ERR_TRUNCATED, table, total
            if stream[pos:pos + 10] != IDENTIFIER:
                return ERR_HEADER, table, total
        elif 0x02 <= kind <= 0x7F:
            return ERR_UNSUPPORTED, table, total
        elif kind >= 0x80:
            if n - pos - 4 < ln:
                return ERR_TRUNCATED, table, total
        else:
            if ln < 4:
                return ERR_HEADER, table, total
            if n - pos - 4 < ln:
                return ERR_TRUNCATED, table, total
            d = ln - 4
            if kind == 0x00:
                d, shift, done = 0, 0, False
                for b in stream[pos + 8:pos + 8 + min(ln - 4, 5)]:
                    d |= (b & 0x7F) << shift
                    shift += 7
                    if not b & 0x80:
                        done = True
                        break
                if not done:
                    return ERR_HEADER, table, total
            if d > CHUNK_MAX:
                return ERR_OVERRUN, table, total
            table.append(pos)
            total += d
        pos += 4 + ln
    return OK, table + [n], total


def read(stream: bytes, decompress) -> bytes:
    """Strict reader: decompress(payload) -> raw bytes for type-00 chunks.
    Raises ValueError(status) on a malformed stream or a CRC mismatch."""
    st, table, _ = chunk_table(stream)
    if st != OK:
        raise ValueError(st)
    out = bytearray()
    for pos in table[:-1]:
        ln = stream[pos + 1] | stream[pos + 2] << 8 | stream[pos + 3] << 16
        crc, = struct.unpack_from("<I", stream, pos + 4)
        body = stream[pos + 8:pos + 4 + ln]
        raw = body if stream[pos] == 0x01 else decompress(body)
        if mask(crc32c(raw)) != crc:
            raise ValueError(ERR_CHECKSUM)
        out += raw
    return bytes(out)

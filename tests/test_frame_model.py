"""CPU: the framing-format model (tests/frame_model.py) against published
CRC-32C values and the specification's constants, and the library's host
chunk walk (snappy_frame_uncompressed_length, which launches no kernel)
against the model on well-formed and malformed streams."""
import struct

import pytest

import frame_model as fm
import oracle
import snappy_amd

# RFC 3720 B.4 and the usual check value; the masked column by the format's formula
VECTORS = [
    (b"123456789", 0xE3069283, 0xC78AB0E5),
    (bytes(32), 0x8A9136AA, None),
    (b"\xff" * 32, 0x62A8AB43, None),
    (bytes(range(32)), 0x46DD794E, None),
    (bytes(range(31, -1, -1)), 0x113FDB5C, None),
    (b"", 0x00000000, 0xA282EAD8),
    (b"a", 0xC1D04330, 0x28E46E78),
]


@pytest.mark.parametrize("data,crc,masked", VECTORS)
def test_model_crc32c_published_vectors(data, crc, masked):
    assert fm.crc32c(data) == crc
    if masked is not None:
        assert fm.mask(crc) == masked


def test_identifier_bytes():
    assert fm.IDENTIFIER == b"\xff\x06\x00\x00sNaPpY" == snappy_amd.FRAME_IDENTIFIER
    assert len(fm.IDENTIFIER) == 10
    assert snappy_amd.ERR_CHECKSUM == -12 == fm.ERR_CHECKSUM


def test_max_frame_output_formula():
    for n in (0, 1, 65535, 65536, 65537, 5 * 65536 + 17, 1 << 30):
        units = (n + 65535) // 65536
        assert snappy_amd.max_frame_output(n) == 10 + 8 * units + snappy_amd.Codec.max_output(n, 65536, snappy_amd.STREAMS)


def _walk(stream):
    v = snappy_amd.ctypes.c_uint64(0)
    p, n, keep = snappy_amd._buf(stream)
    rc = snappy_amd.lib().snappy_frame_uncompressed_length(p, n, snappy_amd.ctypes.byref(v))
    return rc, v.value


def _pieces(sizes, seed=7):
    import datagen
    a = datagen.make("T", sum(sizes), seed).tobytes()
    out, at = [], 0
    for s in sizes:
        out.append(a[at:at + s])
        at += s
    return out


def _c(raw):
    return fm.compressed(raw, oracle.compress(raw) if raw else fm.varint(0))


GOOD = {
    "identifier only": lambda: (fm.IDENTIFIER, 0),
    "empty": lambda: (b"", 0),
    "compressed": lambda: (fm.IDENTIFIER + b"".join(_c(p) for p in _pieces([65536, 65536, 1234])), 2 * 65536 + 1234),
    "stored": lambda: (fm.IDENTIFIER + b"".join(fm.stored(p) for p in _pieces([1, 65536])), 65537),
    "mixed, padding, skippable, identifiers": lambda: (
        fm.IDENTIFIER + _c(_pieces([4096])[0]) + fm.padding(0) + fm.stored(b"xyz") + fm.padding(7) +
        fm.skippable(0x80, b"hello") + fm.IDENTIFIER + _c(_pieces([100])[0]) + fm.IDENTIFIER, 4096 + 3 + 100),
    "zero-length data chunks": lambda: (fm.IDENTIFIER + _c(b"") + fm.stored(b"") + _c(b""), 0),
}


@pytest.mark.parametrize("name", list(GOOD))
def test_host_walk_accepts_what_the_model_writes(name):
    stream, n = GOOD[name]()
    st, table, total = fm.chunk_table(stream)
    assert st == fm.OK and total == n
    assert _walk(stream) == (0, n)
    assert snappy_amd.frame_uncompressed_length(stream) == n


def _bad_streams():
    p = _pieces([3000, 500])
    good = fm.IDENTIFIER + _c(p[0]) + fm.stored(p[1])
    second = len(fm.IDENTIFIER) + len(_c(p[0]))
    big = bytes(65537)
    return {
        "no identifier": (good[10:], fm.ERR_HEADER),
        "identifier with a wrong byte": (good[:9] + b"X" + good[10:], fm.ERR_HEADER),
        "identifier of another length": (b"\xff\x05\x00\x00sNaPp" + good[10:], fm.ERR_HEADER),
        "a later ff chunk that is not the identifier": (good + b"\xff\x06\x00\x00sNaPpZ", fm.ERR_HEADER),
        "type 02": (good + fm.chunk(0x02, b"abcdef"), fm.ERR_UNSUPPORTED),
        "type 7f": (good + fm.chunk(0x7F, b""), fm.ERR_UNSUPPORTED),
        "one byte past the end": (good[:-1], fm.ERR_TRUNCATED),
        "2^24 - 1 past the end": (good + b"\x01\xff\xff\xff", fm.ERR_TRUNCATED),
        "cut inside a chunk header": (good[:second + 2], fm.ERR_TRUNCATED),
        "cut inside the identifier": (fm.IDENTIFIER[:7], fm.ERR_TRUNCATED),
        "skippable chunk past the end": (good + b"\x80\x05\x00\x00abcd", fm.ERR_TRUNCATED),
        "len = 3": (good + b"\x01\x03\x00\x00abc", fm.ERR_HEADER),
        "compressed chunk without a preamble": (good + fm.chunk(0x00, bytes(4)), fm.ERR_HEADER),
        "compressed chunk with an unterminated preamble": (good + fm.chunk(0x00, bytes(4) + b"\x80\x80\x80\x80\x80\x01"),
                                                           fm.ERR_HEADER),
        "compressed chunk that declares 65,537": (good + fm.chunk(0x00, bytes(4) + fm.varint(65537) + b"\x00a"),
                                                  fm.ERR_OVERRUN),
        "stored chunk of 65,537": (good + fm.stored(big), fm.ERR_OVERRUN),
    }


BAD = _bad_streams()


@pytest.mark.parametrize("name", list(BAD))
def test_host_walk_refuses_each_malformed_case(name):
    stream, want = BAD[name]
    assert fm.chunk_table(stream)[0] == want  # the model agrees that this is the error
    assert _walk(stream)[0] == want
    with pytest.raises(snappy_amd.SnappyError) as e:
        snappy_amd.frame_uncompressed_length(stream)
    assert e.value.code == want


def mutated_streams(count, seed):
    """Well-formed streams of small chunks of every type with one byte changed,
    a cut, or both: (stream, model status, model total)."""
    import random
    rng = random.Random(seed)
    raw = _pieces([40])[0]
    parts = [_c(raw), fm.stored(raw), fm.padding(3), fm.skippable(0x90, b"xy"), fm.IDENTIFIER, _c(b""),
             fm.chunk(0x00, bytes(4) + fm.varint(65536) + b"\x00"), fm.chunk(0x01, b"abc"), fm.chunk(0x05, b"")]
    out = []
    for _ in range(count):
        s = bytearray(fm.IDENTIFIER + b"".join(rng.choice(parts[:7] if rng.random() < 0.8 else parts)
                                               for _ in range(rng.randrange(5))))
        if rng.random() < 0.5:
            s[rng.randrange(len(s))] ^= 1 << rng.randrange(8)
        if rng.random() < 0.3:
            del s[rng.randrange(len(s) + 1):]
        st, _, total = fm.chunk_table(bytes(s))
        out.append((bytes(s), st, total))
    return out


def test_host_walk_follows_the_model_on_mutated_streams():
    seen = set()
    for stream, st, total in mutated_streams(400, 2024):
        rc, n = _walk(stream)
        assert rc == st, (stream.hex(), rc, st)
        if st == fm.OK:
            assert n == total
        seen.add(st)
    assert {fm.OK, fm.ERR_HEADER, fm.ERR_TRUNCATED, fm.ERR_UNSUPPORTED} <= seen


def test_model_reader_round_trip_and_checksum():
    p = _pieces([65536, 100])
    stream = fm.IDENTIFIER + _c(p[0]) + fm.stored(p[1])
    assert fm.read(stream, oracle.decompress) == p[0] + p[1]
    bad = bytearray(stream)
    bad[10 + 4] ^= 1  # the first chunk's stored CRC
    with pytest.raises(ValueError) as e:
        fm.read(bytes(bad), oracle.decompress)
    assert e.value.args[0] == fm.ERR_CHECKSUM
    assert struct.unpack_from("<I", stream, 14)[0] == fm.mask(fm.crc32c(p[0]))

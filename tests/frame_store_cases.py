"""The model of the framed compressor with a chunk size and the store rule, and
the inputs the tests of it share (test_frame_store_model.py on the CPU,
test_frame_store.py on the GPU).

The model knows nothing of the library: the pieces' raw streams come from
oracle.compress_streams(a, chunk), the chunks from frame_model, and the rule is
written out here -- with FRAME_STORE a chunk of R input bytes whose raw stream
(preamble included) has P bytes is stored iff P >= R - R // 8."""
import functools

import numpy as np

import datagen
import frame_model as fm
import oracle

FRAME_NO_IDENTIFIER, FRAME_STORE = 1, 2
PLANT_R = [17, 64, 100, 1000, 4096, 32768, 32769, 65535, 65536]


def is_stored(R: int, P: int) -> bool:
    return P >= R - R // 8


def model(a: bytes, chunk: int, store: bool, identifier: bool = True):
    """-> (stream, chunk table, one 'S' or 'C' per chunk)"""
    a = bytes(a)
    out = bytearray(fm.IDENTIFIER if identifier else b"")
    table, kinds = [], ""
    if a:
        payload, offs = oracle.compress_streams(np.frombuffer(a, dtype=np.uint8), chunk)
        for u in range(len(offs) - 1):
            raw = a[u * chunk:(u + 1) * chunk]
            p = bytes(payload[int(offs[u]):int(offs[u + 1])])
            table.append(len(out))
            if store and is_stored(len(raw), len(p)):
                out += fm.stored(raw)
                kinds += "S"
            else:
                out += fm.compressed(raw, p)
                kinds += "C"
    table.append(len(out))
    return bytes(out), table, kinds


def stream_bytes(piece: bytes) -> int:
    """P of one piece: the bytes of its raw stream, preamble included"""
    _, offs = oracle.compress_streams(np.frombuffer(piece, dtype=np.uint8), len(piece))
    return int(offs[1])


@functools.lru_cache(maxsize=None)
def noise(n: int = 65536) -> bytes:
    return np.random.default_rng(7).integers(0, 256, size=n, dtype=np.uint8).tobytes()


@functools.lru_cache(maxsize=None)
def plants(R: int):
    """{d: piece} for d = P - (R - R // 8) in -1, 0, +1 (those found), from the family
    zeros(z) ++ noise(R - z) with z within 80 of (R / 8) / (1 - 3 / 64): a run of
    zeros costs about 3 bytes per 64, so that z puts P at the threshold"""
    z0 = int(round((R / 8) / (1 - 3 / 64)))
    found = {}
    for z in range(max(z0 - 80, 0), min(z0 + 80, R) + 1):
        piece = bytes(z) + noise()[:R - z]
        d = stream_bytes(piece) - (R - R // 8)
        if d in (-1, 0, 1) and d not in found:
            found[d] = piece
    return found


def text(n: int, seed: int = 31) -> bytes:
    return datagen.make("T", n, seed).tobytes()


def rand(n: int, seed: int = 32) -> bytes:
    return datagen.make("R", n, seed).tobytes()


@functools.lru_cache(maxsize=None)
def mixed(chunk: int, pattern: str, tail: int = 0) -> bytes:
    """one chunk of text per 'C' and of noise per 'S'; tail > 0 cuts the last chunk to that length"""
    t, r = text(chunk * len(pattern)), rand(chunk * len(pattern))
    out = b"".join((t if k == "C" else r)[u * chunk:(u + 1) * chunk] for u, k in enumerate(pattern))
    return out[:len(out) - chunk + tail] if tail else out

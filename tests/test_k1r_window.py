"""K1r / K1r64 window refresh: the in-window predecessor search.

A refresh gives every lane of the 64-position window its nearest earlier lane
with the same hash (within DMAX lanes) and that lane's tag.  It can only go
wrong where such a predecessor decides a lane's candidate: short-distance
repeats among literals, at every distance around DMAX (13 in K1r, 12 in
K1r64), and across the 16-lane DPP rows.  The inputs here are dense in those:
small alphabets (4-byte repeats at all distances, hash-equal / tag-unequal
neighbours) and random bytes with planted copies from 1..20 back.  The bar is
the oracle's bytes and unit offsets, bit for bit, and the round trip."""
import functools

import numpy as np
import pytest

import oracle
import snappy_amd

TOTAL = 128 << 10
SINGLE_TAIL = 65536 + 4097  # a short last block: its hash table is smaller

INPUTS = ["alpha2", "alpha3", "alpha4", "alpha6", "plant1", "plant2"]
# (layout, chunk, bytes): K1r at two unit sizes, K1r64 with a full and a short last block
SHAPES = [("streams", 4096, TOTAL), ("streams", 32768, TOTAL), ("single", 65536, TOTAL),
          ("single", 65536, SINGLE_TAIL)]


def planted(seed: int, n: int) -> np.ndarray:
    """Random bytes with a copy of 4..12 bytes from d back about every 24 bytes,
    d cycling 1..20 (byte by byte, so d < length repeats with period d).  The
    gaps are random, so with two seeds the plants start on every lane class of
    a window (0-13, 15/16, 31/32, 47/48, 61-63)."""
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 256, n, dtype=np.uint8)
    gaps = rng.integers(8, 17, n // 8)
    lens = rng.integers(4, 13, n // 8)
    p, k = 24, 0
    while p + 12 < n:
        d = 1 + k % 20
        for i in range(int(lens[k])):
            a[p + i] = a[p + i - d]
        p += int(lens[k]) + int(gaps[k])
        k += 1
    return a


@functools.lru_cache(maxsize=None)
def make(name: str, n: int) -> np.ndarray:
    if name.startswith("alpha"):
        k = int(name[5:])
        a = np.random.default_rng(100 + k).integers(0, k, n, dtype=np.uint8)
    else:
        a = planted(int(name[5:]), n)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def want(name: str, layout: str, chunk: int, n: int):
    """The oracle's bytes (and unit offsets for streams), computed once per case."""
    a = make(name, n)
    if layout == "single":
        return oracle.compress(a.tobytes()), None
    out, offs = oracle.compress_streams(a, chunk)
    return out.tobytes(), offs.copy()


def copy_tokens(stream: bytes) -> int:
    """Number of copy elements of one snappy stream (preamble varint, then tags)."""
    i = 0
    while stream[i] & 0x80:
        i += 1
    i += 1
    copies = 0
    while i < len(stream):
        t = stream[i]
        kind = t & 3
        if kind == 0:
            ln = t >> 2
            extra = ln - 59 if ln >= 60 else 0
            if extra:
                ln = int.from_bytes(stream[i + 1:i + 1 + extra], "little")
            i += 1 + extra + ln + 1
        else:
            copies += 1
            i += (2, 3, 5)[kind - 1]
    assert i == len(stream)
    return copies


def test_oracle_round_trips_inputs():
    """No GPU: the reference of the cases below decodes what it encoded, for
    every input and shape they use."""
    for name in INPUTS:
        for layout, chunk, n in SHAPES:
            a = make(name, n)
            out, offs = want(name, layout, chunk, n)
            if layout == "single":
                assert oracle.decompress(out) == a.tobytes(), (name, layout, n)
            else:
                back = oracle.decompress_streams(np.frombuffer(out, dtype=np.uint8), offs, n, chunk)
                assert np.array_equal(back, a), (name, chunk)


@pytest.mark.gpu
@pytest.mark.parametrize("layout,chunk,n", SHAPES)
@pytest.mark.parametrize("name", INPUTS)
def test_window_predecessors(codec, name, layout, chunk, n):
    import torch
    a = make(name, n)
    lay = snappy_amd.SINGLE if layout == "single" else snappy_amd.STREAMS
    x = torch.from_numpy(np.array(a)).cuda()
    comp, offs = codec.compress_tensor(x, chunk=chunk, layout=lay)
    out, want_offs = want(name, layout, chunk, n)
    assert comp.cpu().numpy().tobytes() == out
    if want_offs is not None:
        assert np.array_equal(offs.cpu().numpy().astype(np.uint64), want_offs)
    back = codec.decompress_tensor(comp, offs, n, chunk=chunk, layout=lay)
    assert np.array_equal(back.cpu().numpy(), a)


@pytest.mark.gpu
def test_token_flush_at_refresh(codec):
    """More than 48 tokens pending when the window moves: the refresh must leave
    the round loop, flush them and resume.  Two-symbol input is all copies: a
    window of 62 positions adds up to 16 tokens, so the pending count passes 48
    every few windows, hundreds of times per 32 KiB unit."""
    import torch
    name, chunk, n = "alpha2", 32768, TOTAL
    a = make(name, n)
    out, want_offs = want(name, "streams", chunk, n)
    for u in range(n // chunk):
        unit = out[int(want_offs[u]):int(want_offs[u + 1])]
        assert copy_tokens(unit) > 20 * 49, u  # dense: at least 20 flushes per unit
    x = torch.from_numpy(np.array(a)).cuda()
    comp, offs = codec.compress_tensor(x, chunk=chunk, layout=snappy_amd.STREAMS)
    assert comp.cpu().numpy().tobytes() == out
    assert np.array_equal(offs.cpu().numpy().astype(np.uint64), want_offs)
    back = codec.decompress_tensor(comp, offs, n, chunk=chunk, layout=snappy_amd.STREAMS)
    assert np.array_equal(back.cpu().numpy(), a)

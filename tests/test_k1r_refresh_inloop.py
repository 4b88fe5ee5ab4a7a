"""K1r's window refresh inside the asm round loop.

A flush-free refresh of a 32 KiB-layout unit no longer leaves the hand-written
statement: the statement itself moves the window (its dwords, hashes, tags,
entry reads, in-window predecessors, lane data, window mask and round limit).
Each input below is dense in one way that path can go wrong:

* mixed200: random bytes with every other run of 100-400 bytes overwritten by
  three symbols.  Lane-space stretches (refreshes inside the statement)
  alternate with W-probe stretches, which reuse the hashes and the window
  position the statement left.
* sparse20: random bytes with a 6-byte copy from 1-29 back every 20-27 bytes.
  Runs of 20-31 misses push skip past 64 - DMAX inside a window: the C++ round
  that follows reads the window position (its step-2 probe mask) after the
  statement moved it.
* alpha2: two symbols, all copies.  More than 48 tokens are pending at many
  refreshes (the exit to the C++ refresh that remains), a deferred token is
  pending across the refreshes inside the statement, and runs of 64 or more
  equal bytes leave mid-round for a C++ match extension and refresh.

Chunks 300 and 1000 have hash tables of 512 and 1,024 slots (another shift);
at chunk 1000 the last unit has 72 bytes; every unit ends with a window cut by
L - 16.  The bar is the oracle's bytes and unit offsets, bit for bit, and the
round trip.  One single-layout case shows K1r64 still agrees."""
import functools

import numpy as np
import pytest

import oracle
import snappy_amd

TOTAL = 128 << 10
SINGLE_TAIL = 65536 + 4097
INPUTS = ["mixed200", "sparse20", "alpha2"]
CHUNKS = [300, 1000, 4096, 32768]


def mixed(seed: int, n: int) -> np.ndarray:
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 256, n, dtype=np.uint8)
    p, k = 0, 0
    while p < n:
        ln = int(rng.integers(100, 401))
        if k & 1:
            a[p:p + ln] = rng.integers(0, 3, len(a[p:p + ln]), dtype=np.uint8)
        p += ln
        k += 1
    return a


def sparse(seed: int, n: int) -> np.ndarray:
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 256, n, dtype=np.uint8)
    p = 32
    while p + 6 < n:
        d = int(rng.integers(1, 30))
        for i in range(6):
            a[p + i] = a[p + i - d]
        p += int(rng.integers(20, 28))
    return a


@functools.lru_cache(maxsize=None)
def make(name: str, n: int) -> np.ndarray:
    if name == "mixed200":
        a = mixed(203, n)
    elif name == "sparse20":
        a = sparse(21, n)
    else:
        a = np.random.default_rng(102).integers(0, 2, n, dtype=np.uint8)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def want(name: str, chunk: int):
    """The oracle's bytes and unit offsets, computed once per case."""
    out, offs = oracle.compress_streams(make(name, TOTAL), chunk)
    return out.tobytes(), offs.copy()


def elements(stream: bytes):
    """(literal lengths, number of copies) of one snappy stream."""
    i = 0
    while stream[i] & 0x80:
        i += 1
    i += 1
    lits, copies = [], 0
    while i < len(stream):
        t = stream[i]
        kind = t & 3
        if kind == 0:
            ln = t >> 2
            extra = ln - 59 if ln >= 60 else 0
            if extra:
                ln = int.from_bytes(stream[i + 1:i + 1 + extra], "little")
            lits.append(ln + 1)
            i += 1 + extra + ln + 1
        else:
            copies += 1
            i += (2, 3, 5)[kind - 1]
    assert i == len(stream)
    return lits, copies


def test_inputs_have_their_properties():
    """No GPU: per 32 KiB unit the oracle's streams show what each input is for
    (bounds a little under what the generators give), and the oracle decodes
    what it encoded at every chunk."""
    for name in INPUTS:
        out, offs = want(name, 32768)
        for u in range(TOTAL // 32768):
            lits, copies = elements(out[int(offs[u]):int(offs[u + 1])])
            if name == "mixed200":
                assert copies >= 3352 and max(lits) >= 400, (u, copies, max(lits))
            elif name == "sparse20":
                assert sum(1 for x in lits if 20 <= x <= 31) >= 369, u
            else:
                assert copies >= 6512 and copies > 20 * 49, (u, copies)
        for chunk in CHUNKS:
            out, offs = want(name, chunk)
            back = oracle.decompress_streams(np.frombuffer(out, dtype=np.uint8), offs, TOTAL, chunk)
            assert np.array_equal(back, make(name, TOTAL)), (name, chunk)
    assert TOTAL % 1000 == 72


@pytest.mark.gpu
@pytest.mark.parametrize("chunk", CHUNKS)
@pytest.mark.parametrize("name", INPUTS)
def test_refresh_inloop(codec, name, chunk):
    import torch
    a = make(name, TOTAL)
    x = torch.from_numpy(np.array(a)).cuda()
    comp, offs = codec.compress_tensor(x, chunk=chunk, layout=snappy_amd.STREAMS)
    out, want_offs = want(name, chunk)
    assert np.array_equal(offs.cpu().numpy().astype(np.uint64), want_offs)
    assert comp.cpu().numpy().tobytes() == out
    back = codec.decompress_tensor(comp, offs, TOTAL, chunk=chunk, layout=snappy_amd.STREAMS)
    assert np.array_equal(back.cpu().numpy(), a)


@pytest.mark.gpu
def test_single_layout_still_agrees(codec):
    """K1r64 (65,536-byte blocks, a short last one): its statement has no such path."""
    import torch
    a = make("mixed200", TOTAL)[:SINGLE_TAIL]
    x = torch.from_numpy(np.array(a)).cuda()
    comp, offs = codec.compress_tensor(x, chunk=65536, layout=snappy_amd.SINGLE)
    assert comp.cpu().numpy().tobytes() == oracle.compress(a.tobytes())
    back = codec.decompress_tensor(comp, offs, SINGLE_TAIL, chunk=65536, layout=snappy_amd.SINGLE)
    assert np.array_equal(back.cpu().numpy(), a)

"""K1r's token flush and tag-collision rounds inside the asm round loop.

A refresh with more than 48 tokens pending flushes them inside the hand-written
statement (token words, encoded sizes, the K2 segment record) and moves the
window there too; a round whose candidate had the probe's tag but other bytes
finishes as a miss inside the statement.  Each input below is dense in one way
those paths can go wrong:

* alpha2f: two symbols, all copies.  A flush is due at nearly every refresh,
  with 49-64 tokens pending; a unit holds thousands of tokens, so K2 segment
  records (every 256 tokens) fall at every alignment against the flushes.  A
  wrong record, size or token word is wrong K2 bytes.
* escapes: the same with planted runs of 255-400 random bytes (a literal gap
  that needs the token's long form) and of 300-400 equal bytes (a copy length
  that needs it, by way of the statement's code-4 exit), 700-1300 bytes apart:
  each sits among a full set of pending tokens.  Such a flush must leave the
  statement before it changes anything, and the C++ flush must find the state
  it always found.
* sparse20f: random bytes with a 6-byte copy from 1-29 back every 20-27 bytes.
  Every table slot is occupied and skip stays low, so candidates with the
  probe's 8-bit tag and other bytes turn up inside the step-1 range: on a
  round's first probe lane (its p - 1 is inserted late), on later lanes, and
  right before the window has to move.

Chunks 300 and 1000 have hash tables of 512 and 1,024 slots (another shift).
The bar is the oracle's bytes and unit offsets, bit for bit, and the round
trip.  One single-layout case shows K1r64 still agrees."""
import functools

import numpy as np
import pytest

import oracle
import snappy_amd

TOTAL = 128 << 10
SINGLE_TAIL = 65536 + 4097
INPUTS = ["alpha2f", "escapes", "sparse20f"]
CHUNKS = [300, 1000, 4096, 32768]
MUL = 0x1E35A7BD
DMAX, RMIN, LSMIN = 13, 2, 4  # the kernel's round shape (SNAPPY_K1R_DMAX, _RMIN, _LSMIN)


def escapes(seed: int, n: int) -> np.ndarray:
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 2, n, dtype=np.uint8)
    p, k = 1500, 0
    while p + 420 < n:
        if k & 1:
            ln = int(rng.integers(300, 401))
            a[p:p + ln] = k >> 1 & 1
        else:
            ln = int(rng.integers(255, 401))
            a[p:p + ln] = rng.integers(2, 256, ln, dtype=np.uint8)
        p += ln + int(rng.integers(700, 1301))
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
    if name == "alpha2f":
        a = np.random.default_rng(311).integers(0, 2, n, dtype=np.uint8)
    elif name == "escapes":
        a = escapes(312, n)
    else:
        a = sparse(313, n)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def want(name: str, chunk: int):
    """The oracle's bytes and unit offsets, computed once per case."""
    out, offs = oracle.compress_streams(make(name, TOTAL), chunk)
    return out.tobytes(), offs.copy()


def literal_bytes(n: int) -> int:
    return n + (1 if n <= 60 else 2 if n <= 256 else 3)


def copy_bytes(ln: int, off: int) -> int:
    n64 = (ln - 68 + 63) >> 6 if ln > 68 else 0
    rem = ln - 64 * n64
    has60 = rem > 64
    last = rem - 60 if has60 else rem
    return 3 * (n64 + has60) + (2 if last < 12 and off < 2048 else 3)


def probe_unit(b: bytes):
    """The probe loop of one unit, with the kernel's slot and tag (the table index
    and the next 8 bits of BE32 * MUL) and the shape of its lane-space rounds: a
    round holds up to DMAX step-1 probes of one window (q0 = the first probe - 1,
    moved when fewer than RMIN probe lanes are left) and ends at its first
    candidate with the probe's tag.  Returns the tokens (gap, length, offset),
    the encoded size, and the tag-equal, bytes-different probes of rounds the asm
    statement runs (skip <= 64 - DMAX at the round's start): on the round's first
    lane, on a later lane, and followed at once by a window move."""
    L = len(b)
    T, lg = 256, 8
    while T < 4096 and T < L:
        T <<= 1
        lg += 1
    sh = 32 - lg
    bp = b + bytes(4)

    def hw(q):
        w = int.from_bytes(bp[q:q + 4], "big")
        pr = (w * MUL) & 0xFFFFFFFF
        return pr >> sh, (pr >> (sh - 8)) & 0xFF, w

    tab = [0] * T
    toks, size, end = [], 0, 0
    first = later = moves = 0
    p, skip = 1, 33
    q0, rfirst, rlast, rasm = None, -1, -1, False
    newround, after_coll = True, False
    while not (L - p < (skip >> 5) + 15):
        ls = skip <= 64 - LSMIN and p <= L - 16
        if not ls:
            q0, newround, after_coll = None, True, False
        elif newround:
            lane0 = p - q0 if q0 is not None else 99
            if lane0 + RMIN > 62:
                moves += after_coll and q0 is not None
                q0, lane0 = p - 1, 1
            rfirst, rlast, rasm = p, q0 + min(lane0 + DMAX - 1, 62, L - 16 - q0), skip <= 64 - DMAX
            newround = False
        after_coll = False
        h, t, w = hw(p)
        c = tab[h]
        _, tc, wc = hw(c)
        if wc == w:
            n = 4
            while p + n < L and b[p + n] == b[c + n]:
                n += 1
            toks.append((p - end, n, p - c))
            size += (literal_bytes(p - end) if p > end else 0) + copy_bytes(n, p - c)
            tab[h] = p
            p += n
            end = p
            skip = 32
            newround = True
        else:
            if ls and rasm and tc == t:
                if p == rfirst:
                    first += 1
                else:
                    later += 1
                newround = after_coll = True
            elif ls and p == rlast:
                newround = True
            tab[hw(p - 1)[0]] = p - 1
            tab[h] = p
            p += skip >> 5
            skip += 1
    size += literal_bytes(L - end) if L > end else 0
    return toks, size, first, later, moves


@functools.lru_cache(maxsize=None)
def probes(name: str, chunk: int):
    """probe_unit() of every unit, its encoded size checked against the oracle's stream."""
    a = make(name, TOTAL).tobytes()
    _, offs = want(name, chunk)
    res = []
    for u in range((TOTAL + chunk - 1) // chunk):
        b = a[u * chunk:(u + 1) * chunk]
        r = probe_unit(b)
        hdr = 1 + (len(b) >= 128) + (len(b) >= 16384)
        assert hdr + r[1] == int(offs[u + 1]) - int(offs[u]), (name, chunk, u)
        res.append(r)
    return res


def test_inputs_have_their_properties():
    """No GPU: the restated probe loop (its encoded sizes equal to the oracle's
    stream lengths, unit by unit) shows what each input is for.  Per 32 KiB unit,
    bounds a little under what the generators give; at every chunk size where a
    kind can occur, at least one of it; and the oracle decodes what it encoded."""
    for name in INPUTS:
        for u, (toks, _, first, later, moves) in enumerate(probes(name, 32768)):
            copies = len(toks)
            gaps = sum(1 for g, n, o in toks if g >= 255)
            longs = sum(1 for g, n, o in toks if n >= 259)
            print(name, u, "copies", copies, "gaps >= 255", gaps, "copies >= 259", longs,
                  "collisions first / later / then a move", first, later, moves)
            if name == "alpha2f":
                assert copies >= 6400 and copies > 25 * 256 and gaps == 0 and longs == 0, (u, copies)
            elif name == "escapes":
                assert copies >= 4800 and gaps >= 11 and longs >= 10, (u, copies, gaps, longs)
            else:
                assert first >= 7 and later >= 70 and moves >= 2, (u, first, later, moves)
        for chunk in CHUNKS:
            res = probes(name, chunk)
            if name == "escapes" and chunk >= 1000:
                assert sum(1 for r in res for g, n, o in r[0] if g >= 255) >= 1, chunk
                assert sum(1 for r in res for g, n, o in r[0] if n >= 259) >= 1, chunk
            if name == "sparse20f":
                tot = [sum(r[k] for r in res) for k in (2, 3, 4)]
                print(name, chunk, "collisions first / later / then a move", *tot)
                assert min(tot) >= 1, (chunk, tot)
            if name != "sparse20f" and chunk >= 1000:  # more tokens than a flush holds, in every full unit
                assert min(len(r[0]) for r in res[:-1]) > 64, chunk
            out, offs = want(name, chunk)
            back = oracle.decompress_streams(np.frombuffer(out, dtype=np.uint8), offs, TOTAL, chunk)
            assert np.array_equal(back, make(name, TOTAL)), (name, chunk)


@pytest.mark.gpu
@pytest.mark.parametrize("chunk", CHUNKS)
@pytest.mark.parametrize("name", INPUTS)
def test_flush_inloop(codec, name, chunk):
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
    """K1r64 (65,536-byte blocks, a short last one): its statement has neither path."""
    import torch
    a = make("escapes", TOTAL)[:SINGLE_TAIL]
    x = torch.from_numpy(np.array(a)).cuda()
    comp, offs = codec.compress_tensor(x, chunk=65536, layout=snappy_amd.SINGLE)
    assert comp.cpu().numpy().tobytes() == oracle.compress(a.tobytes())
    back = codec.decompress_tensor(comp, offs, SINGLE_TAIL, chunk=65536, layout=snappy_amd.SINGLE)
    assert np.array_equal(back.cpu().numpy(), a)

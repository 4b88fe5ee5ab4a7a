"""The hit round's tail in K1r's asm round loop: the length test, and the way
from a hit that ends the window straight into the refresh.

A hit round tests its length once for a tag collision (fewer than 4 equal
bytes) before it writes the next round's first lane; 64 or more equal bytes
are found on the leaving path alone (first lane + length is past every window
limit); the tag-collision ways fix skip by the previous round's pending flag.  In
K1r a hit that ends the window away from the unit's end goes to the refresh (or
the flush before it) without the clamp to the unit's end and with skip = 32 and
the flush test on the drained count alone.  Each input is dense in one way
those paths can go wrong:

* lens: two-symbol filler with planted pairs of a unique block, the second
  copy right after a match that moved the window or at any lane: matches of
  56-70, 125-131 and 250-300 bytes found on lane 1, mid-window and on lanes
  59-62.  (Lane 0 holds p - 1 of a window's first probe and is never probed,
  and a window's limit is at most lane 60, so a length of 60 or more always
  ends the window: 60-63 by the direct way, 64 and more by the code-4 exit;
  128 and more have no differing dword among the 32 the round looks at.)  The
  longest length that stays (first lane + length == the limit) and the first
  that leaves are both there.
* ends: per unit a planted match that ends 17 .. 0 bytes before the unit's end
  (d = its end - (L - 16) = -1 .. 16): d <= 0 from a window that ends far from
  the unit's end is the direct way's side of its compare (d = 0 the boundary),
  d >= 1 the clamp and the code-1 exit; in the last window, whose limit is
  L - 16 - q0, the hit whose next lane is exactly the limit stays and the next
  one leaves.
* colls: planted pairs of 4-byte words with the same table slot and 8-bit tag
  at every table size, the second one right after a match (skip exactly 32, on
  the round's first lane or a later one), after a full round of misses (skip
  above 32), right after a match of 60-63 bytes (the first round of a window
  moved by the direct way) and there after a flush.  A wrong previous-round
  flag moves the next probe and so the output.
* pend: two symbols with runs of 300-400 equal bytes: hits end the window with
  46, 47 (no flush) and 48, 49 (flush) tokens drained, and flushes entered by the
  direct way hold a long-form token and leave by code 2.

model_unit() restates the probe loop with the kernel's round shape and token
bookkeeping; its encoded sizes equal the oracle's stream lengths unit by unit,
and test_inputs_reach_their_states asserts on it that the inputs reach the
states above.  The bar on the GPU is the oracle's bytes and unit offsets, bit
for bit, and the round trip.  One single-layout case covers K1r64, whose both
loops share the length test."""
import functools
from collections import Counter

import numpy as np
import pytest

import oracle
import snappy_amd

TOTAL = 128 << 10
SINGLE_TAIL = 65536 + 4097
INPUTS = ["lens", "ends", "colls", "pend"]
CHUNKS = [300, 1000, 4096, 32768]
MUL = 0x1E35A7BD
MUL_INV = pow(MUL, -1, 1 << 32)
DMAX, RMIN, LSMIN = 13, 2, 4  # the kernel's round shape (SNAPPY_K1R_DMAX, _RMIN, _LSMIN)
L0MAX = 62 - RMIN


def uniq(rng, n: int) -> np.ndarray:
    """n bytes outside the filler's alphabet."""
    return rng.integers(2, 256, n, dtype=np.uint8)


def lens(seed: int, n: int) -> np.ndarray:
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 2, n, dtype=np.uint8)
    classes = [(56, 63), (60, 63), (64, 70), (125, 131), (250, 300), (20, 59)]
    p, k = 40, 0

    def put(x, gap_lo, gap_hi):
        nonlocal p
        a[p:p + len(x)] = x
        p += len(x) + (int(rng.integers(gap_lo, gap_hi)) if gap_hi else 0)

    while p + 1000 < n:
        lo, hi = classes[(k // 3) % len(classes)]
        x = uniq(rng, int(rng.integers(lo, hi + 1)))
        put(x, 3, 40)  # the source, then a byte of the filler
        if k % 3 == 0:  # a 64-byte match first: the window moves, the copy is probed on lane 1
            y = uniq(rng, 64)
            put(y, 3, 20)
            put(y, 0, 0)
        elif k % 3 == 1:  # and a match of 58 / 59 bytes and 0-2 misses after it: lanes 59-62
            y, w = uniq(rng, 64), uniq(rng, 58 + k // 3 % 2)
            put(y, 3, 20)
            put(w, 3, 20)
            put(y, 0, 0)
            put(w, 0, 0)
            put(uniq(rng, k // 6 % 3), 0, 0)
        put(x, 5, 60)
        k += 1
    return a


def ends(seed: int, n: int, chunk: int) -> np.ndarray:
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 2, n, dtype=np.uint8)
    ds = [0, -1, 1, 16] + [x for i in range(2, 16) for x in (i, (0, 1, -1)[i % 3])]  # every other unit ends at the boundary
    for u in range(n // chunk):
        e = (u + 1) * chunk
        d = ds[u % len(ds)]
        ln = int(rng.integers(max(6, d + 5), 50))  # (it starts where the unit is still probed)
        x = uniq(rng, ln)
        stop = e - 16 + d
        src = stop - ln - int(rng.integers(60, 100)) - ln  # (filler enough for matches: skip is 32 again)
        if src < u * chunk + 8:
            continue
        a[src:src + ln] = x
        a[stop - ln:stop] = x
        if stop < e:
            a[stop] = 255 if a[src + ln] != 255 else 254  # the match ends at stop
    return a


def colliding(rng, k: int):
    """k different words whose products with MUL agree in their top 20 bits: the
    same slot and tag for every table size (256 .. 4,096 slots)."""
    top = int(rng.integers(0, 1 << 20)) << 12
    low = rng.choice(1 << 12, k, replace=False)
    return [np.frombuffer((((top | int(x)) * MUL_INV) & 0xFFFFFFFF).to_bytes(4, "big"), dtype=np.uint8) for x in low]


def colls(seed: int, n: int) -> np.ndarray:
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 2, n, dtype=np.uint8)
    p, k = 30, 0
    while p + 400 < n:
        wa, wb = colliding(rng, 2)
        kind = k % 5
        a[p:p + 4] = wa
        p += 4 + int(rng.integers(4, 16))
        if kind == 2:  # a full round of misses, then the collision
            m = int(rng.integers(14, 20))
            a[p:p + m] = uniq(rng, m)
            p += m
        else:
            ln = int(rng.integers(60, 64)) if kind >= 3 else int(rng.integers(8, 13))
            z = uniq(rng, ln)
            a[p:p + ln] = z
            p += ln + int(rng.integers(4, 16))
            a[p:p + ln] = z  # its match ends at the planted word, or 1-3 misses before it
            p += ln
            if kind in (1, 4):
                g = int(rng.integers(1, 4))
                a[p:p + g] = uniq(rng, g)
                p += g
        a[p:p + 4] = wb
        p += 4 + int(rng.integers(10, 90))
        k += 1
    return a


def pend_runs(seed: int, n: int) -> np.ndarray:
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 2, n, dtype=np.uint8)
    p, k = 900, 0
    while p + 420 < n:
        ln = int(rng.integers(300, 401))
        a[p:p + ln] = k & 1
        p += ln + int(rng.integers(500, 1101))
        k += 1
    return a


@functools.lru_cache(maxsize=None)
def make(name: str, chunk: int) -> np.ndarray:
    if name == "lens":
        a = lens(411, TOTAL)
    elif name == "ends":
        a = ends(412, TOTAL, chunk)
    elif name == "colls":
        a = colls(413, TOTAL)
    else:
        a = pend_runs(414, TOTAL)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def want(name: str, chunk: int):
    """The oracle's bytes and unit offsets, computed once per case."""
    out, offs = oracle.compress_streams(make(name, chunk), chunk)
    return out.tobytes(), offs.copy()


def literal_bytes(n: int) -> int:
    return n + (1 if n <= 60 else 2 if n <= 256 else 3)


def copy_bytes(ln: int, off: int) -> int:
    n64 = (ln - 68 + 63) >> 6 if ln > 68 else 0
    rem = ln - 64 * n64
    has60 = rem > 64
    last = rem - 60 if has60 else rem
    return 3 * (n64 + has60) + (2 if last < 12 and off < 2048 else 3)


def lane_class(f: int) -> str:
    return "l1" if f == 1 else "l59" if f >= 59 else "mid"


def len_class(n: int) -> str:
    for name, lo, hi in (("60-63", 60, 63), ("64-68", 64, 68), ("127-129", 127, 129), ("252+", 252, 1 << 20)):
        if lo <= n <= hi:
            return name
    return "other"


def model_unit(b: bytes):
    """One unit as K1r runs it.  The probe loop with the kernel's slot and tag (the
    table index and the next 8 bits of BE32 * MUL); lane-space rounds while skip
    <= 64 - LSMIN: a window q0 (its first probe - 1, moved when fewer than RMIN
    probe lanes are left), a round of up to DMAX step-1 probes that ends at its
    first candidate with the probe's tag, the match's token deferred into the
    next round, a flush at a refresh with more than 48 tokens pending (the deferred
    one counted); serial probes above that, which flush at 64.  Returns the
    encoded size and a Counter of what the rounds of the asm statement (skip <=
    64 - DMAX at the round's start) met:
      ("stay" | "fast" | "x4" | "clamp", lane class, length class)   a hit's way on
      ("edge", "stay" | "leave")    a hit whose next lane is the window limit / one past it
      ("d", way, d)                 a hit's end - (L - 16), -2 .. 16, by its way on
      ("lastwin", limit, "stay" | "clamp")   the same boundary at the last window's limit
      ("coll", "hit" | "miss", "first" | "later", None | "move" | "flush")   a tag collision:
           the round before it, its lane, and whether its round is the first of a
           window a hit just moved (after a flush there)
      ("collskip", skip)            the skip a collision found
      ("fastpend", n)               the drained tokens at a hit that ends the window
      ("flush", "fast" | "tail", "short" | "long")   a flush inside the statement
    """
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

    ev = Counter()
    tab = [0] * T
    size, end = 0, 0
    pending, dk = [], None  # the drained tokens (gap, length) and the deferred one
    p, skip = 1, 33

    def is_long(t):
        return t[0] >= 255 or t[1] >= 259

    def flush():
        pending.clear()

    def refresh(way):
        """The window moves to p - 1; way: None from C++, "fast" / "tail" inside the statement."""
        flushed = len(pending) + (dk is not None) > 48
        if flushed:
            if way:
                ev["flush", way, "long" if len(pending) > 63 or any(map(is_long, pending)) else "short"] += 1
            flush()
        return p - 1, ("flush" if flushed else "move") if way == "fast" else None

    def token(pf, n, c):
        nonlocal size, end
        size += (literal_bytes(pf - end) if pf > end else 0) + copy_bytes(n, pf - c)
        t = (pf - end, n)
        end = pf + n
        return t

    while not (L - p < (skip >> 5) + 15):
        if skip > 64 - LSMIN:  # a serial probe (the kernel's W-probe rounds)
            h, t, w = hw(p)
            c = tab[h]
            _, tc, wc = hw(c)
            if wc == w:
                n = 4
                while p + n < L and b[p + n] == b[c + n]:
                    n += 1
                if len(pending) == 64:
                    flush()
                pending.append(token(p, n, c))
                tab[h] = p
                p += n
                skip = 32
            else:
                tab[hw(p - 1)[0]] = p - 1
                tab[h] = p
                p += skip >> 5
                skip += 1
            continue
        # ---- lane-space rounds
        q0, fresh = refresh(None)
        prev = None
        while True:
            lane0 = p - q0
            asm = skip <= 64 - DMAX
            lim_e = L - 16 - q0
            if asm:
                last = min(lane0 + DMAX - 1, 62, lim_e)
            else:  # the C++ round: probes up to skip 64, whose step is 2 (it needs L - p >= 17)
                kcap = 64 - skip
                last = min(lane0 + kcap, 62, lim_e)
                if last == lane0 + kcap and last > L - 17 - q0:
                    last -= 1
            flag = dk is not None
            if flag:
                pending.append(dk)
                dk = None
            f = None
            for l in range(lane0, last + 1):
                q = q0 + l
                h, t, w = hw(q)
                c = tab[h]
                _, tc, wc = hw(c)
                if tc == t:
                    f = l
                    break
                tab[hw(q - 1)[0]] = q - 1
                tab[h] = q
            way = "tail"
            if f is None:
                nk = last - lane0 + 1
                p = q0 + lane0 + nk - 1 + ((skip + nk - 1) >> 5)
                skip += nk
                prev = "miss"
            elif wc == w:
                pf = q0 + f
                n = 4
                while pf + n < L and b[pf + n] == b[c + n]:
                    n += 1
                dk = token(pf, n, c)
                tab[h] = pf
                p = pf + n
                skip = 32
                prev = "hit"
                if asm:
                    lim0 = min(L0MAX, lim_e)
                    nl, d = f + n, p - (L - 16)
                    kind = "stay" if nl <= lim0 else "x4" if n >= 64 else "clamp" if d > 0 else "fast"
                    ev[kind, lane_class(f), len_class(n)] += 1
                    if nl == lim0:
                        ev["edge", "stay"] += 1
                    if nl == lim0 + 1 and n < 64:
                        ev["edge", "leave"] += 1
                    if -2 <= d <= 16 and n < 64:
                        ev["d", kind, d] += 1
                    if lim_e <= L0MAX and n < 64 and nl in (lim_e, lim_e + 1):
                        ev["lastwin", lim_e, "stay" if nl == lim_e else "clamp"] += 1
                    if kind == "fast":
                        ev["fastpend", len(pending)] += 1
                        way = "fast"
            else:  # a tag collision: a miss at lane f
                pf = q0 + f
                if asm:
                    ev["coll", "hit" if flag else "miss", "first" if f == lane0 else "later", fresh] += 1
                    ev["collskip", skip] += 1
                tab[hw(pf - 1)[0]] = pf - 1
                tab[h] = pf
                p = pf + ((skip + f - lane0) >> 5)
                skip += f - lane0 + 1
                prev = "coll"
            fresh = None
            if not (skip <= 64 - LSMIN and p <= L - 16):
                break
            if p - q0 > L0MAX:
                q0, fresh = refresh(way if asm else None)
        if dk is not None:
            pending.append(dk)
            dk = None
    size += literal_bytes(L - end) if L > end else 0
    return size, ev


@functools.lru_cache(maxsize=None)
def events(name: str, chunk: int):
    """model_unit() of every unit, its encoded size checked against the oracle's
    stream; the units' counters summed."""
    a = make(name, chunk).tobytes()
    _, offs = want(name, chunk)
    tot = Counter()
    for u in range((TOTAL + chunk - 1) // chunk):
        b = a[u * chunk:(u + 1) * chunk]
        size, ev = model_unit(b)
        hdr = 1 + (len(b) >= 128) + (len(b) >= 16384)
        assert hdr + size == int(offs[u + 1]) - int(offs[u]), (name, chunk, u)
        tot.update(ev)
    return tot


def show(name, chunk, ev):
    for k in sorted(ev, key=str):
        print(name, chunk, k, ev[k])


def test_inputs_reach_their_states():
    """No GPU: the model (its encoded sizes equal to the oracle's stream lengths,
    unit by unit) shows that each input reaches the states it is for, at every
    chunk size whose units have room for them; and the oracle decodes what it
    encoded."""
    for name in INPUTS:
        for chunk in CHUNKS:
            ev = events(name, chunk)
            show(name, chunk, ev)
            out, offs = want(name, chunk)
            back = oracle.decompress_streams(np.frombuffer(out, dtype=np.uint8), offs, TOTAL, chunk)
            assert np.array_equal(back, make(name, chunk)), (name, chunk)

    for chunk in CHUNKS:
        ev = events("lens", chunk)
        # (a 300-byte unit has no room for the planted way to lanes 59-62, nor for two runs of 125 and more)
        lens_fit = ["60-63", "64-68"] + (["127-129", "252+"] if chunk >= 1000 else [])
        for lc in ("l1", "mid") + (("l59",) if chunk >= 1000 else ()):
            for ln in lens_fit:
                kind = "fast" if ln == "60-63" else "x4"
                assert ev[kind, lc, ln] >= 1, (chunk, kind, lc, ln)
        assert ev["edge", "stay"] >= 1 and ev["edge", "leave"] >= 1, chunk
        assert sum(v for k, v in ev.items() if k[0] == "stay") >= 100, chunk

    for chunk in CHUNKS:
        ev = events("ends", chunk)
        units = TOTAL // chunk
        # the planted ends cycle through d = 0, -1, 1, 16, then 2 .. 15 with 0 / 1 / -1 between them, unit by unit
        reach = [0, -1, 1, 16][:units] + (list(range(2, 16)) if units >= 32 else [])
        for d in reach:
            got = sum(v for k, v in ev.items() if k[0] == "d" and k[2] == d)
            assert got >= 1, (chunk, d)
            if d >= 1:  # past L - 16: never the direct way
                assert ev["d", "fast", d] == 0 and ev["d", "stay", d] == 0, (chunk, d)
        if units >= 100:
            assert ev["d", "fast", 0] >= 1 and ev["d", "fast", -1] >= 1 and ev["d", "clamp", 1] >= 1, chunk
            assert ev["d", "stay", 0] >= 1 and ev["d", "clamp", 16] >= 1, chunk
            lanes_stay = {k[1] for k in ev if k[0] == "lastwin" and k[2] == "stay"}
            lanes_clamp = {k[1] for k in ev if k[0] == "lastwin" and k[2] == "clamp"}
            print("ends", chunk, "last-window limits with the boundary hit:", sorted(lanes_stay), sorted(lanes_clamp))
            assert len(lanes_stay) >= 10 and len(lanes_clamp) >= 10, (chunk, lanes_stay, lanes_clamp)

    for chunk in CHUNKS:
        ev = events("colls", chunk)
        c = Counter()
        for k, v in ev.items():
            if k[0] == "coll":
                c[k[1], k[2]] += v
                if k[3]:
                    c["moved", k[1]] += v
                    c[k[3], k[2]] += v
        print("colls", chunk, dict(c))
        assert c["hit", "first"] >= 5 and c["hit", "later"] >= 5 and c["miss", "first"] + c["miss", "later"] >= 5, chunk
        assert c["moved", "hit"] >= 3 and c["move", "first"] >= 1 and c["move", "later"] >= 1, chunk
        if chunk >= 1000:  # (a 300-byte unit never has 48 tokens pending beside a planted record)
            assert c["flush", "first"] + c["flush", "later"] >= 1, chunk
        assert ev["collskip", 32] >= 5 and sum(v for k, v in ev.items() if k[0] == "collskip" and k[1] > 32) >= 5, chunk

    for chunk in (4096, 32768):
        ev = events("pend", chunk)
        for n in (46, 47, 48, 49):
            assert ev["fastpend", n] >= 1, (chunk, n)
        assert ev["flush", "fast", "short"] >= 1 and ev["flush", "fast", "long"] >= 1, chunk


@pytest.mark.gpu
@pytest.mark.parametrize("chunk", CHUNKS)
@pytest.mark.parametrize("name", INPUTS)
def test_hit_tail(codec, name, chunk):
    import torch
    a = make(name, chunk)
    x = torch.from_numpy(np.array(a)).cuda()
    comp, offs = codec.compress_tensor(x, chunk=chunk, layout=snappy_amd.STREAMS)
    out, want_offs = want(name, chunk)
    assert np.array_equal(offs.cpu().numpy().astype(np.uint64), want_offs)
    assert comp.cpu().numpy().tobytes() == out
    back = codec.decompress_tensor(comp, offs, TOTAL, chunk=chunk, layout=snappy_amd.STREAMS)
    assert np.array_equal(back.cpu().numpy(), a)


@functools.lru_cache(maxsize=None)
def single_input() -> np.ndarray:
    """A 65,536-byte block of lens, colls and ends in turn, and a short block."""
    a = np.concatenate([make("lens", 32768)[:24576], make("colls", 32768)[:24576], make("ends", 300)[:SINGLE_TAIL - 49152]])
    a.setflags(write=False)
    return a


def test_single_input_reaches_k1r64s_states():
    """No GPU: the model's rounds on the first block (K1r64 has the same round shape
    and table): lengths of 64 and more, and collisions after a hit and after a miss."""
    _, ev = model_unit(single_input()[:65536].tobytes())
    show("single", 65536, ev)
    assert sum(v for k, v in ev.items() if k[0] == "x4") >= 10
    assert sum(v for k, v in ev.items() if k[0] == "coll" and k[1] == "hit") >= 5
    assert sum(v for k, v in ev.items() if k[0] == "coll" and k[1] == "miss") >= 5


@pytest.mark.gpu
def test_single_layout(codec):
    """K1r64 (65,536-byte blocks, a short last one): both its loops have the length
    test, its code-4 exit now taken on the leaving path and its code-5 exit before lane0 is written."""
    import torch
    a = single_input()
    x = torch.from_numpy(np.array(a)).cuda()
    comp, offs = codec.compress_tensor(x, chunk=65536, layout=snappy_amd.SINGLE)
    assert comp.cpu().numpy().tobytes() == oracle.compress(a.tobytes())
    back = codec.decompress_tensor(comp, offs, SINGLE_TAIL, chunk=65536, layout=snappy_amd.SINGLE)
    assert np.array_equal(back.cpu().numpy(), a)

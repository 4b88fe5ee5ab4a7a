"""K1r / K1r64 with the unit in registers in memory byte order.

The registers hold each dword as it lies in memory.  The four bytes at a
position x are funnelled out of the dword that holds x and the one after it by
v_alignbyte_b32 with x as the shift (pa at pf, ca at c, a window lane's bytes at
q0 + lane), the first differing byte of two such values is the lowest set byte
of their xor, and only the hash sees a byte-swapped (big-endian) value.  What can
go wrong depends on the two positions' low bits, on which dword and which byte
of it differs first, and on where a dword comes from (registers, the register
pair that wraps, global memory, the byte-wise load of an unaligned or partial
dword).  The inputs here are planted so that every such case is met inside the
asm round loop; model_unit() restates the kernel's rounds (its encoded sizes are
checked against the oracle's streams unit by unit) and
test_inputs_reach_their_cases asserts on it that they are.

K1r input (`planted`, built per unit length): random bytes with
* copies: for each (pf & 3, c & 3) a copy of each length 4-7, 60-68, 248-251 and
  252-255 after a gap of 5-8 bytes, from a source in an earlier gap: the first
  differing dword is lane 1, 15, 16, 17 or 62 of the 64 the round gathers, or
  none of lanes 0-62 (the length read back from lane 63), ending at each of its
  four bytes;
* tag collisions (the first differing dword is lane 0): for each (pf & 3, c & 3)
  a pair of words with the same slot and tag that share no byte and one that
  shares the first byte.  A candidate that was inserted has the probe's slot and
  tag, and such pairs that share two or three bytes do not exist at these table
  sizes: they would differ by d < 65,536 with d * kMul mod 2^32 within
  2^(24 - lg) of zero, and no such d exists for 1,024 .. 4,096 slots
  (test_no_closer_collisions checks all of them).  Position 0 is the one
  candidate that need not have been inserted: a slot nothing has written holds
  it with the first word's tag, so only the 8 tag bits have to agree.  Every unit
  plants, at a pf & 3 that moves with the unit's number, a word that shares two
  and one that shares three bytes with the unit's first word, has its tag and
  probes a slot not yet written: lane 0 ending at bytes 2 and 3 with c = 0, at
  each pf & 3 (the other fifteen (pf & 3, c & 3) cannot end there);
* candidates at positions 0-3 of every unit: a copy of the unit's first bytes
  or a word that collides with them, in turn;
* a copy of 60-63 bytes followed at once by another copy: the window moves and
  its first probe, lane 1, is a hit, at each q0 & 3 (the refreshed lanes' hashes
  decide it);
* 40-42 unique bytes and a copy: a W-probe hit at each p & 3 (the C++ funnel);
* a last copy that runs to the unit's end.
Unit lengths 1,024, 1,025, 2,050, 4,095 and 4,096: the odd ones put the units at
all four base alignments (dwords built byte by byte) and end in a partial dword
that a match runs through (the zero fill past L); 4,096-byte units also run from
bases 1-3.

K1r64 input: eight 65,536-byte units of test_k1r64_ring's generators (two each of
far_run, far_alpha, wrap, edge): candidates fetched from global memory, from the
register pair 127 / 0 and within 512 bytes of the ring's first resident byte, at
each c & 3, in asm rounds; run as one stream of blocks from bases 0-3.

The bar is the oracle's bytes and unit offsets, bit for bit, and the round trip.
Builds with v_ffbh_u32 left in the hit round, and with the funnel's two dwords
swapped, fail this file (profiles/r16c_*)."""
import functools
from collections import Counter

import numpy as np
import pytest

import oracle
import snappy_amd
import test_k1r64_ring as ring

MUL = 0x1E35A7BD
MUL_INV = pow(MUL, -1, 1 << 32)
LSMIN, RMIN = 4, 2  # the kernel's round shape (SNAPPY_K1R_LSMIN, _RMIN; DMAX 13, K1r64 12)
L0MAX = 62 - RMIN
CHUNKS = [1024, 1025, 2050, 4095, 4096]
PASSES = 3
COPY_LENS = [4, 5, 6, 7] + list(range(60, 69)) + list(range(248, 256))
LANES = (0, 1, 15, 16, 62)
BLOCK = 65536
BIG_KINDS = ["far_run", "far_alpha", "wrap", "edge"]


def lg_of(L: int) -> int:
    T, lg = 256, 8
    while T < 4096 and T < L:
        T <<= 1
        lg += 1
    return lg


def literal_bytes(n: int) -> int:
    return n + (1 if n <= 60 else 2 if n <= 256 else 3)


def copy_bytes(ln: int, off: int) -> int:
    n64 = (ln - 68 + 63) >> 6 if ln > 68 else 0
    rem = ln - 64 * n64
    has60 = rem > 64
    last = rem - 60 if has60 else rem
    return 3 * (n64 + has60) + (2 if last < 12 and off < 2048 else 3)


def model_unit(b: bytes, dmax: int = 13, big: bool = False):
    """One unit as K1r runs it (test_k1r_tail's model with this file's events):
    lane-space rounds while skip <= 64 - LSMIN, a round of up to dmax step-1 probes
    that ends at its first candidate with the probe's tag; serial probes (the
    kernel's W-probe rounds) above that.  Returns the encoded size and a Counter
    of what the rounds of the asm statement (skip <= 64 - dmax at the round's
    start) met.  n is the common prefix of the bytes at pf and c with zeros past
    the unit's end, as the registers hold them:
      ("hit", pf & 3, c & 3, lane, n & 3)   lane = n // 4 if that is one of LANES,
                                            "none" for n >= 252, else "other"
      ("len", length)              the match's length, 4-7 and 60-68
      ("cpos", c, "match" | "coll")   a candidate at position 0-3
      ("c0", pf & 3)               a verified match whose candidate is position 0
      ("twin0", pf & 3, n)         a tag collision with position 0 that shares n = 2 or 3 bytes
      ("winhit", q0 & 3, "entry" | "moved")   the first round of a window hits on lane 1
      ("toend", L & 3)             a match that runs to the unit's end
      ("far" | "wrap" | "edge", c & 3)   big: the candidate's place against the ring
    and from the serial probes ("wprobe", p & 3, c & 3) for every hit."""
    L = len(b)
    lg = lg_of(L)
    sh = 32 - lg
    x = np.frombuffer(b + bytes(4), dtype=np.uint8).astype(np.uint64)
    w = (x[:-3] << 24) | (x[1:-2] << 16) | (x[2:-1] << 8) | x[3:]
    pr = (w * MUL) & 0xFFFFFFFF
    H, TG, W = (pr >> sh).tolist(), ((pr >> (sh - 8)) & 0xFF).tolist(), w.tolist()
    bz = b + bytes(8)
    ev = Counter()
    tab = [0] * (1 << lg)
    size, end = 0, 0
    p, skip = 1, 33

    def token(pf, n, c):
        nonlocal size, end
        size += (literal_bytes(pf - end) if pf > end else 0) + copy_bytes(n, pf - c)
        end = pf + n

    while not (L - p < (skip >> 5) + 15):
        if skip > 64 - LSMIN:  # a serial probe
            h = H[p]
            c = tab[h]
            if W[c] == W[p]:
                n = 4
                while p + n < L and b[p + n] == b[c + n]:
                    n += 1
                ev["wprobe", p & 3, c & 3] += 1
                token(p, n, c)
                tab[h] = p
                p += n
                skip = 32
            else:
                tab[H[p - 1]] = p - 1
                tab[h] = p
                p += skip >> 5
                skip += 1
            continue
        q0, fresh = p - 1, "entry"
        while True:
            lane0 = p - q0
            asm = skip <= 64 - dmax
            lim_e = L - 16 - q0
            if asm:
                last = min(lane0 + dmax - 1, 62, lim_e)
            else:  # the C++ round: probes up to skip 64, whose step is 2 (it needs L - p >= 17)
                kcap = 64 - skip
                last = min(lane0 + kcap, 62, lim_e)
                if last == lane0 + kcap and last > L - 17 - q0:
                    last -= 1
            f = None
            for l in range(lane0, last + 1):
                q = q0 + l
                h = H[q]
                c = tab[h]
                if TG[c] == TG[q]:
                    f = l
                    break
                tab[H[q - 1]] = q - 1
                tab[h] = q
            if f is None:
                nk = last - lane0 + 1
                p = q0 + lane0 + nk - 1 + ((skip + nk - 1) >> 5)
                skip += nk
            else:
                pf = q0 + f
                nr = 0
                while pf + nr < L + 4 and bz[pf + nr] == bz[c + nr]:
                    nr += 1
                n = min(nr, L - pf)
                if asm:
                    m = nr >> 2
                    ev["hit", pf & 3, c & 3, m if m in LANES else "none" if nr >= 252 else "other", nr & 3] += 1
                    if c < 4:
                        ev["cpos", c, "match" if nr >= 4 else "coll"] += 1
                    if c == 0 and nr >= 4:
                        ev["c0", pf & 3] += 1
                    if c == 0 and nr in (2, 3):
                        ev["twin0", pf & 3, nr] += 1
                    if fresh and f == 1:
                        ev["winhit", q0 & 3, fresh] += 1
                    if nr >= 4:
                        if n <= 7 or 60 <= n <= 68:
                            ev["len", n] += 1
                        if pf + n == L:
                            ev["toend", L & 3] += 1
                    if big:
                        F = ((pf >> 8) - 126) << 8  # test_k1r64_ring: the ring's first resident byte is in [F - 256, F]
                        if F > 0:
                            kind = ("far" if c + 512 <= F else "edge" if F - 512 <= c < F
                                    else "wrap" if c >= F and (c >> 8) & 127 == 127 else None)
                            if kind:
                                ev[kind, c & 3] += 1
                if nr >= 4:
                    token(pf, n, c)
                    tab[h] = pf
                    p = pf + n
                    skip = 32
                else:  # a tag collision: a miss at lane f
                    tab[H[pf - 1]] = pf - 1
                    tab[h] = pf
                    p = pf + ((skip + f - lane0) >> 5)
                    skip += f - lane0 + 1
            fresh = None
            if not (skip <= 64 - LSMIN and p <= L - 16):
                break
            if p - q0 > L0MAX:
                q0, fresh = p - 1, "moved"
    size += literal_bytes(L - end) if L > end else 0
    return size, ev


# ---------------------------------------------------------------- K1r input


def partner(wa: int, lg: int, share: int, rng):
    """A word with wa's slot and tag (1 << lg slots) that shares exactly `share`
    leading bytes with it, or None."""
    lim = 1 << (24 - lg)
    top = ((wa * MUL) & 0xFFFFFFFF) & ~(lim - 1)
    w = ((np.uint64(top) | np.arange(lim, dtype=np.uint64)) * np.uint64(MUL_INV)) & np.uint64(0xFFFFFFFF)
    d = w ^ np.uint64(wa)
    ok = (d >> np.uint64(24) != 0) if share == 0 else ((d >> np.uint64(24) == 0) & (d >> np.uint64(16) != 0))
    w = w[ok]
    return int(w[int(rng.integers(0, len(w)))]) if len(w) else None


def plan(rng):
    items = []
    for pfa in range(4):
        for ca in range(4):
            items += [("copy", pfa, ca, n) for n in COPY_LENS]
            items += [("coll", pfa, ca, share) for share in (0, 1)]
    items += [("adj", q) for q in range(4) for _ in range(3)]
    items += [("wp", pa) for pa in range(4) for _ in range(3)]
    return [items[i] for i in rng.permutation(len(items))]


def room(item) -> int:
    """The bytes an item may take."""
    return {"copy": 8 + (item[3] if item[0] == "copy" else 0), "coll": 48, "adj": 90, "wp": 75}[item[0]]


def build_unit(rng, L: int, u: int, queue: list) -> np.ndarray:
    """One unit of L bytes: the candidates at positions 0-3, then items off the queue
    while they fit, then copies up to a last one that runs to the unit's end."""
    a = np.zeros(L, dtype=np.uint8)
    lg = lg_of(L)
    srcs = [[], [], [], []]  # gap positions (every one a miss, so inserted) by their low bits
    p = 0
    term = None  # the byte that would extend the last copy

    def gap(k):
        nonlocal p, term
        x = rng.integers(0, 256, k, dtype=np.uint8)
        while term is not None and x[0] == term:
            x[0] = rng.integers(0, 256)
        a[p:p + k] = x
        for q in range(max(p, 4), p + k):
            srcs[q & 3].append(q)
        p += k
        term = None

    def gap_to(low, least):
        gap(least + ((low - (p + least)) & 3))

    def word_at(q):
        return int.from_bytes(a[q:q + 4].tobytes(), "big")

    def put_word(wv):
        nonlocal p
        a[p:p + 4] = np.frombuffer(wv.to_bytes(4, "big"), dtype=np.uint8)
        p += 4

    def copy_from(c, n, tweak=True):
        nonlocal p, term
        if tweak and c > 0 and a[p - 1] == a[c - 1]:
            a[p - 1] ^= 0x55  # (or the copy would be found a byte early)
        for i in range(n):
            a[p + i] = a[c + i]
        p += n
        term = int(a[c + n])

    def source(ca, avoid=None):
        for k in range(4):  # (a unit's first copies: whatever class has a source yet)
            pool = [c for c in srcs[(ca + k) & 3][-12:] if c + 4 <= p and (avoid is None or a[c] != avoid)]
            if pool:  # (each source once: a copy's own position takes its slot)
                c = pool[int(rng.integers(0, len(pool)))]
                srcs[c & 3].remove(c)
                return c
        raise AssertionError("no source")

    def copy(pfa, ca, n, least=5):
        gap_to(pfa, least)
        copy_from(source(ca), n)

    def reset():  # a short copy: skip is 32 again
        copy(int(rng.integers(0, 4)), int(rng.integers(0, 4)), int(rng.integers(8, 13)))

    def coll(pfa, wa, share):
        wb = partner(wa, lg, share, rng)
        gap_to(pfa, 2)
        put_word(wb)
        gap(3)

    def prod(wv):
        return (wv * MUL) & 0xFFFFFFFF

    def twins(share):
        """Words with the tag of the unit's first word that share exactly its first `share` bytes."""
        w0 = word_at(0)
        bits = 8 * (4 - share)
        w = np.uint64(w0 >> bits << bits) | np.arange(1 << bits, dtype=np.uint64)
        tag = ((w * np.uint64(MUL)) >> np.uint64(24 - lg)) & np.uint64(0xFF)
        ok = (tag == (prod(w0) >> (24 - lg)) & 0xFF) & (((w ^ np.uint64(w0)) >> np.uint64(bits - 8)) & np.uint64(0xFF) != 0)
        return [int(v) for v in rng.permutation(w[ok])]

    def unset_twin(pfa, share):
        """A probe at pf & 3 = pfa whose slot nothing has written: its candidate is position 0 with the
        first word's tag (the table's initial state), and its word shares `share` bytes with that word."""
        nonlocal p
        gap_to(pfa, 2)
        for wv in twins(share):
            put_word(wv)
            if all(prod(word_at(q)) >> (32 - lg) != prod(wv) >> (32 - lg) for q in range(p - 4)):
                break
            p -= 4  # (every twin's slot is taken: this unit goes without; the model counts the others)
        gap(3)
        reset()

    gap(7)  # positions 0-3 and their words
    while not twins(3):  # (three shared bytes leave 255 words: one of them must have the tag)
        a[0:4] = rng.integers(0, 256, 4, dtype=np.uint8)
    unset_twin(u + 2, 3)  # first: the fewer slots are written, the surer the twin's is not
    unset_twin(u, 2)
    for c in (int(v) for v in rng.permutation(4)):
        if (u + c) & 1:
            gap_to((u >> 1) + c, 3)
            copy_from(c, int(rng.integers(5, 10)))
        else:
            coll((u >> 1) + c, word_at(c), 0)
            reset()
    if u == 0:  # every class of source before the first item asks for one
        gap(12)
        reset()
    while True:
        k = next((k for k in range(min(len(queue), 40)) if p + room(queue[k]) + 8 + 24 <= L), None)
        if k is None:
            break
        item = queue.pop(k)
        if item[0] == "copy":
            copy(item[1], item[2], item[3])
        elif item[0] == "coll":
            _, pfa, ca, share = item
            while True:
                wa = int(rng.integers(0, 1 << 32))
                if partner(wa, lg, share, rng) is not None:
                    break
            gap_to(ca, 3)
            put_word(wa)
            coll(pfa, wa, share)
            reset()
        elif item[0] == "adj":
            n = int(rng.integers(60, 64))
            copy((item[1] + 1 - n) & 3, int(rng.integers(0, 4)), n)
            copy_from(source(int(rng.integers(0, 4)), avoid=term), 8, tweak=False)  # at once: the moved window's lane 1
        else:  # 40 or 42 misses from skip 32 (the probes step by 2 from the 33rd on), then the copy
            gap_to(int(rng.integers(0, 4)), 5)
            copy_from(source(int(rng.integers(0, 4))), 8 + ((p - item[1]) & 1))  # it ends an even way from the hit
            gap_to(item[1], 40)
            copy_from(source(int(rng.integers(0, 4))), 12)
    while L - p > 80:
        copy(int(rng.integers(0, 4)), int(rng.integers(0, 4)), int(rng.integers(8, 41)))
    gap(5 + int(rng.integers(0, 4)))
    copy_from(source(int(rng.integers(0, 4))), L - p)
    return a


@functools.lru_cache(maxsize=None)
def planted(chunk: int) -> np.ndarray:
    rng = np.random.default_rng([516, chunk])
    queue = [it for _ in range(PASSES) for it in plan(rng)]
    units = []
    while queue:
        units.append(build_unit(rng, chunk, len(units), queue))
    while len(units) % 8:  # every (u & 1, alignment) for the candidates at positions 0-3
        units.append(build_unit(rng, chunk, len(units), queue))
    a = np.concatenate(units)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def want(chunk: int):
    out, offs = oracle.compress_streams(planted(chunk), chunk)
    return out.tobytes(), offs.copy()


@functools.lru_cache(maxsize=None)
def events(chunk: int):
    a = planted(chunk).tobytes()
    _, offs = want(chunk)
    tot = Counter()
    for u in range(len(a) // chunk):
        b = a[u * chunk:(u + 1) * chunk]
        size, ev = model_unit(b)
        hdr = 1 + (len(b) >= 128) + (len(b) >= 16384)
        assert hdr + size == int(offs[u + 1]) - int(offs[u]), (chunk, u)
        tot.update(ev)
    return tot


# ---------------------------------------------------------------- K1r64 input


@functools.lru_cache(maxsize=None)
def big_input() -> np.ndarray:
    a = np.concatenate([ring.unit_of(name, 516 + 10 * s + k, BLOCK) for s in range(2) for k, name in enumerate(BIG_KINDS)])
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def big_events():
    a = big_input().tobytes()
    _, offs = oracle.compress_streams(big_input(), BLOCK)
    tot = Counter()
    for u in range(len(a) // BLOCK):
        size, ev = model_unit(a[u * BLOCK:(u + 1) * BLOCK], dmax=12, big=True)
        assert 3 + size == int(offs[u + 1]) - int(offs[u]), u
        tot.update(ev)
    return tot


def test_no_closer_collisions():
    """Two words with the same slot and tag that share their first two bytes differ
    by d < 65,536 with d * kMul within 2^(24 - lg) of a multiple of 2^32: for tables
    of 1,024 slots and more there is no such d, so a tag collision with a candidate
    that was inserted (any but position 0 out of a slot never written) first differs
    at byte 0 or 1."""
    d = np.arange(1, 65536, dtype=np.uint64)
    x = (d * np.uint64(MUL)) & np.uint64(0xFFFFFFFF)
    near = np.minimum(x, np.uint64(1 << 32) - x)
    assert int(near.min()) >= 1 << (24 - 10)


def test_inputs_reach_their_cases():
    """No GPU: the model (its encoded sizes equal to the oracle's stream lengths,
    unit by unit) shows that every case of this file is met in an asm round."""
    for chunk in CHUNKS:
        ev = events(chunk)
        n_units = len(planted(chunk)) // chunk
        print(chunk, n_units, "units;", sum(v for k, v in ev.items() if k[0] == "hit"), "asm hit rounds")
        for pfa in range(4):
            for ca in range(4):
                for lane in (1, 15, 16, 62, "none"):
                    for byte in range(4):
                        assert ev["hit", pfa, ca, lane, byte] >= 1, (chunk, pfa, ca, lane, byte)
                for byte in (0, 1):  # (2 and 3 with an inserted candidate: test_no_closer_collisions)
                    assert ev["hit", pfa, ca, 0, byte] >= 1, (chunk, pfa, ca, 0, byte)
            for byte in (2, 3):  # position 0 out of a slot never written: the tag alone has to agree
                assert ev["twin0", pfa, byte] >= 1, (chunk, pfa, byte)
        for n in [4, 5, 6, 7] + list(range(60, 69)):
            assert ev["len", n] >= 8, (chunk, n)
        for c in range(4):
            assert ev["cpos", c, "match"] >= 1 and ev["cpos", c, "coll"] >= 1, (chunk, c)
            assert ev["c0", c] >= 1, (chunk, c)  # (c: pf & 3 of a verified copy of position 0)
        for q in range(4):
            assert ev["winhit", q, "moved"] >= 1, (chunk, q)
            assert sum(v for k, v in ev.items() if k[0] == "wprobe" and k[1] == q) >= 1, (chunk, q)
        assert ev["toend", chunk & 3] >= n_units // 2, chunk


def test_big_input_reaches_its_cases():
    """No GPU: K1r64's rounds on the eight blocks: far, wrap and edge candidates at
    each c & 3, and every (pf & 3, c & 3) with matches short and long."""
    ev = big_events()
    for kind in ("far", "wrap", "edge"):
        got = [ev[kind, ca] for ca in range(4)]
        print(kind, got)
        assert min(got) >= 4, (kind, got)
    for pfa in range(4):
        for ca in range(4):
            assert sum(v for k, v in ev.items() if k[0] == "hit" and k[1:3] == (pfa, ca)) >= 20, (pfa, ca)


def run_streams(codec, a: np.ndarray, chunk: int, off: int, out: bytes, want_offs):
    import torch
    buf = torch.zeros(off + a.size, dtype=torch.uint8, device="cuda")
    x = buf[off:]
    x.copy_(torch.from_numpy(np.array(a)))
    assert x.data_ptr() % 4 == off
    comp, offs = codec.compress_tensor(x, chunk=chunk, layout=snappy_amd.STREAMS)
    assert np.array_equal(offs.cpu().numpy().astype(np.uint64), want_offs)
    assert comp.cpu().numpy().tobytes() == out
    back = codec.decompress_tensor(comp, offs, a.size, chunk=chunk, layout=snappy_amd.STREAMS)
    assert np.array_equal(back.cpu().numpy(), a)


@pytest.mark.gpu
@pytest.mark.parametrize("chunk", CHUNKS)
def test_k1r_planted(codec, chunk):
    out, want_offs = want(chunk)
    run_streams(codec, planted(chunk), chunk, 0, out, want_offs)


@pytest.mark.gpu
@pytest.mark.parametrize("off", [1, 2, 3])
def test_k1r_planted_bases(codec, off):
    """4,096-byte units from a base at each odd alignment: every dword built byte by byte."""
    out, want_offs = want(4096)
    run_streams(codec, planted(4096), 4096, off, out, want_offs)


@functools.lru_cache(maxsize=None)
def big_want() -> bytes:
    return oracle.compress(big_input().tobytes())


@pytest.mark.gpu
@pytest.mark.parametrize("off", [0, 1, 2, 3])
def test_k1r64_blocks(codec, off):
    """Eight 65,536-byte blocks of one stream; off 0 stages segments by LDS-DMA, the others load them byte by byte."""
    import torch
    a = big_input()
    buf = torch.zeros(off + a.size, dtype=torch.uint8, device="cuda")
    x = buf[off:]
    x.copy_(torch.from_numpy(np.array(a)))
    comp, offs = codec.compress_tensor(x, chunk=BLOCK, layout=snappy_amd.SINGLE)
    assert comp.cpu().numpy().tobytes() == big_want()
    back = codec.decompress_tensor(comp, offs, a.size, chunk=BLOCK, layout=snappy_amd.SINGLE)
    assert np.array_equal(back.cpu().numpy(), a)

"""K4 (k4_decompress_units / k4_decompress_back, k4_body<BACK>) on planted element
streams: every hard-coded edge of the decoder reached on purpose.

Streams are built element by element (golden_inputs.enc_literal / enc_copy /
varint) over fresh random bytes, so a wrong source byte shows with probability
255/256.  k4_model() restates k4_body's control flow in Python -- the 768-byte
window (slide at o >= 256, restart at o >= 512), the up to three 64-position
halves (the next one only while E < 64 and hpos <= 440), the 64 element lanes,
the long-literal cut (e_lsrc + e_len > 508: k4_literal_hbm as the batch's first
element, a batch cut otherwise), the 1,024-bit span cut and span_cut, the 4 KiB
ring with lo = op_end - 4096, per copy and 64-byte pass the far / overlapping /
in-pass lanes, and the flush at op - F >= 2048 down to a multiple of 1,024 --
and checks that its batches execute exactly the serial element walk and end at
the unit's length.  test_inputs_have_their_properties (no GPU) runs it over every
input below, as pass 1 over the STREAMS units and as pass 2 over the deferred
blocks of the SINGLE stream, and asserts that each edge is reached on both sides.

A case is a list of elements that starts with a `reset` literal of 520-523 bytes:
it is long, so it is a batch of its own through k4_literal_hbm, and the batch after
it starts with a restarted window (o = 0..3) and a pass phase of 0, wherever the
case stands.  In the STREAMS inputs a case is one unit (varint(chunk), the case,
filler literals of 1-60 bytes up to chunk), chunk 8192 (every dst 16-aligned: the
u32x4 flush) and 8191 (all 16 residues: the byte flush); in the SINGLE input the
same cases are concatenated into 65,536-byte blocks.

Families:

* overlap: every copy (off 1..70, len 1..64) as copy-2, copy-4 and (len 4..11)
  copy-1, each at four or more phases of the 64-byte pass, one with phase + len >
  64 (len >= 2; a 1-byte copy never continues in the next pass) and one with
  phase < off (the source begins in the previous pass); groups of ~25 copies
  separated by 1-3 literal bytes, each group after a long literal (one batch).
* ring: offsets 3000..4200 with lengths 1, 2, 63, 64 and a random one, after 4,300+
  bytes from one literal (k4_literal_hbm, F = kop + kl) and from literals of <= 60
  bytes (the passes, the 2,048 / 1,024 flush); `edge` copies whose offset is set
  from the model's trace so that the first source byte is lo - 1, lo, lo + 1 or
  the copy straddles lo.
* long: literals of 509, 1023-1025, 4095-4097, 4100 and 8000 bytes with 2-4
  length bytes, as the first and as the k-th element of their batch, at every
  (dst & 3, src & 3), followed by copies reaching 1, kl - 1, kl, 4095, 4096 and
  4097 bytes back; sweeps of e_lsrc + e_len over 500..516 (508 | 509, and the next
  batch's o at 511 | 512) for every header width; 256-byte literals with one length
  byte at batch-start o of 244..258 (255 | 256; the only way a width-1 literal
  reaches k4_literal_hbm).
* span: 0-3 literal bytes and runs of 64-byte copies whose output ends at exactly
  1023, 1024 and 1025 at an element end; the batches after the cut run under
  span_cut.
* lanes: runs of 150 two-byte elements (E = 64 with dropped elements), mixes of
  2/3/5-byte elements and short literals (halves ending at 64..68), literals that
  put hpos on 436..446 (440 | 441).

The SINGLE input: after block 0 every block's first element is a copy reaching
back over the boundary (or a straddling literal followed by one), so pass 1 defers
it and k4_decompress_back decodes all of it; the boundaries cycle through a plain
back copy, an overlapping copy (off < len) at the boundary, one beginning within
off bytes after it, straddling copies (plain and overlapping) and straddling
literals (short and long).  The index is computed on the host from the element
walk and must equal codec.index_tensor's.

Hostile lengths (test_hostile_*): 4-byte-width literals declaring 2^32, 2^32 - 1,
2^32 - 5, 2^31 and 2^24 bytes, copy offsets 0 / e_op / e_op + 1, elements cut one
byte short, a literal overrunning by one byte, a preamble of chunk +- 1; the GPU
accepts exactly what the oracle accepts.  Every such literal is refused, as the
oracle refuses it: K4 adds a literal's length and size with saturation (in 32 bits
2^32 would be a length of 0 and a size of 5, which passes every check).  Each is
placed after other elements of its batch and, following a literal of 600 bytes,
as its batch's first element (k4_model's probe shows the lane), in pass 1 and in
pass 2.  In SINGLE the copy offsets are the copy's global position (accepted) and
that + 1 (ERR_OFFSET) in block 1, for a copy inside the block, a copy starting it
and a copy straddling into it, and positions 0 and 1 as block 0's first element.

Measured (test_inputs_have_their_properties prints them):
* STREAMS units per family (either chunk): overlap 278, ring 124, long 750, span 30,
  lanes 33; the SINGLE stream is 5,761,995 bytes in 88 blocks, 87 through pass 2
  (32 resumed literals, 22 resumed copies, 11 of them overlapping; 295 bytes of
  overlapping copies repeat an earlier block's bytes).
* pass 1 (chunk 8192 / 8191) and pass 2: batches starting at o = 255 | 256: 21 | 40,
  34 | 27 and 11 | 14; at 511 | 512: 8 | 9, 6 | 10 and 3 | 8; hpos 440 | 441: 26 | 14,
  23 | 30 and 4 | 3; e_lsrc + e_len 508 | 509: 60 | 78, 63 | 65 and 16 | 20, every
  value of 500..516 58-103, 61-99 and 10-25 times; batch output of 1023 / 1024 /
  1025 at an element end: 22 / 75 / 19, 22 / 72 / 19 and 17 / 73 / 17; first source
  byte at lo - 1 / lo / lo + 1: 570 / 568 / 486, 570 / 569 / 485 and 568 / 569 / 485;
  passes with a copy on both sides of lo: 1106, 1106 and 1119.
* all 9,520 (off, len, kind) triples of the overlap family at 4 or more phases with
  the two required ones, in each of the three; halves ending at 64 / 65 / 66 / 67 /
  68: 4611 / 3575 / 2851 / 2202 / 2029 (8192) and 1608 / 1611 / 1358 / 764 / 552
  (pass 2); batches with E = 64 and dropped elements 442, 467 and 22; batches under
  span_cut 220, 218 and 203.
* k4_literal_hbm: all 16 (dst & 3, src & 3) pairs, tails 0..3, 1-4 length bytes,
  ~2,990 calls in each, 1,762 / 1,763 / 2,864 with [F, kop) unflushed; 194 of 509
  bytes, 59-60 of each of 1023..4100, 51 of 8000.
* flushes: 5,112 at dst & 15 = 0 (8192), 311-327 at each of the 16 residues (8191);
  pass 2: 3,431 at dst & 15 = 0 and, one block modelled at each output shift of
  1..15 (the GPU test decodes the whole stream at all 16), 31-48 at each residue.

The bar: bit-exact against the oracle for every unit, the call succeeds, and the
64 sentinel bytes before and after the output are untouched."""
import collections
import functools

import numpy as np
import pytest

import datagen
import oracle
import snappy_amd
from golden_inputs import enc_copy, enc_literal, varint

BLOCK = 65536
RING, FLUSH_AT, FLUSH_GRAN, MAP_BITS = 4096, 2048, 1024, 1024  # kK4Ring, kK4FlushAt, kK4FlushGran, kK4MapBits
LONG_AT, HALF_AT = 508, 440
CHUNKS = [8192, 8191]
FAMILIES = ["overlap", "ring", "long", "span", "lanes"]
SENTINEL = 0xA5
KIND = {1: 1, 2: 2, 3: 4}  # element type -> enc_copy kind


# ---------------------------------------------------------------------------
# elements: ("L", n, width) a literal of n fresh bytes; ("C", len, off, kind) a
# copy; ("E", len, delta, kind) an edge copy: its offset is patched from the
# model's trace so that its first source byte is lo + delta
# ---------------------------------------------------------------------------
class Tape:
    """Fresh random bytes, each used once."""

    def __init__(self, seed: int, n: int):
        self.a = datagen.make("R", n, seed).tobytes()
        self.p = 0

    def take(self, n: int) -> bytes:
        b = self.a[self.p:self.p + n]
        assert len(b) == n, "tape exhausted"
        self.p += n
        return b


def out_len(ops) -> int:
    return sum(op[1] for op in ops)


def encode(ops, tape: Tape, at: int = 0):
    """-> the elements' bytes and {position of an edge copy (from `at`): (delta, kind)}."""
    body, edges = bytearray(), {}
    for op in ops:
        if op[0] == "L":
            body += enc_literal(tape.take(op[1]), op[2])
        elif op[0] == "C":
            body += enc_copy(op[1], op[2], op[3])
        else:
            edges[at + len(body)] = (op[2], op[3])
            body += enc_copy(op[1], 1, op[3])
    return bytes(body), edges


def filler(rng, n: int):
    """Literals of 1-60 bytes, n bytes in all."""
    ops = []
    while n:
        k = min(n, int(rng.integers(1, 61)))
        ops.append(("L", k, -1))
        n -= k
    return ops


def reset(rng):
    return ("L", 520 + int(rng.integers(0, 4)), 2)


def lits_of_size(x: int):
    """Literals of <= 60 bytes whose encoded sizes add up to x (>= 2)."""
    ops = []
    while x:
        s = 61 if x >= 63 or x == 61 else (x - 2 if x > 61 else x)
        ops.append(("L", s - 1, 0))
        x -= s
    return ops


# ---------------------------------------------------------------------------
# the families
# ---------------------------------------------------------------------------
def overlap_cases(seed: int):
    rng = np.random.default_rng(seed)
    need_a = collections.defaultdict(list)  # len -> items that still need phase + len > 64
    need_b = collections.defaultdict(list)  # off -> items that still need phase < off
    need_any = []
    for off in range(1, 71):
        for ln in range(1, 65):
            for kind in (2, 4) + ((1,) if 4 <= ln <= 11 else ()):
                item = (off, ln, kind)
                (need_a[ln] if ln >= 2 else need_any).append(item)
                need_b[off].append(item)
                need_any += [item, item]
    for v in list(need_a.values()) + list(need_b.values()):
        rng.shuffle(v)
    rng.shuffle(need_any)
    used = collections.defaultdict(set)
    left = sum(map(len, need_a.values())) + sum(map(len, need_b.values())) + len(need_any)

    def pick(phase: int):
        """An item whose open requirement this phase meets (the scarcest first)."""
        order = [0, 1, 2] if rng.integers(3) else [2, 0, 1]
        for which in order:
            if which < 2:  # (an item already placed at this phase has met the requirement: any phase will do)
                need = need_a if which == 0 else need_b
                for key in (range(max(2, 65 - phase), 65) if which == 0 else range(phase + 1, 71)):
                    while need[key]:
                        it = need[key].pop()
                        if phase not in used[it]:
                            return it
                        need_any.insert(0, it)
            else:
                for i in range(len(need_any) - 1, max(-1, len(need_any) - 40), -1):
                    if phase not in used[need_any[i]]:
                        return need_any.pop(i)
        return None

    cases, case = [], []
    while left:
        if out_len(case) + 530 + 1000 > 8191:
            cases.append(case)
            case = []
        case.append(("L", 509 + int(rng.integers(0, 12)), 2))  # a batch of its own; the group is the next
        pos = comp = nel = 0
        while left and pos < 930 and comp < 165 and nel < 58:
            seps = [int(s) for s in rng.permutation(3) + 1]
            if pos == 0:
                seps = [0] + seps  # the group's first copy may follow the long literal directly: phase 0
            for sep in seps:
                it = pick((pos + sep) % 64)
                if it:
                    break
            else:  # nothing fits: more literal bytes
                sep = int(rng.integers(1, 4))
                case.append(("L", sep, 0))
                pos, comp, nel = pos + sep, comp + sep + 1, nel + 1
                continue
            off, ln, kind = it
            used[it].add((pos + sep) % 64)
            if sep:
                case.append(("L", sep, 0))
                comp, nel = comp + sep + 1, nel + 1
            case.append(("C", ln, off, kind))
            pos, comp, nel = pos + sep + ln, comp + (2 if kind == 1 else 3 if kind == 2 else 5), nel + 1
            left -= 1
    cases.append(case)
    return cases


def ring_cases(seed: int):
    rng = np.random.default_rng(seed)
    cases = []
    for prefix in ("one", "small"):
        todo = [(off, ln) for off in range(3000, 4201)
                for ln in (1, 2, 63, 64, int(rng.integers(3, 63)))]
        rng.shuffle(todo)
        edge = [("E", ln, d) for _ in range(40) for ln in (1, 2, 7, 33, 63, 64) for d in (-1, 0, 1, "mid")]
        todo = todo + edge
        while todo:
            p = 4300 + int(rng.integers(0, 64))
            case = [("L", p, -1)] if prefix == "one" else filler(rng, p)
            total = p
            while todo and total + 3 + todo[-1][1] <= 8191:
                it = todo.pop()
                sep = int(rng.integers(1, 4))
                kind = 2 if rng.integers(2) else 4
                case.append(("L", sep, 0))
                if it[0] == "E":
                    d = -(it[1] // 2) if it[2] == "mid" else it[2]
                    case.append(("E", it[1], d, kind))
                else:
                    case.append(("C", it[1], it[0], kind))
                total += sep + it[1]
            cases.append(case)
    return cases


def after_copies(rng, kl: int, e_op: int):
    """Copies reaching 1, kl - 1, kl, 4095, 4096 and 4097 bytes back from a literal's end."""
    ops = []
    for off in (1, kl - 1, kl, 4095, 4096, 4097):
        sep = int(rng.integers(1, 4))
        ln = int(rng.integers(4, 12))
        if 1 <= off <= e_op:  # measured from the literal's end, then from wherever the copy stands
            ops += [("L", sep, 0), ("C", ln, off, 2 if off < 4095 else 4)]
            e_op += sep + ln
    return ops


def long_cases(seed: int):
    rng = np.random.default_rng(seed)
    cases = []
    for kl in (509, 1023, 1024, 1025, 4095, 4096, 4097, 4100, 8000):
        for width in (2, 3, 4):
            for j in range(5):          # literals before it in its batch (j = 0: the batch's first element)
                for a in range(4):      # bytes before it, mod 4
                    if j == 0 and kl == 8000 and a:
                        continue
                    case = [] if kl == 8000 else [("L", 520 + (0 if j else a), 2)]
                    if j:
                        p = 20 + a
                        cut = sorted(int(c) for c in rng.choice(np.arange(1, p), j - 1, replace=False))
                        case += [("L", y - x, 0) for x, y in zip([0] + cut, cut + [p])]
                    case.append(("L", kl, width))
                    case += after_copies(rng, kl, out_len(case))
                    cases.append(case)
    for s_nom in range(494, 519):  # e_lsrc + e_len = s_nom + o, o = 0..5 at the batch start
        for width in (1, 2, 3, 4):  # the k-th element of its batch
            x = 264 if width == 1 else 41
            case = [reset(rng)] + lits_of_size(x) + [("L", s_nom - x - 1 - width, width)]
            cases.append(case + after_copies(rng, case[-1][1], out_len(case)))
        for width in (2, 3, 4):     # the first
            case = [reset(rng), ("L", s_nom - 1 - width, width)]
            cases.append(case + after_copies(rng, case[-1][1], out_len(case)))
    for x in range(240, 262):  # a batch that starts at o = x + 0..5
        for kl, width in ((256, 1), (530, 2)):
            case = [reset(rng)] + lits_of_size(x) + [("L", kl, width)]
            cases.append(case + after_copies(rng, kl, out_len(case)))
    return cases


def span_cases(seed: int):
    rng = np.random.default_rng(seed)
    runs = {1023: [(0, [64] * 15 + [63]), (3, [64] * 15 + [60])],
            1024: [(0, [64] * 16), (2, [64] * 15 + [62])],
            1025: [(1, [64] * 16), (3, [64] * 15 + [62])]}
    cases = []
    for end, variants in runs.items():
        for x, lens in variants:
            for off in (1, 7, 63, 64, 200):
                case = [reset(rng)] + ([("L", x, 0)] if x else [])
                assert x + sum(lens) == end
                for i, ln in enumerate(lens + [64] * 40):
                    case.append(("C", ln, off, 4 if i % 5 == 4 else 2))
                cases.append(case)
    return cases


def lanes_cases(seed: int):
    rng = np.random.default_rng(seed)
    cases = []
    for _ in range(4):  # two-byte elements only
        case = [reset(rng)]
        for i in range(150):
            case.append(("L", 1, 0) if i % 2 == 0 or rng.integers(4) == 0
                        else ("C", int(rng.integers(4, 12)), int(rng.integers(1, 41)), 1))
        cases.append(case)
    for _ in range(12):  # 2/3/5-byte elements and short literals
        case = [reset(rng)]
        for i in range(220):
            r = int(rng.integers(10))
            if r < 2:
                case.append(("L", int(rng.integers(1, 5)), 0))
            elif r < 5:
                case.append(("C", int(rng.integers(4, 12)), int(rng.integers(1, 300)), 1))
            elif r < 8:
                case.append(("C", int(rng.integers(1, 20)), int(rng.integers(1, 500)), 2))
            else:
                case.append(("C", int(rng.integers(1, 20)), int(rng.integers(1, 500)), 4))
        cases.append(case)
    for h_nom in range(430, 447):  # hpos = h_nom + o after the literal's half
        case = [reset(rng), ("L", h_nom - 3, 2)]
        for i in range(60):
            case.append(("L", 1, 0) if i % 2 == 0 else ("C", 4 + i % 8, 1 + i % 40, 1))
        cases.append(case)
    return cases


@functools.lru_cache(maxsize=None)
def cases_of(family: str):
    fn = {"overlap": overlap_cases, "ring": ring_cases, "long": long_cases, "span": span_cases,
          "lanes": lanes_cases}[family]
    cases = fn(700 + FAMILIES.index(family))
    assert all(out_len(c) <= 8191 for c in cases), family
    return cases


# ---------------------------------------------------------------------------
# k4_body restated
# ---------------------------------------------------------------------------
class Stats:
    def __init__(self):
        self.n = collections.Counter()         # named events
        self.o_pre = collections.Counter()     # o at a batch start, before the slide / restart
        self.hexit = collections.Counter()     # where a half's last element ends (64..)
        self.hpos = collections.Counter()      # hpos where another half is considered (E < 64, no span_cut)
        self.lsum = collections.Counter()      # e_lsrc + e_len of the literals up to the first long one
        self.span_end = collections.Counter()  # out_off + e_len of 1023 / 1024 / 1025
        self.src_lo = collections.Counter()    # a copy's first source byte - lo (lo > 0), -1 / 0 / 1
        self.phases = collections.defaultdict(set)  # (off, len, kind) -> pass phases, off <= 70
        self.hbm_pairs = set()                 # k4_literal_hbm: (dst & 3, src & 3)
        self.hbm_tails = set()                 # its tail bytes
        self.hbm_widths = set()                # its header's length bytes
        self.hbm_lens = collections.Counter()
        self.flush_res = collections.Counter()  # dst & 15 of the ring flushes


def parse_element(byte, p: int):
    """(type, size, length, offset or literal header length) of the element at p,
    as snappy_oracle.c computes them (no wrap)."""
    tag = byte(p)
    t, m = tag & 3, tag >> 2
    if t == 0:
        k = max(m, 59) - 59
        lv = sum(byte(p + 1 + i) << (8 * i) for i in range(k)) if k else m
        return 0, lv + k + 2, lv + 1, 1 + k
    if t == 1:
        return 1, 2, (m & 7) + 4, ((tag >> 5) << 8) | byte(p + 1)
    if t == 2:
        return 2, 3, m + 1, byte(p + 1) | byte(p + 2) << 8
    return 3, 5, m + 1, byte(p + 1) | byte(p + 2) << 8 | byte(p + 3) << 16 | byte(p + 4) << 24


def k4_model(buf, c0: int, c1n: int, c_end: int, want: int, base: int, hdr, skip0: int, skip1: int,
             back: bool, dst16: int, S: Stats, trace=None, probe=None):
    """One unit through k4_body<back>: "ok", or "defer" (pass 1 only).  buf holds
    the stream at its true alignment (c0 includes the bias).  A refusal the kernel
    would return is an assertion here: the inputs are valid.  With probe = the
    position of a (hostile) element, the walk stops there and returns its lane in
    its batch."""
    c1 = min(c_end if skip1 else c1n, c_end)
    clen = c1 - c0
    tail_ip = c1n - c0 if skip1 and c0 <= c1n < c1 else -1

    def byte(x):
        return buf[c0 + x] if c0 + x < c1 else 0

    def flush(f, t):
        if t > f:
            S.flush_res[dst16 & 15] += 1
            S.n["flush_u32x4" if dst16 & 15 == 0 else "flush_bytes"] += 1

    def hbm(ip_data, kl, kop, width):
        d, s = dst16 + kop, c0 + ip_data
        S.hbm_pairs.add((d & 3, s & 3))
        S.hbm_tails.add((kl - min(-d & 3, kl)) & 3)
        S.hbm_widths.add(width)
        S.hbm_lens[kl] += 1

    B, ip, op, F = c0 & ~3, 0, 0, 0
    if hdr is not None:  # the preamble must declare hdr
        v = k = 0
        while True:
            b = byte(k)
            v |= (b & 0x7F) << (7 * k)
            k += 1
            if not b & 0x80:
                break
        assert v == hdr and not skip0
        ip = k
    if skip0:  # the unit starts inside the element at c0
        t, size, ln, info = parse_element(byte, 0)
        assert skip0 < ln and size <= clen
        k = min(ln - skip0, want)
        if t == 0:
            hbm(info + skip0, k, 0, info - 1)
            F = k
            S.n["resume_literal"] += 1
        elif not back:
            return "defer"
        else:
            assert info and info + skip0 <= base
            S.n["resume_copy"] += 1
            S.n["resume_copy_overlap"] += info < ln
        op, ip = k, size
    ip0, op0 = ip, op
    seq = []  # the executed elements
    span_cut = False
    while op < want:
        assert ip < clen
        o = c0 + ip - B
        S.o_pre[o] += 1
        if o >= 256:
            if o < 512:
                B, o = B + 256, o - 256
                S.n["slide"] += 1
            else:
                B = (c0 + ip) & ~3
                o = c0 + ip - B
                S.n["restart"] += 1

        def half(ho):
            p, out = ho, []
            while p < ho + 64:
                e = parse_element(byte, ip + p - o)
                out.append((p - o,) + e)
                p += e[1]
            assert len(out) <= 32
            return out, p - ho

        els, xa = half(o)
        S.hexit[xa] += 1
        E, hpos, dropped = len(els), o + xa, False
        S.n["batch_under_span_cut"] += span_cut
        for _ in (1, 2):
            if E < 64 and not span_cut:
                S.hpos[hpos] += 1
            if not (E < 64 and hpos <= HALF_AT) or span_cut:
                break
            eb, xb = half(hpos)
            S.hexit[xb] += 1
            dropped |= E + len(eb) > 64
            els += eb[:64 - E]
            E = len(els)
            hpos += xb
        S.n["E64"] += E == 64
        S.n["E64_dropped"] += E == 64 and dropped
        # the packed scan: sizes and lengths clamped to 1,023
        in_off, out_off, exact, a, b, x = [], [], [], 0, 0, 0
        for e in els:
            in_off.append(a & 0xFFFF)
            out_off.append(b & 0xFFFF)
            exact.append(x)
            a += min(e[2], 1023)
            b += min(e[3], 1023)
            x += e[3]
        lens = [e[3] for e in els]
        nexec = E
        for k, (rel, t, size, ln, info) in enumerate(els):
            e_ip, e_op = ip + in_off[k], op + out_off[k]
            if e_op >= want:
                nexec = k
                break
            if probe is not None and c0 + e_ip == probe:
                return k
            assert size <= clen - e_ip, "truncated"
            if back:
                if ln > want - e_op:
                    assert e_ip == tail_ip, "overrun"
                    lens[k] = want - e_op
                if t:
                    assert info, "offset 0"
                    if info > e_op:
                        assert info - e_op <= base, "offset"
                        S.n["e_back"] += 1
            else:
                if t and info - 1 >= e_op:
                    assert info, "offset 0"
                    return "defer"
                if ln > want - e_op:
                    assert e_ip == tail_ip and e_op == want - skip1, "overrun"
                    S.n["tail_element"] += 1
                    nexec = k + 1
                    break
        assert nexec, "no progress"
        for k in range(nexec):  # the scan is exact for every executed lane
            assert in_off[k] == els[k][0] and out_off[k] == exact[k], (k, in_off[k], out_off[k], els[k])
        long_k = None
        for k in range(nexec):
            if els[k][1] == 0:
                s = c0 + ip + in_off[k] - B + els[k][4] + lens[k]
                S.lsum[s] += 1
                if s > LONG_AT:
                    long_k = k
                    break
        direct = long_k == 0
        if direct:
            nexec = 1
            kl = min(lens[0], want - op)
            S.n["hbm_literal"] += 1
            S.n["hbm_literal_unflushed"] += op > F
            flush(F, op)
            hbm(ip + els[0][4], kl, op, els[0][4] - 1)
            F = op + kl
        else:
            if long_k is not None:
                nexec = long_k
                S.n["long_cut"] += 1
            over = None
            for k in range(nexec):
                end = out_off[k] + lens[k]
                if end in (1023, 1024, 1025):
                    S.span_end[end] += 1
                if k and end > MAP_BITS:
                    over = k
                    break
            if over is not None:
                nexec = over
                S.n["span_cut"] += 1
            span_cut = over is not None
            op_end = min(op + out_off[nexec - 1] + lens[nexec - 1], want)
            lo = max(op_end - RING, 0)
            assert op_end - F <= RING - 64, "the ring holds [F, op_end)"
            for k in range(nexec):
                rel, t, size, ln, off = els[k]
                if t == 0:
                    continue
                e_op = op + out_off[k]
                e_end = min(e_op + lens[k], op_end)
                phase = (e_op - op) % 64
                if off <= 70:
                    S.phases[(off, ln, KIND[t])].add(phase)
                if trace is not None:
                    trace.append((c0 + ip + in_off[k], e_op, lo))
                if lo and e_op - off - lo in (-1, 0, 1):
                    S.src_lo[e_op - off - lo] += 1
                S.n["copy_overlap"] += off < e_end - e_op
                any_far = any_in = False
                for P in range(e_op - phase, e_end, 64):  # its passes
                    sa, sb = max(P, e_op), min(P + 64, e_end)
                    if off >= 64 + 64:  # neither overlapping nor in this pass
                        far = min(max(lo + off - sa, 0), sb - sa)
                        near_in = False
                    else:
                        far, near_in = 0, False
                        for x in range(sa, sb):
                            d = x - e_op
                            src = x - off if d < off else e_op - off + d % off
                            if src < lo:  # (pass 2: an overlapping copy repeating bytes of an earlier unit)
                                far += 1
                                S.n["overlap_far"] += d >= off
                            elif src >= P:
                                near_in = True
                    any_far |= far > 0
                    any_in |= near_in
                    S.n["pass_lo_both_sides"] += 0 < far < sb - sa
                S.n["copy_far"] += any_far
                S.n["copy_in_pass"] += any_in
        seq += [(ip + in_off[k], op + out_off[k]) for k in range(nexec)]
        ip += in_off[nexec - 1] + els[nexec - 1][2]
        op = min(op + out_off[nexec - 1] + els[nexec - 1][3], want)
        if op - F >= FLUSH_AT:
            T = op & ~(FLUSH_GRAN - 1)
            flush(F, T)
            F = T
    flush(F, op)
    assert op == want
    # the serial walk
    walk, x, y = [], ip0, op0
    while y < want:
        _, size, ln, _ = parse_element(byte, x)
        walk.append((x, y))
        x, y = x + size, y + ln
    assert seq == walk, "the batches execute the serial element walk"
    assert y == want or (tail_ip >= 0 and walk[-1][0] == tail_ip), "the unit ends at its length"
    return "ok"


def patch_edges(buf: bytearray, edges: dict, trace) -> int:
    """Set every edge copy's offset so that its first source byte is lo + delta."""
    done = 0
    for pos, e_op, lo in trace:
        if pos in edges and lo:
            delta, kind = edges[pos]
            off = e_op - lo - delta
            assert 1 <= off <= e_op and off < 65536
            buf[pos + 1:pos + 3] = off.to_bytes(2, "little")
            done += 1
    return done


# ---------------------------------------------------------------------------
# the STREAMS inputs (pass 1): a case per unit
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def streams_input(family: str, chunk: int):
    """-> payload (uint8), offsets (int64), unit count, model statistics."""
    cases = cases_of(family)
    rng = np.random.default_rng(800 + FAMILIES.index(family) + chunk)
    tape = Tape(900 + FAMILIES.index(family) + chunk, len(cases) * chunk + 4096)
    buf, offs, edges = bytearray(), [0], {}
    for case in cases:
        buf += varint(chunk)
        body, e = encode(case + filler(rng, chunk - out_len(case)), tape, len(buf))
        edges.update(e)
        buf += body
        offs.append(len(buf))
    for rounds in range(2 if edges else 1):
        S, trace = Stats(), []
        for u in range(len(cases)):
            r = k4_model(buf, offs[u], offs[u + 1], offs[-1], chunk, u * chunk, chunk, 0, 0, False,
                         (u * chunk) & 15, S, trace if edges and rounds == 0 else None)
            assert r == "ok", (family, chunk, u)
        if edges and rounds == 0:
            assert patch_edges(buf, edges, trace) >= len(edges) * 3 // 4
    payload = np.frombuffer(bytes(buf), dtype=np.uint8)
    return payload, np.array(offs, dtype=np.int64), len(cases), S


@functools.lru_cache(maxsize=None)
def streams_want(family: str, chunk: int) -> np.ndarray:
    payload, offs, units, _ = streams_input(family, chunk)
    out = oracle.decompress_streams(payload, offs.astype(np.uint64), units * chunk, chunk)
    out.setflags(write=False)
    return out


# ---------------------------------------------------------------------------
# the SINGLE input (pass 2): the same cases in 65,536-byte blocks
# ---------------------------------------------------------------------------
def host_index(stream: bytes):
    """The block index by the element walk: bits [0, 40) the offset of the element
    holding the block's first byte, bits [40, 64) how many of its bytes precede it."""
    def byte(x):
        return stream[x]
    n = k = 0
    while True:
        b = stream[k]
        n |= (b & 0x7F) << (7 * k)
        k += 1
        if not b & 0x80:
            break
    entries, x, op, nb = [0], k, 0, BLOCK
    while op < n:
        _, size, ln, _ = parse_element(byte, x)
        while nb < op + ln and nb < n:
            entries.append(x | (nb - op) << 40)
            nb += BLOCK
        x, op = x + size, op + ln
    assert op == n
    entries.append(x)
    return n, entries


@functools.lru_cache(maxsize=None)
def single_input():
    """-> stream (uint8), index (int64), n, pass-1 statistics of block 0, pass-2 statistics."""
    rng = np.random.default_rng(850)
    ops, out, v = filler(rng, 60000), 60000, 0  # block 0 (pass 1) holds no case

    def boundary(nb: int):
        """Filler up to the block boundary nb and the elements around it."""
        nonlocal v
        kind = v % 8
        v += 1
        k = int(rng.integers(1, 60))  # bytes of a straddling element before the boundary
        gap = nb - out - (k if kind >= 3 else 0)
        b = filler(rng, gap)
        if kind == 0:    # a plain copy reaching back
            b.append(("C", int(rng.integers(4, 65)), int(rng.integers(64, 60000)), 4))
        elif kind == 1:  # an overlapping copy at the boundary
            off = int(rng.integers(1, 64))
            b.append(("C", int(rng.integers(off + 1, 65)), off, 2))
        elif kind == 2:  # an overlapping copy beginning within off bytes after it
            off = int(rng.integers(2, 64))
            j = int(rng.integers(1, off))
            b += [("C", j, int(rng.integers(100, 5000)), 2), ("C", int(rng.integers(off + 1, 65)), off, 4)]
        elif kind == 3:  # a straddling copy
            b.append(("C", 64, int(rng.integers(64, 70000)), 4))
        elif kind == 4:  # a straddling overlapping copy
            b.append(("C", 64, int(rng.integers(1, 60)), 2))
        else:            # a straddling literal, then a copy reaching back over it
            ln = (k + 1 + int(rng.integers(0, 40)), 600, 1500)[kind - 5]
            b += [("L", ln, -1), ("C", 12, ln + 7, 4)]
        return b

    cases = [c for f in FAMILIES for c in cases_of(f)]
    order = np.random.default_rng(851).permutation(len(cases))
    for i in order:
        case = cases[i]
        nb = (out // BLOCK + 1) * BLOCK
        if out + out_len(case) + 200 > nb:
            b = boundary(nb)
            ops += b
            out += out_len(b)
        ops += case
        out += out_len(case)
    ops += filler(rng, 300)
    n = out + 300
    tape = Tape(950, n + 4096)
    body, edges = encode(ops, tape, len(varint(n)))
    buf = bytearray(varint(n) + body)
    n2, entries = host_index(bytes(buf))
    assert n2 == n
    units = (n + BLOCK - 1) // BLOCK
    assert len(entries) == units + 1
    mask = (1 << 40) - 1
    for rounds in range(2):
        S1, S2, trace, deferred = Stats(), Stats(), [], 0
        for u in range(units):
            want = min(BLOCK, n - u * BLOCK)
            args = (buf, entries[u] & mask, entries[u + 1] & mask, entries[-1], want, u * BLOCK, n if u == 0 else None,
                    entries[u] >> 40, entries[u + 1] >> 40)
            r = k4_model(*args, False, 0, Stats() if u else S1, trace if u == 0 and rounds == 0 else None)
            if r == "defer":
                deferred += 1
                assert k4_model(*args, True, 0, S2, trace if rounds == 0 else None) == "ok"
        assert deferred == units - 1, "every block after the first goes to pass 2"
        if rounds == 0:
            assert patch_edges(buf, edges, trace) >= len(edges) * 3 // 4
    S2.n["blocks"] = deferred
    # decoded into an output s_out = 1..15 bytes off a 16-byte boundary (every block's dst
    # has that residue): one block per s_out is enough to show its flushes
    for r in range(1, 16):
        u = 1 + r
        args = (buf, entries[u] & mask, entries[u + 1] & mask, entries[-1], BLOCK, u * BLOCK, None, entries[u] >> 40,
                entries[u + 1] >> 40)
        S = Stats()
        assert k4_model(*args, True, r, S) == "ok"
        S2.flush_res.update(S.flush_res)
        S2.hbm_pairs |= S.hbm_pairs
    stream = np.frombuffer(bytes(buf), dtype=np.uint8)
    return stream, np.array(entries, dtype=np.int64), n, S1, S2


# ---------------------------------------------------------------------------
# the CPU proof
# ---------------------------------------------------------------------------
def merged(stats):
    S = Stats()
    for s in stats:
        for name, v in vars(s).items():
            mine = getattr(S, name)
            if isinstance(v, collections.Counter):
                mine.update(v)
            elif isinstance(v, set):
                mine |= v
            else:
                for key, ph in v.items():
                    mine[key] |= ph
    return S


def check_conditions(S: Stats, what: str, residues):
    n = S.n
    both = {"o at a batch start 255 | 256": (S.o_pre, 255, 256),
            "o at a batch start 511 | 512": (S.o_pre, 511, 512),
            "hpos 440 | 441": (S.hpos, 440, 441),
            "e_lsrc + e_len 508 | 509": (S.lsum, 508, 509),
            "batch output 1024 | 1025": (S.span_end, 1024, 1025),
            "batch output 1023": (S.span_end, 1023, 1023),
            "copy source lo - 1 | lo": (S.src_lo, -1, 0),
            "copy source lo + 1": (S.src_lo, 1, 1)}
    for name, (c, a, b) in both.items():
        print(f"  {what}: {name}: {c[a]} | {c[b]}")
        assert c[a] >= 1 and c[b] >= 1, (what, name)
    print(f"  {what}: e_lsrc + e_len:", {s: S.lsum[s] for s in range(500, 517)})
    assert all(S.lsum[s] for s in range(500, 517)), what
    print(f"  {what}: a half's last element ends at:", {x: S.hexit[x] for x in range(64, 69)})
    assert all(S.hexit[x] for x in range(64, 69)), what
    # the overlap family: every pair and encoding at the phases required
    short = []
    for off in range(1, 71):
        for ln in range(1, 65):
            for kind in (2, 4) + ((1,) if 4 <= ln <= 11 else ()):
                ph = S.phases[(off, ln, kind)]
                if not (len(ph) >= 4 and (ln == 1 or any(p + ln > 64 for p in ph)) and any(p < off for p in ph)):
                    short.append((off, ln, kind, sorted(ph)))
    print(f"  {what}: overlap (off, len, kind) triples:", sum(1 for k in S.phases if k[0] <= 70),
          "missing a required phase:", len(short))
    assert not short, (what, short[:5])
    print(f"  {what}: k4_literal_hbm (dst & 3, src & 3) pairs {len(S.hbm_pairs)}, tails {sorted(S.hbm_tails)}, "
          f"length bytes {sorted(S.hbm_widths)}, with [F, kop) unflushed {n['hbm_literal_unflushed']} of "
          f"{n['hbm_literal']}, lengths", {k: S.hbm_lens[k] for k in (509, 1023, 1024, 1025, 4095, 4096, 4097,
                                                                    4100, 8000)})
    assert len(S.hbm_pairs) == 16 and S.hbm_tails == {0, 1, 2, 3} and S.hbm_widths >= {1, 2, 3, 4}, what
    assert n["hbm_literal_unflushed"] >= 16 and n["long_cut"] >= 16, what
    assert all(S.hbm_lens[k] for k in (509, 1023, 1024, 1025, 4095, 4096, 4097, 4100, 8000)), what
    print(f"  {what}: flushes by dst & 15:", dict(sorted(S.flush_res.items())))
    assert all(S.flush_res[r] for r in residues), what
    for name in ("pass_lo_both_sides", "E64_dropped", "batch_under_span_cut", "span_cut", "copy_far",
                 "copy_overlap", "copy_in_pass", "slide", "restart", "long_cut"):
        print(f"  {what}: {name}: {n[name]}")
        assert n[name] >= 1, (what, name)


def test_inputs_have_their_properties():
    """No GPU: k4_model() runs every input (its batches execute the serial walk and
    end at the unit's length) and every edge named in the module docstring is
    reached, in the pass-1 inputs and in the pass-2 inputs."""
    per = {}
    for chunk in CHUNKS:
        for family in FAMILIES:
            payload, offs, units, S = streams_input(family, chunk)
            per[(family, chunk)] = S
            print(f"STREAMS {family} chunk {chunk}: {units} units, {payload.size} bytes, batches under span_cut "
                  f"{S.n['batch_under_span_cut']}, E = 64 with drops {S.n['E64_dropped']}, far copies "
                  f"{S.n['copy_far']}, passes on both sides of lo {S.n['pass_lo_both_sides']}, HBM literals "
                  f"{S.n['hbm_literal']}, flushes {sum(S.flush_res.values())}")
            want = streams_want(family, chunk)
            assert want.size == units * chunk
    for chunk in CHUNKS:
        print(f"pass 1, chunk {chunk}:")
        check_conditions(merged(per[(f, chunk)] for f in FAMILIES), f"pass 1 / {chunk}",
                         range(16) if chunk % 16 else [0])
    stream, index, n, S1, S2 = single_input()
    print(f"SINGLE: {n} bytes in {index.size - 1} blocks, {S2.n['blocks']} through pass 2; resumed literals "
          f"{S2.n['resume_literal']}, copies {S2.n['resume_copy']} (overlapping {S2.n['resume_copy_overlap']}), "
          f"copies into earlier blocks {S2.n['e_back']}, overlapping copies repeating earlier blocks' bytes "
          f"{S2.n['overlap_far']}")
    assert n <= 64 << 20
    assert len(oracle.decompress(stream.tobytes())) == n
    assert S2.n["resume_literal"] >= 3 and S2.n["resume_copy"] >= 3 and S2.n["resume_copy_overlap"] >= 1
    assert S2.n["overlap_far"] >= 3 and S2.n["e_back"] >= S2.n["blocks"] // 2
    print("pass 2:")
    check_conditions(S2, "pass 2", range(16))


# ---------------------------------------------------------------------------
# the GPU tests
# ---------------------------------------------------------------------------
def decode_guarded(codec, comp, offs, n, chunk, layout, s_in=0, s_out=0):
    """Decode into a buffer with 64 sentinel bytes on both sides -> the output (numpy)."""
    import torch
    d = torch.zeros(comp.size + 8, dtype=torch.uint8, device="cuda")
    d[s_in:s_in + comp.size] = torch.from_numpy(np.array(comp))
    o = torch.from_numpy(np.array(offs, dtype=np.int64)).cuda()
    buf = torch.full((n + 128 + 16,), SENTINEL, dtype=torch.uint8, device="cuda")
    out = buf[64 + s_out:64 + s_out + n]
    back = codec.decompress_tensor(d[s_in:s_in + comp.size], o, n, chunk=chunk, layout=layout, out=out)
    assert back.data_ptr() == out.data_ptr()
    got = buf.cpu().numpy()
    assert (got[:64 + s_out] == SENTINEL).all() and (got[64 + s_out + n:] == SENTINEL).all(), "sentinels"
    return got[64 + s_out:64 + s_out + n]


def assert_units_equal(got, want, chunk, what):
    if not np.array_equal(got, want):
        bad = np.flatnonzero(got != want)
        units = np.unique(bad // chunk)
        raise AssertionError(f"{what}: {units.size} units differ, first unit {units[0]} at byte "
                             f"{bad[0] % chunk} of it")


@pytest.mark.gpu
@pytest.mark.parametrize("chunk", CHUNKS)
@pytest.mark.parametrize("family", FAMILIES)
def test_streams_planted(codec, family, chunk):
    """Pass 1: every case its own unit, thousands of units in one launch."""
    payload, offs, units, _ = streams_input(family, chunk)
    got = decode_guarded(codec, payload, offs, units * chunk, chunk, snappy_amd.STREAMS)
    assert_units_equal(got, streams_want(family, chunk), chunk, (family, chunk))


@pytest.mark.gpu
@pytest.mark.parametrize("family", FAMILIES)
def test_streams_planted_alignment(codec, family):
    """A subset of every family from a stream 0-3 bytes into its dword (bias) and
    into an output 0-15 bytes off a 16-byte boundary."""
    for chunk in CHUNKS:
        payload, offs, units, _ = streams_input(family, chunk)
        pick = min(units, 24)
        first = (units - pick) // 2 if family == "long" else 0
        sub = payload[offs[first]:offs[first + pick]]
        so = offs[first:first + pick + 1] - offs[first]
        want = streams_want(family, chunk)[first * chunk:(first + pick) * chunk]
        # every s_out at two residues of s_in
        for s_in, s_out in [(s_out & 3, s_out) for s_out in range(16)] + [((s_out + 1) & 3, s_out) for s_out in range(16)]:
            got = decode_guarded(codec, sub, so, pick * chunk, chunk, snappy_amd.STREAMS, s_in, s_out)
            assert_units_equal(got, want, chunk, (family, chunk, s_in, s_out))


@functools.lru_cache(maxsize=None)
def single_want() -> np.ndarray:
    return np.frombuffer(oracle.decompress(single_input()[0].tobytes()), dtype=np.uint8)


@pytest.mark.gpu
def test_single_planted_index(codec):
    """The host-built index of the SINGLE stream is what the device indexes."""
    import torch
    stream, index, n, _, _ = single_input()
    n_dev, offs_dev = codec.index_tensor(torch.from_numpy(np.array(stream)).cuda())
    assert n_dev == n and np.array_equal(offs_dev.cpu().numpy(), index)


@pytest.mark.gpu
@pytest.mark.parametrize("s_out", [0, 4, 8, 12])
def test_single_planted_pass2(codec, s_out):
    """Pass 2: the same cases in one stream whose blocks all copy from earlier ones,
    decoded with the host-built index into outputs 0-15 bytes off a 16-byte
    boundary (s_out .. s_out + 3, the stream 0-3 bytes into its dword)."""
    stream, index, n, _, _ = single_input()
    for k in range(4):
        got = decode_guarded(codec, stream, index, n, BLOCK, snappy_amd.SINGLE, (k + s_out // 4) & 3, s_out + k)
        assert_units_equal(got, single_want(), BLOCK, ("SINGLE", s_out + k))


# ---------------------------------------------------------------------------
# hostile lengths and refusals
# ---------------------------------------------------------------------------
HCHUNK = 8192


def lit4(declared: int) -> bytes:
    """The header of a literal declaring `declared` bytes in four length bytes."""
    return bytes([63 << 2]) + ((declared - 1) & 0xFFFFFFFF).to_bytes(4, "little")


def hostile_bodies():
    """name -> (elements' bytes of one 8,192-byte unit with one hostile element,
    the error code where it is unambiguous).  Around the hostile element the unit
    is complete: a decoder that skipped it would end at 8,192 bytes."""
    tape = Tape(990, 1 << 20)
    rng = np.random.default_rng(991)

    def enc(ops):
        return encode(ops, tape)[0]

    def rest(n):  # n bytes of small elements
        return enc(filler(rng, n))

    cases = {}

    def put(name, head, hostile, tail, code=None, lane0=None):
        """lane0: the hostile literal must (True) / must not (False) start its batch."""
        cases[name] = (head + hostile + tail, code, len(head), lane0)

    for declared, name in ((1 << 32, "2^32"), ((1 << 32) - 1, "2^32-1"), ((1 << 32) - 5, "2^32-5"),
                           (1 << 31, "2^31"), (1 << 24, "2^24")):
        put(f"literal {name} first", b"", lit4(declared), rest(HCHUNK), None, True)
        put(f"literal {name} after", enc([("L", 90, 1), ("L", 10, 0)]), lit4(declared), rest(HCHUNK - 100), None, False)
        put(f"literal {name} second after a long literal", enc([("L", 600, 2), ("L", 5, 0)]), lit4(declared),
            rest(HCHUNK - 605), None, False)
        # the 600-byte literal is a batch of its own (k4_literal_hbm): the next batch starts here
        put(f"literal {name} batch-first after a long literal", enc([("L", 600, 2)]), lit4(declared),
            rest(HCHUNK - 600), None, True)
    for kind in (1, 2, 4):
        put(f"copy-{kind} offset 0", rest(300), enc_copy(8, 0, kind), rest(HCHUNK - 308), snappy_amd.ERR_OFFSET)
    for kind in (1, 2, 4):
        put(f"copy-{kind} cut short", rest(HCHUNK - 8), enc_copy(8, 100, kind)[:-1], b"")
    for width in (0, 1, 4):
        put(f"literal width {width} cut short", rest(HCHUNK - 40), enc([("L", 40, width)])[:-1], b"")
        put(f"literal width {width} overrun", rest(HCHUNK - 40), enc([("L", 41, width)]), b"")
    put("control", b"", b"", rest(HCHUNK))
    return cases


def streams_only_bodies():
    """Copy offsets against the unit's start, which only a STREAMS unit has: e_op
    (legal, reaches byte 0) and e_op + 1, inside the unit and as its first element
    (offsets 0 and 1 at e_op = 0)."""
    tape = Tape(996, 1 << 19)
    rng = np.random.default_rng(997)

    def rest(n):
        return encode(filler(rng, n), tape)[0]

    cases = {}
    for kind in (1, 2, 4):
        cases[f"copy-{kind} offset e_op"] = (rest(300) + enc_copy(8, 300, kind) + rest(HCHUNK - 308), None, 0, None)
        for name, off, head in (("e_op + 1", 301, 300), ("0 first", 0, 0), ("e_op + 1 first", 1, 0)):
            cases[f"copy-{kind} offset {name}"] = (rest(head) + enc_copy(8, off, kind) + rest(HCHUNK - head - 8),
                                                   snappy_amd.ERR_OFFSET, 0, None)
    return cases


def oracle_accepts(unit: bytes, n: int):
    try:
        w = oracle.decompress(unit)
    except ValueError:
        return None
    return w if len(w) == n else None


def gpu_decode(codec, comp: bytes, offs, n, chunk, layout):
    """-> (output bytes, 0) or (None, error code)."""
    try:
        got = decode_guarded(codec, np.frombuffer(comp, dtype=np.uint8), np.array(offs, dtype=np.int64), n, chunk,
                             layout)
    except snappy_amd.SnappyError as e:
        return None, e.code
    return got.tobytes(), 0


@pytest.mark.gpu
def test_hostile_streams(codec):
    """STREAMS: five units per launch, the hostile one in the middle."""
    tape = Tape(992, 1 << 20)
    rng = np.random.default_rng(993)
    good = [varint(HCHUNK) + encode(filler(rng, HCHUNK), tape)[0] for _ in range(4)]
    bodies = {**hostile_bodies(), **streams_only_bodies()}
    cases = {name: (varint(HCHUNK) + body, code, at, lane0) for name, (body, code, at, lane0) in bodies.items()}
    body = bodies["control"][0]
    cases["preamble chunk + 1"] = (varint(HCHUNK + 1) + body, snappy_amd.ERR_HEADER, 0, None)
    cases["preamble chunk - 1"] = (varint(HCHUNK - 1) + body, snappy_amd.ERR_HEADER, 0, None)
    accepted = refused = 0
    for name, (unit, code, at, lane0) in cases.items():
        units = good[:2] + [unit] + good[2:]
        offs = [0]
        for u in units:
            offs.append(offs[-1] + len(u))
        want = [oracle_accepts(u, HCHUNK) for u in units]
        assert all(w is not None for i, w in enumerate(want) if i != 2)
        if lane0 is not None:  # where the hostile literal stands in its batch
            lane = k4_model(b"".join(units), offs[2], offs[3], offs[-1], HCHUNK, 2 * HCHUNK, HCHUNK, 0, 0, False, 0,
                            Stats(), None, offs[2] + len(varint(HCHUNK)) + at)
            assert (lane == 0) == lane0, (name, lane)
        got, rc = gpu_decode(codec, b"".join(units), offs, 5 * HCHUNK, HCHUNK, snappy_amd.STREAMS)
        print(f"STREAMS {name}: oracle {'accepts' if want[2] is not None else 'refuses'}, GPU rc {rc}")
        assert (got is not None) == (want[2] is not None), name
        if got is not None:
            assert got == b"".join(want), name
            accepted += 1
        else:
            refused += 1
            if code is not None:
                assert rc == code, (name, rc)
    assert accepted >= 4 and refused >= 30


def single_hostile(body: bytes, tape, rng, defer: bool, at: int = 20000):
    """One stream of three blocks, `body` (8,192 bytes of elements, one hostile)
    `at` bytes into block 1 -> stream, index built from the intended elements,
    n, the body's position in the stream."""
    n = 3 * BLOCK
    first = [("C", 8, 77, 2)] if defer else [("L", 8, 0)]  # block 1 through pass 2 / pass 1
    b0 = encode(filler(rng, BLOCK), tape)[0]
    lead = encode(first + filler(rng, at - 8), tape)[0] if at else b""
    b1 = lead + body + encode(filler(rng, BLOCK - at - HCHUNK), tape)[0]
    b2 = encode(filler(rng, BLOCK), tape)[0]
    head = varint(n)
    stream = head + b0 + b1 + b2
    index = [0, len(head) + len(b0), len(head) + len(b0) + len(b1), len(stream)]
    return stream, index, n, len(head) + len(b0) + len(lead)


def single_copy_cases(tape, rng):
    """name -> (stream, n, must be accepted): copy-4 whose offset is its global
    output position (legal, reaches byte 0 of the stream) and that + 1, as an
    element inside block 1 (after a literal: pass 1 defers at it; after a copy
    into block 0: pass 2 from the block's start), as block 1's first element, as a
    copy straddling into block 1 (resumed with skip0 = 9), and at positions 0 and 1
    as block 0's first element."""
    n = 3 * BLOCK

    def enc(ops):
        return encode(ops, tape)[0]

    cases = {}
    for d in (0, 1):
        what = "position" if d == 0 else "position + 1"
        for first, pas in ((("L", 8, 0), "pass 1 defers"), (("C", 8, 77, 2), "pass 2")):
            g = BLOCK + 20000
            cases[f"copy-4 inside block 1, offset its {what}, {pas}"] = (
                varint(n) + enc(filler(rng, BLOCK) + [first] + filler(rng, 20000 - 8) + [("C", 8, g + d, 4)] +
                                filler(rng, 2 * BLOCK - 20008)), d == 0)
        cases[f"copy-4 starting block 1, offset its {what}"] = (
            varint(n) + enc(filler(rng, BLOCK) + [("C", 8, BLOCK + d, 4)] + filler(rng, 2 * BLOCK - 8)), d == 0)
        cases[f"copy-4 straddling into block 1, offset its {what}"] = (
            varint(n) + enc(filler(rng, BLOCK - 9) + [("C", 30, BLOCK - 9 + d, 4)] + filler(rng, 2 * BLOCK - 21)), d == 0)
        cases[f"copy-4 starting block 0, offset {d}"] = (varint(n) + enc([("C", 8, d, 4)] + filler(rng, n - 8)), False)
    return {name: (stream, n, ok) for name, (stream, ok) in cases.items()}


@pytest.mark.gpu
def test_hostile_single(codec):
    """SINGLE with a caller-supplied index, the hostile element in block 1 of 3,
    decoded by pass 1 and (the block starting with a copy into block 0) by pass 2;
    the host API, which indexes the stream itself, refuses and accepts the same."""
    tape = Tape(994, 24 << 20)
    rng = np.random.default_rng(995)
    accepted = refused = 0
    for name, (body, code, at, lane0) in hostile_bodies().items():
        if "cut short" in name or "overrun" in name:
            continue  # at the stream's end below
        first = name.endswith(" first")  # as block 1's first element: pass 1 only
        for defer in (False,) if first else (False, True):
            stream, index, n, pos = single_hostile(body, tape, rng, defer, 0 if first else 20000)
            want = oracle_accepts(stream, n)
            if lane0 is not None:  # where the hostile literal stands in its batch
                lane = k4_model(stream, index[1], index[2], index[3], BLOCK, BLOCK, None, 0, 0, defer, 0, Stats(), None,
                                pos + at)
                assert (lane == 0) == lane0, (name, defer, lane)
            got, rc = gpu_decode(codec, stream, index, n, BLOCK, snappy_amd.SINGLE)
            try:
                host = snappy_amd.decompress(stream)
            except snappy_amd.SnappyError as e:
                host = None
                assert code is None or e.code == code, (name, e.code)
            print(f"SINGLE {name} pass {2 if defer else 1}: oracle {'accepts' if want is not None else 'refuses'}, "
                  f"GPU rc {rc}, host API {'accepts' if host is not None else 'refuses'}")
            assert (got is not None) == (want is not None), (name, defer)
            assert (host is not None) == (want is not None), (name, defer, "host API")
            if want is not None:
                assert got == want and host == want, (name, defer)
                accepted += 1
            else:
                refused += 1
                if code is not None:
                    assert rc == code, (name, rc)
    # copy offsets at and one past the stream's first byte (k4_body<true>'s back_lim, the resume path)
    for name, (stream, n, ok) in single_copy_cases(tape, rng).items():
        index = host_index(stream)[1]
        want = oracle_accepts(stream, n)
        assert (want is not None) == ok, name
        got, rc = gpu_decode(codec, stream, index, n, BLOCK, snappy_amd.SINGLE)
        try:
            host = snappy_amd.decompress(stream)
        except snappy_amd.SnappyError:
            host = None
        print(f"SINGLE {name}: oracle {'accepts' if ok else 'refuses'}, GPU rc {rc}, "
              f"host API {'accepts' if host is not None else 'refuses'}")
        assert (got is not None) == ok and (host is not None) == ok, name
        if ok:
            assert got == want == host, name
            accepted += 1
        else:
            assert rc == snappy_amd.ERR_OFFSET, (name, rc)
            refused += 1
    # the stream's last element cut short / overrunning, and the preamble off by one
    n = BLOCK + 5000
    ends = {"control": (encode([("L", 40, 0)], tape)[0], n, None)}
    for kind in (1, 2, 4):
        ends[f"copy-{kind} cut short"] = (encode([("L", 32, 0)], tape)[0] + enc_copy(8, 100, kind)[:-1], n, None)
    for width in (0, 1, 4):
        ends[f"literal width {width} cut short"] = (encode([("L", 40, width)], tape)[0][:-1], n, None)
        ends[f"literal width {width} overrun"] = (encode([("L", 41, width)], tape)[0], n, None)
    ends["preamble n + 1"] = (ends["control"][0], n + 1, snappy_amd.ERR_HEADER)
    ends["preamble n - 1"] = (ends["control"][0], n - 1, snappy_amd.ERR_HEADER)
    for name, (tail, declared, code) in ends.items():
        b0 = encode(filler(rng, BLOCK), tape)[0]
        b1 = encode(filler(rng, 5000 - 40), tape)[0] + tail
        head = varint(declared)
        stream = head + b0 + b1
        index = [0, len(head) + len(b0), len(stream)]
        want = oracle_accepts(stream, declared)
        got, rc = gpu_decode(codec, stream, index, n, BLOCK, snappy_amd.SINGLE)  # the caller says n
        try:
            host = snappy_amd.decompress(stream)
        except snappy_amd.SnappyError:
            host = None
        print(f"SINGLE end {name}: oracle {'accepts' if want is not None else 'refuses'}, GPU rc {rc}, "
              f"host API {'accepts' if host is not None else 'refuses'}")
        ok = want is not None and declared == n
        assert (got is not None) == ok, name
        assert (host is not None) == (want is not None), (name, "host API")
        if ok:
            assert got == want == host, name
            accepted += 1
        else:
            refused += 1
            if code is not None:
                assert rc == code, (name, rc)
    assert accepted >= 4 and refused >= 30

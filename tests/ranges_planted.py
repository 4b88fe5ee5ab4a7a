"""Builders, byte-stream models and the GPU call of tests/test_ranges_planted.py.

The planted element streams are test_k4_decode's (imported, not copied): its
STREAMS inputs as they are, and its cases once more as a SINGLE stream whose
blocks are mostly *independent* (single_independent_input), because range decode
has no second pass and refuses every dependent block."""
import collections
import functools

import numpy as np

import oracle
import test_k4_decode as k4

BLOCK = k4.BLOCK
MASK = (1 << 40) - 1
SENT = 0xA5
GUARD = 64
OK, ERR_ARG, ERR_TRUNCATED, ERR_CAPACITY, ERR_DEPENDENT = 0, -1, -3, -6, -13
EARLY = (ERR_ARG, ERR_CAPACITY, ERR_TRUNCATED)  # refused before any load or store

# The boundary at each block's end, in this order (an event "d" makes two blocks of
# kind d).  A straddling element (b, c, d, e) always starts in a block that is not
# dependent: after a dependent block (e, f, g) comes a, f or g.
CYCLE = ["a", "e1", "f", "a", "b", "e2", "g", "a", "c1", "e4", "a", "c2", "c3", "c4", "d", "b"]
KINDS = "abcdefg"


# ---------------------------------------------------------------------------
# the byte stream's elements, and the dependency rule on them
# ---------------------------------------------------------------------------
def walk(stream: bytes):
    """-> n, [(position, output position, type, size, length, offset or header length)]"""
    n = k = 0
    while True:
        b = stream[k]
        n |= (b & 0x7F) << (7 * k)
        k += 1
        if not b & 0x80:
            break
    byte, x, op, out = stream.__getitem__, k, 0, []
    while op < n:
        t, size, ln, info = k4.parse_element(byte, x)
        out.append((x, op, t, size, ln, info))
        x, op = x + size, op + ln
    assert op == n and x == len(stream)
    return n, out


def dependent_blocks(stream: bytes, block: int = BLOCK):
    """ranges_model.dependent_blocks for bytes: a block is dependent iff it resumes a
    copy or holds a copy whose source begins before the block."""
    dep = set()
    for _, pos, t, _, ln, off in walk(stream)[1]:
        if t == 0:
            continue
        for b in range(pos // block, (pos + ln - 1) // block + 1):
            if pos < b * block or pos - off < b * block:
                dep.add(b)
    return dep


def element_end(stream: bytes, x: int) -> int:
    return x + k4.parse_element(stream.__getitem__, x)[1]


def tail_kind(stream: bytes, entry: int):
    """("L", length bytes) / ("C", copy kind) of the element that entry's block resumes"""
    t, _, _, info = k4.parse_element(stream.__getitem__, entry & MASK)
    return ("L", info - 1) if t == 0 else ("C", k4.KIND[t])


# ---------------------------------------------------------------------------
# 1b: the SINGLE stream of independent blocks
# ---------------------------------------------------------------------------
def boundary(var: str, rng):
    """-> (bytes of the elements that lie before the block boundary, the elements)"""
    if var == "a":
        return 0, []
    if var == "b":
        k = int(rng.integers(1, 60))
        return k, [("L", int(rng.integers(k + 1, 61)), 0)]
    if var[0] == "c":
        w = int(var[1])
        ln = {1: 200, 2: 600, 3: 5000, 4: 3000}[w]
        return int(rng.integers(1, ln)), [("L", ln, w)]
    if var == "d":
        return int(rng.integers(30000, 50001)), [("L", 140000, 3 + int(rng.integers(0, 2)))]
    if var[0] == "e":  # its source inside the block where it starts
        kind = int(var[1])
        ln = int(rng.integers(5, 12)) if kind == 1 else int(rng.integers(2, 65))
        off = int(rng.integers(1, 2048 if kind == 1 else 60000)) if rng.integers(2) else int(rng.integers(1, ln + 3))
        return int(rng.integers(1, ln)), [("C", ln, off, kind)]
    if var == "f":
        r = int(rng.integers(1, 300)) if rng.integers(2) else 0
        off = r + int(rng.integers(1, 60000))
        return 0, k4.filler(rng, r) + [("C", int(rng.integers(4, 65)), off, 2 if off < 65536 and rng.integers(2) else 4)]
    assert var == "g"
    off = int(rng.integers(1, 64))
    return 0, [("C", int(rng.integers(off + 1, 65)), off, 2)]


@functools.lru_cache(maxsize=None)
def single_independent_input():
    """-> stream (uint8), index (int64), n, {block: the kind a..g of the boundary at
    its start}, k4_model's statistics over the blocks it decodes."""
    rng = np.random.default_rng(860)
    cases = [c for f in k4.FAMILIES for c in k4.cases_of(f)]
    order = [int(i) for i in np.random.default_rng(861).permutation(len(cases))]
    ops, out, kinds, ev, q = [], 0, {}, 0, 0
    while q < len(order):
        nb = (out // BLOCK + 1) * BLOCK
        var = CYCLE[ev % len(CYCLE)]
        ev += 1
        before, els = boundary(var, rng)
        while q < len(order) and out + k4.out_len(cases[order[q]]) + before + 200 <= nb:
            ops += cases[order[q]]
            out += k4.out_len(cases[order[q]])
            q += 1
        ops += k4.filler(rng, nb - out - before) + els
        out = nb - before + k4.out_len(els)
        kinds[nb // BLOCK] = var[0]
        if var == "d":
            kinds[nb // BLOCK + 1] = "d"
    ops += k4.filler(rng, 300)
    n = out + 300
    tape = k4.Tape(960, n + 4096)
    head = k4.varint(n)
    body, edges = k4.encode(ops, tape, len(head))
    buf = bytearray(head + body)
    n2, entries = k4.host_index(bytes(buf))
    units = (n + BLOCK - 1) // BLOCK
    assert n2 == n and len(entries) == units + 1
    for rounds in range(2):
        S, trace = k4.Stats(), []
        for u in range(units):
            k4.k4_model(buf, entries[u] & MASK, entries[u + 1] & MASK, entries[-1], min(BLOCK, n - u * BLOCK),
                        u * BLOCK, n if u == 0 else None, entries[u] >> 40, entries[u + 1] >> 40, False, 0, S,
                        trace if rounds == 0 else None)
        if rounds == 0:  # (a block deferred before its edge copies keeps their offset of 1)
            assert k4.patch_edges(buf, edges, trace) >= len(edges) // 2
    assert k4.host_index(bytes(buf))[1] == entries
    stream = np.frombuffer(bytes(buf), dtype=np.uint8)
    return stream, np.array(entries, dtype=np.int64), n, kinds, S


@functools.lru_cache(maxsize=None)
def single_independent_want() -> np.ndarray:
    return np.frombuffer(oracle.decompress(single_independent_input()[0].tobytes()), dtype=np.uint8)


@functools.lru_cache(maxsize=None)
def single_independent_dependent():
    return frozenset(dependent_blocks(single_independent_input()[0].tobytes()))


def model_statuses():
    """k4_model(BACK=False) of every block of the SINGLE stream: "ok" / "defer" """
    stream, index, n, _, _ = single_independent_input()
    e, buf = [int(x) for x in index], stream.tobytes()
    return [k4.k4_model(buf, e[u] & MASK, e[u + 1] & MASK, e[-1], min(BLOCK, n - u * BLOCK), u * BLOCK,
                        n if u == 0 else None, e[u] >> 40, e[u + 1] >> 40, False, 0, k4.Stats())
            for u in range(len(e) - 1)]


def block_span(stream: bytes, entries, u: int):
    """The compressed bytes block u needs resident: from its entry to the next one,
    or to the end of the element that straddles out of it."""
    x1 = entries[u + 1] & MASK
    return entries[u] & MASK, element_end(stream, x1) if entries[u + 1] >> 40 else x1


# ---------------------------------------------------------------------------
# the GPU call: the whole sentinel-filled buffer is compared
# ---------------------------------------------------------------------------
def up(a):
    import torch
    a = np.array(a)
    return torch.from_numpy(a).cuda() if a.size else torch.empty(0, dtype=torch.uint8, device="cuda")


class Packer:
    """Output offsets: each range at the residue mod 16 asked for, sentinel bytes between"""

    def __init__(self, gap: int = 3):
        self.gap, self.oo, self.ranges = gap, 0, []

    def add(self, start: int, length: int, res: int):
        oo = self.oo + self.gap
        oo += (res - oo) % 16
        self.ranges.append((int(start), int(length), oo))
        self.oo = oo + length

    @property
    def total(self):
        return self.oo + self.gap


def decode_ranges(codec, comp, offs, n, chunk, layout, ranges, out_bytes, data, model, origin=0, early=EARLY):
    """One call into a buffer of sentinels with GUARD more of them on both sides (the
    output proper is 16-aligned, so out_offset mod 16 is the address residue).  The
    statuses must be `model`; a range whose model status is 0 holds data[start, start
    + length); every other byte is the sentinel, but for the own output range of a
    range that fails while it decodes: a status not in `early` (K4 itself reports
    ERR_TRUNCATED for an element cut short, after it has stored the unit's bytes up
    to it: the hostile tests pass early = ()).  -> the statuses."""
    import torch
    buf = torch.full((out_bytes + 2 * GUARD,), SENT, dtype=torch.uint8, device="cuda")
    out = buf[GUARD:GUARD + out_bytes]
    assert out.data_ptr() % 16 == 0
    _, st = codec.decompress_ranges_tensor(comp, offs, n, ranges, out=out, chunk=chunk, layout=layout,
                                           comp_origin=origin)
    st = [int(x) for x in st.cpu().numpy()]
    got = buf.cpu().numpy()
    assert len(model) == len(ranges)
    wrong = [(i, ranges[i], st[i], model[i]) for i in range(len(ranges)) if st[i] != model[i]]
    assert not wrong, f"{len(wrong)} statuses differ (index, range, got, model): {wrong[:6]}"
    exp = np.full(got.size, SENT, dtype=np.uint8)
    for (a, ln, oo), m in zip(ranges, model):
        if m == OK:
            exp[GUARD + oo:GUARD + oo + ln] = data[a:a + ln]
        elif m not in early:
            exp[GUARD + oo:GUARD + oo + ln] = got[GUARD + oo:GUARD + oo + ln]
    bad = np.flatnonzero(got != exp)
    if bad.size:
        at = int(bad[0]) - GUARD
        inside = [(i, r) for i, r in enumerate(ranges) if r[2] <= at < r[2] + r[1]][:1]
        raise AssertionError(f"{bad.size} bytes differ, the first at output byte {at}: "
                             + (f"byte {at - inside[0][1][2]} of range {inside[0]}" if inside else "outside every range"))
    first = next((m for m in model if m != OK), OK)
    assert codec.last_ranges_status == first, (codec.last_ranges_status, first)
    return st


def census():
    """The counts of 1d over the SINGLE stream -> dict"""
    stream, index, n, kinds, S = single_independent_input()
    buf, e = stream.tobytes(), [int(x) for x in index]
    dep = single_independent_dependent()
    units = len(e) - 1
    out_of = collections.Counter()
    inside = []
    for u in range(units):
        if u in dep:
            continue
        if u + 1 < units and e[u + 1] >> 40:
            out_of[tail_kind(buf, e[u + 1])] += 1
        if e[u] >> 40 and e[u + 1] >> 40 and e[u] & MASK == e[u + 1] & MASK and buf[e[u] & MASK] & 3 == 0:
            inside.append(u)
    return {"n": n, "bytes": len(buf), "units": units, "dependent": sorted(dep),
            "kinds": collections.Counter(kinds.values()), "straddles_out": out_of, "inside_literal": inside,
            "independent_after_0": sum(1 for u in range(1, units) if u not in dep)}

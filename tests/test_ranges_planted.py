"""Range decode (snappy_amd_decompress_ranges_device) on planted
streams: kr4_decode_range_units -- k4_body<false, false, false, true>, a code
object of its own -- on the edges test_k4_decode plants for K4, kr0_range_check at
a straddling tail element, kr6_clip's three paths and the range key.

The element streams are test_k4_decode's, imported: its STREAMS inputs unchanged
(one case per unit, chunk 8192 and 8191), and its cases once more as one SINGLE
stream of *independent* blocks (ranges_planted.single_independent_input), since a
range has no second pass.  Its block boundaries cycle through
  (a) an exact element boundary,
  (b) a literal of <= 60 bytes straddling, 1..59 bytes before the boundary,
  (c) straddling literals with 1, 2, 3 and 4 length bytes (200, 600, 5,000 and
      3,000 bytes),
  (d) a literal of 140,000 bytes that begins in block b, covers b + 1 and ends in
      b + 2,
  (e) a straddling copy-1 / copy-2 / copy-4 whose source lies in the block where
      it starts (that block is not dependent, the next one is),
  (f) a plain copy reaching back over the boundary,
  (g) an overlapping copy (off < len) as the block's first element,
so that every straddling element starts in a block that is not dependent.  Which
blocks are dependent is decided on the bytes (ranges_planted.dependent_blocks:
ranges_model's rule restated for an element walk, pinned to it on
ranges_cases.FOREIGN), and k4_model(BACK = False) must return "defer" for exactly
those.

Every GPU decode goes into a buffer of sentinels and the whole buffer is compared
(ranges_planted.decode_ranges): the oracle's bytes in every range the model calls
OK, the sentinel everywhere else, but for the own output of a range that fails
while it decodes.  The bytes are oracle.decompress / oracle.decompress_streams'.

The window tests need a second range that decodes in every row, so each window
reaches, on the side away from its cut, far enough to hold that range's block:
the windows cut at their end start at an earlier independent block (one whose own
tail element ends before the cut), the window that starts one byte late ends
after a later one.  The range inside the block under test is the whole block
(interior, straight to the output) at odd address residues and an edge range at
even ones: a unit that kr0_range_check let through by mistake and K4 then refused
would leave an edge range's output untouched, but not an interior one's.

Measured (test_planted_inputs_have_their_properties prints them):
* the SINGLE stream: 6,424,717 bytes decoded, 4,958,864 compressed, 99 blocks, 30
  of them dependent and 68 independent after block 0; blocks per boundary kind a / b
  / c / d / e / f / g: 24 / 11 / 23 / 10 / 18 / 6 / 6; elements straddling out of an
  independent block: literals with 0 / 1 / 2 / 3 / 4 length bytes 11 / 6 / 6 / 8 /
  13, copy-1 / copy-2 / copy-4 6 / 6 / 6; 5 blocks wholly inside a literal; over the
  independent blocks k4_model counts 5,056 copies further back than the ring, 1,939
  literals through k4_literal_hbm, 78 tail elements and 44 resumed literals.
* the STREAMS units (chunk 8192): 7,594 copies further back than 4,096 bytes.
* on the MI355X every GPU test of this module takes under 1 s (the longest are
  test_single_independent_blocks, 0.8 s, and the first use of each STREAMS input,
  0.2-0.6 s, most of it the input's build on the host); the module 6 s.

A deliberate break and the tests that fail (the first, second and fourth tried on
the MI355X in a scratch build, the third by reading: it would leave the slots):
* kr0_range_check, `size > left` -> `size > left + 1`: the window one byte short is
  accepted, K4 stores the block's bytes before it meets the cut element:
  test_windows_cut_at_the_tail_element, every header width and copy kind (not
  "inside": a resumed literal that does not fit is refused before any store).
* kr6_clip, `8 * sa` -> `8 * (sa ^ 1)`: test_clip_sweep and every
  test_streams_planted_staged.
* `(edge - 1) % slot_cap` -> `edge % slot_cap` in one of its two places: the clip
  reads another unit's slot: test_streams_planted_staged, test_clip_sweep.
* atomicMin -> atomicMax on the range key (k4_body): the key stays ~0 and the
  range reports 0: test_single_independent_blocks, test_hostile_units,
  test_lowest_failing_unit_wins (in
  kr0_range_check: test_windows_cut_at_the_tail_element)."""
import collections

import numpy as np
import pytest

import datagen
import oracle
import ranges_cases as rc
import ranges_model as rm
import ranges_planted as rp
import snappy_amd
import test_k4_decode as k4
from golden_inputs import build_stream
from ranges_planted import BLOCK, MASK, OK, Packer, decode_ranges, up

DEP, TRUNC = snappy_amd.ERR_DEPENDENT, snappy_amd.ERR_TRUNCATED


# ---------------------------------------------------------------------------
# 1: the inputs and their proof (no GPU)
# ---------------------------------------------------------------------------
def test_dependency_model_on_bytes_is_ranges_model():
    assert (rp.OK, rp.ERR_ARG, rp.ERR_TRUNCATED, rp.ERR_CAPACITY, rp.ERR_DEPENDENT) == (
        0, snappy_amd.ERR_ARG, snappy_amd.ERR_TRUNCATED, snappy_amd.ERR_CAPACITY, snappy_amd.ERR_DEPENDENT)
    for name, ops in rc.FOREIGN.items():
        dep = rp.dependent_blocks(build_stream(ops))
        assert dep == rm.dependent_blocks(ops) == set(rc.FOREIGN_DEPENDENT[name]), name


def test_planted_inputs_have_their_properties():
    """No GPU: the oracle and k4_model run the SINGLE stream of independent blocks,
    the model defers exactly the dependent blocks, and every boundary kind, header
    width and copy kind the GPU tests rely on is there."""
    stream, index, n, kinds, S = rp.single_independent_input()
    c = rp.census()
    dep = set(c["dependent"])
    print(f"SINGLE independent: {n} bytes decoded, {c['bytes']} compressed, {c['units']} blocks, {len(dep)} dependent, "
          f"{c['independent_after_0']} independent after block 0")
    print("  blocks per boundary kind:", dict(sorted(c["kinds"].items())))
    print("  elements straddling out of an independent block:", dict(sorted(c["straddles_out"].items())))
    print("  blocks wholly inside a literal:", c["inside_literal"])
    print(f"  k4_model over the independent blocks: far copies {S.n['copy_far']}, HBM literals {S.n['hbm_literal']}, "
          f"tail elements {S.n['tail_element']}, resumed literals {S.n['resume_literal']}")
    assert rp.single_independent_want().size == n
    st = rp.model_statuses()
    assert [u for u, s in enumerate(st) if s == "defer"] == sorted(dep)
    assert all(s in ("ok", "defer") for s in st)
    assert dep == {u for u, kind in kinds.items() if kind in "efg"}
    assert all(c["kinds"][kind] >= 3 for kind in rp.KINDS), c["kinds"]
    assert all(c["straddles_out"][key] >= 1 for key in [("L", w) for w in range(5)] + [("C", k) for k in (1, 2, 4)])
    assert len(c["inside_literal"]) >= 1
    assert c["independent_after_0"] >= 40 and len(dep) >= 9
    assert c["bytes"] <= 16 << 20 and n <= 16 << 20
    far = sum(k4.streams_input(f, 8192)[3].n["copy_far"] for f in k4.FAMILIES)
    print(f"STREAMS units, chunk 8192: copies further back than 4,096 bytes: {far}")
    assert far >= 1000


# ---------------------------------------------------------------------------
# 2: STREAMS planted, every unit interior
# ---------------------------------------------------------------------------
def streams_on_gpu(family, chunk):
    payload, offs, units, _ = k4.streams_input(family, chunk)
    return up(payload), up(offs), units, k4.streams_want(family, chunk)


@pytest.mark.gpu
@pytest.mark.parametrize("chunk", k4.CHUNKS)
@pytest.mark.parametrize("family", k4.FAMILIES)
def test_streams_planted_interior(codec, family, chunk):
    """Runs of 1..3 whole units straight to out + land, the i-th range of a call at
    output residue (i + k) mod 16, k = 0 and 5."""
    comp, offs, units, want = streams_on_gpu(family, chunk)
    for k in (0, 5):
        p, u, i = Packer(), 0, 0
        while u < units:
            run = 1 if family == "span" else min(1 + i % 3, units - u)
            p.add(u * chunk, run * chunk, (i + k) % 16)
            u, i = u + run, i + 1
        assert {r[2] % 16 for r in p.ranges} == set(range(16))
        decode_ranges(codec, comp, offs, units * chunk, chunk, snappy_amd.STREAMS, p.ranges, p.total, want,
                      [OK] * len(p.ranges))


# ---------------------------------------------------------------------------
# 3: STREAMS planted, every unit staged, the slots reused
# ---------------------------------------------------------------------------
STAGED = [(f, c, 5) for f in k4.FAMILIES for c in k4.CHUNKS] + [(f, c, 0) for f in ("ring", "long") for c in k4.CHUNKS]


@pytest.mark.gpu
@pytest.mark.parametrize("family,chunk,slots", STAGED)
def test_streams_planted_staged(codec, monkeypatch, family, chunk, slots):
    """Every unit as an edge unit -- [1, size), [0, size - 1) or a random [lo, hi) --
    and ranges from inside unit u to inside u + 2; with 5 slots each is reused by
    hundreds of other units, so a far copy or a long literal that read the slot's
    stale bytes shows."""
    if slots:
        monkeypatch.setenv("SNAPPY_AMD_RANGE_SLOTS", str(slots))
    else:
        monkeypatch.delenv("SNAPPY_AMD_RANGE_SLOTS", raising=False)
    comp, offs, units, want = streams_on_gpu(family, chunk)
    rng = np.random.default_rng(870 + chunk)
    p = Packer()
    for u in range(units):
        if u % 3 == 0:
            lo, hi = 1, chunk
        elif u % 3 == 1:
            lo, hi = 0, chunk - 1
        else:
            lo = int(rng.integers(1, chunk - 1))
            hi = int(rng.integers(lo + 1, chunk + 1))
        p.add(u * chunk + lo, hi - lo, (7 * u + 3) % 16)
    for u in range(0, units - 2, 5):
        lo, hi = int(rng.integers(1, chunk)), int(rng.integers(1, chunk))
        p.add(u * chunk + lo, 2 * chunk - lo + hi, (u + 11) % 16)
    decode_ranges(codec, comp, offs, units * chunk, chunk, snappy_amd.STREAMS, p.ranges, p.total, want,
                  [OK] * len(p.ranges))


# ---------------------------------------------------------------------------
# 4: the SINGLE stream of independent blocks
# ---------------------------------------------------------------------------
@pytest.mark.gpu
def test_single_independent_blocks(codec):
    """One call: every independent block whole (interior) and as [b0 + 1, b0 + size
    - 1), a range inside every dependent block, ranges over two and three
    consecutive independent blocks (edge, interior, edge) and over an independent
    and a dependent block."""
    stream, index, n, _, _ = rp.single_independent_input()
    want, dep = rp.single_independent_want(), rp.single_independent_dependent()
    comp = up(stream)
    n_dev, offs = codec.index_tensor(comp)
    assert n_dev == n and np.array_equal(offs.cpu().numpy(), index)
    offs = offs.contiguous()
    units = index.size - 1

    def size(u):
        return min(BLOCK, n - u * BLOCK)

    p, model = Packer(), []
    for u in range(units):
        b0 = u * BLOCK
        if u in dep:
            p.add(b0 + 10 + 97 * u % 5000, 1000, u % 16)
            model.append(DEP)
        else:
            p.add(b0, size(u), u % 16)
            p.add(b0 + 1, size(u) - 2, (u + 7) % 16)
            model += [OK, OK]
    # a resumed literal (skip0 > 0: k4_literal_hbm to dst) as an interior unit at every
    # residue: one block per header width, and one wholly inside a literal
    buf, e = stream.tobytes(), [int(x) for x in index]
    resumed = {}
    for u in range(1, units - 1):
        if u not in dep and e[u] >> 40:
            inside = e[u] & MASK == e[u + 1] & MASK
            resumed.setdefault("inside" if inside else rp.tail_kind(buf, e[u]), u)
    assert set(resumed) == {"inside"} | {("L", w) for w in range(5)}, resumed
    for u in resumed.values():
        for res in range(16):
            p.add(u * BLOCK, BLOCK, res)
            model.append(OK)
    spans = collections.Counter()
    for u in range(units - 1):
        for k in (2, 3):
            if u + k > units:
                continue
            deps = [b in dep for b in range(u, u + k)]
            if any(deps) and (k == 3 or all(deps)):
                continue
            a = u * BLOCK + 1 + 37 * u % 60000
            b = (u + k - 1) * BLOCK + 1 + 53 * u % (size(u + k - 1) - 1)
            p.add(a, b - a, (3 * u + k) % 16)
            model.append(DEP if any(deps) else OK)
            spans[(k, tuple(deps))] += 1
    print("spans (blocks, dependent):", dict(spans))
    assert spans[(2, (False, False))] >= 10 and spans[(3, (False, False, False))] >= 5
    assert spans[(2, (False, True))] >= 5 and spans[(2, (True, False))] >= 5
    decode_ranges(codec, comp, offs, n, BLOCK, snappy_amd.SINGLE, p.ranges, p.total, want, model)


# ---------------------------------------------------------------------------
# 5: windows cut at a straddling tail element
# ---------------------------------------------------------------------------
def window_blocks():
    """{what straddles out: block u}: one independent block per literal header width
    and copy kind, and a block wholly inside the 140,000-byte literal."""
    stream, index, n, _, _ = rp.single_independent_input()
    buf, e = stream.tobytes(), [int(x) for x in index]
    dep, c = rp.single_independent_dependent(), rp.census()
    pick = {}
    for u in range(3, len(e) - 4):
        if u not in dep and e[u + 1] >> 40 and u not in c["inside_literal"]:
            pick.setdefault(rp.tail_kind(buf, e[u + 1]), u)
    pick["inside"] = next(u for u in c["inside_literal"] if u >= 3)
    return pick


@pytest.mark.gpu
@pytest.mark.parametrize("what", [("L", 0), ("L", 1), ("L", 2), ("L", 3), ("L", 4), ("C", 1), ("C", 2), ("C", 4), "inside"],
                         ids=lambda w: w if isinstance(w, str) else f"{w[0]}{w[1]}")
def test_windows_cut_at_the_tail_element(codec, what):
    """kr0_range_check's tail-element branch: the window must hold the straddling
    element whole -- exactly fitting is accepted; one byte short, cut inside its
    length bytes, cut at its first byte (o1 == w1), and a window that starts one
    byte late are ERR_TRUNCATED before any store.  At every address residue mod 4;
    a second range in a block that is wholly resident decodes in every row."""
    import torch
    stream, index, n, _, _ = rp.single_independent_input()
    want, dep = rp.single_independent_want(), rp.single_independent_dependent()
    buf, e = stream.tobytes(), [int(x) for x in index]
    offs = up(index)
    u = window_blocks()[what]
    w0, end = rp.block_span(buf, e, u)
    o1 = e[u + 1] & MASK
    kind = rp.tail_kind(buf, e[u + 1])
    assert what == "inside" or kind == what
    assert end == rp.element_end(buf, o1) and w0 <= o1 < end
    # the second range's block: before u and resident even when the window ends at o1;
    # after u and resident even when the window starts at w0 + 1
    before = next(v for v in range(u - 1, 0, -1) if v not in dep and rp.block_span(buf, e, v)[1] <= o1)
    after = next(v for v in range(u + 1, len(e) - 1) if v not in dep and e[v] & MASK > w0)
    a0, a1 = e[before] & MASK, rp.block_span(buf, e, after)[1]
    width = kind[1] if kind[0] == "L" else 0
    cuts = {end - 1, o1}                       # one byte short; at the tail element's first byte
    cuts |= {o1 + 1 + j for j in range(width)}  # after the tag, inside the length bytes
    if width:
        cuts.add(o1 + 1 + width)               # the header whole, the literal's bytes missing
    rows = [(a0, end, before, OK)] + [(a0, w1, before, TRUNC) for w1 in sorted(cuts)] + [(w0 + 1, a1, after, TRUNC)]
    assert all(a0 < w1 < end for w1 in cuts)
    b0, size = u * BLOCK, min(BLOCK, n - u * BLOCK)
    for res in range(4):
        mine = (b0 + 100, size - 107, 5 + res) if res % 2 == 0 else (b0, size, 5 + res)
        for wa, wb, v, expect in rows:
            raw = torch.full((wb - wa + 64,), 0xFF, dtype=torch.uint8, device="cuda")
            raw[res:res + wb - wa] = up(stream[wa:wb])
            win = raw[res:res + wb - wa]
            assert win.data_ptr() % 4 == res
            other = (v * BLOCK + 5, 1000, 5 + res + BLOCK + 40)
            decode_ranges(codec, win, offs, n, BLOCK, snappy_amd.SINGLE, [mine, other], other[2] + 1000 + 9, want,
                          [expect, OK], origin=wa)


# ---------------------------------------------------------------------------
# 6: the clip, every (source, destination) residue
# ---------------------------------------------------------------------------
@pytest.mark.gpu
def test_clip_sweep(codec):
    """kr6_clip's 16-byte, plain-dword and funnel-shift paths: every (lo mod 16, dst
    mod 16) pair at lengths 1..48 (h0 > len, body == 0), around the 256 x 16-byte
    stride and two longer ones; hi at the slot's last byte (the funnel reads the
    dword after it), at the last byte of the 1,000-byte tail block, and one-byte
    ranges at the blocks' ends.  Random bytes: a misplaced one shows."""
    n = 2 * BLOCK + 1000
    data = datagen.make("R", n, 880)
    comp, offs = codec.compress_tensor(up(data))
    comp, offs = comp.contiguous(), offs.contiguous()
    want = np.frombuffer(oracle.decompress(comp.cpu().numpy().tobytes()), dtype=np.uint8)
    assert np.array_equal(want, data)
    lengths = list(range(1, 49)) + list(range(4079, 4114)) + [8191, 8208]
    p, i = Packer(gap=1), 0
    for ln in lengths:
        for sr in range(16):
            for dr in range(16):
                lo = BLOCK + 16 * (1 + (131 * i) % 3000) + sr  # (16 * 3001 + 15 + 8208 < 65536)
                p.add(lo, ln, dr)
                i += 1
    swept = len(p.ranges)
    for dr in range(16):
        for back in range(17, 81):             # hi = the block's last byte, every lo mod 16
            p.add(2 * BLOCK - back, back, dr)
        for back in (1, 5, 17, 100, 999, 1000):
            p.add(n - back, back, dr)
        for b0, size in ((0, BLOCK), (BLOCK, BLOCK), (2 * BLOCK, 1000)):
            p.add(b0, 1, dr)
            p.add(b0 + size - 1, 1, dr)
    print(f"clip sweep: {swept} swept ranges, {len(p.ranges)} in all, {p.total} output bytes")
    assert swept == 256 * 85
    decode_ranges(codec, comp, offs, n, BLOCK, snappy_amd.SINGLE, p.ranges, p.total, want, [OK] * len(p.ranges))


# ---------------------------------------------------------------------------
# 7: hostile units and the lowest failing unit
# ---------------------------------------------------------------------------
C = k4.HCHUNK


def hostile_payload():
    """Five units per case -- good, good, the case's unit, good, good -- as
    test_hostile_streams builds them, all cases in one payload."""
    tape = k4.Tape(992, 1 << 20)
    rng = np.random.default_rng(993)
    good = [k4.varint(C) + k4.encode(k4.filler(rng, C), tape)[0] for _ in range(4)]
    bodies = {**k4.hostile_bodies(), **k4.streams_only_bodies()}
    cases = {name: (k4.varint(C) + body, code) for name, (body, code, _, _) in bodies.items()}
    body = bodies["control"][0]
    cases["preamble chunk + 1"] = (k4.varint(C + 1) + body, snappy_amd.ERR_HEADER)
    cases["preamble chunk - 1"] = (k4.varint(C - 1) + body, snappy_amd.ERR_HEADER)
    return good, cases


def offsets_of(units):
    offs = [0]
    for u in units:
        offs.append(offs[-1] + len(u))
    return offs


@pytest.mark.gpu
def test_hostile_units(codec):
    """The units K4 is documented to refuse before any out-of-range access, through
    the RANGE instantiation: one range per unit, interior and edge alternating (both
    ways round), accepted exactly where the oracle accepts and refused with the
    code of the whole-stream decode; the same statuses from a window that ends at
    the hostile unit's last byte."""
    good, cases = hostile_payload()
    units, model, names, whole = [], [], [], {}
    for name, (unit, code) in cases.items():
        five = good[:2] + [unit] + good[2:]
        ok = k4.oracle_accepts(unit, C) is not None
        got, rcode = k4.gpu_decode(codec, b"".join(five), offsets_of(five), 5 * C, C, snappy_amd.STREAMS)
        print(f"{name}: oracle {'accepts' if ok else 'refuses'}, whole-stream rc {rcode}")
        assert (got is not None) == ok, name
        if code is not None:
            assert rcode == code and not ok, (name, rcode)
        if "offset e_op + 1" in name or "offset 0 first" in name:
            assert rcode == snappy_amd.ERR_OFFSET, (name, rcode)  # a copy reaching before its unit
        units += five
        model += [OK, OK, rcode, OK, OK]
        names.append(name)
        whole[name] = rcode
    assert sum(1 for r in whole.values() if r == OK) >= 4 and sum(1 for r in whole.values() if r != OK) >= 30
    payload = b"".join(units)
    offs_h = offsets_of(units)
    want = np.frombuffer(b"".join(k4.oracle_accepts(u, C) or bytes(C) for u in units), dtype=np.uint8)
    comp, offs, n = up(np.frombuffer(payload, dtype=np.uint8)), up(np.array(offs_h, dtype=np.int64)), len(units) * C

    def ranges_of(us, parity):
        p = Packer()
        for u in us:
            if (u + parity) % 2:
                p.add(u * C, C, (u + 3) % 16)
            else:
                p.add(u * C + 1, C - 2, (u + 3) % 16)
        return p

    for parity in (0, 1):
        p = ranges_of(range(len(units)), parity)
        decode_ranges(codec, comp, offs, n, C, snappy_amd.STREAMS, p.ranges, p.total, want, model, early=())
    # no read depends on bytes past the window: it ends at the hostile unit's last byte
    for c, name in enumerate(names):
        h = 5 * c + 2
        p = ranges_of(range(5 * c, h + 1), c % 2)
        decode_ranges(codec, comp[:offs_h[h + 1]], offs, n, C, snappy_amd.STREAMS, p.ranges, p.total, want,
                      model[5 * c:h + 1], early=())


@pytest.mark.gpu
def test_lowest_failing_unit_wins(codec):
    """Two ranges over two hostile units with different codes and a good unit between
    them, in either order: each reports its lower unit's code."""
    good, cases = hostile_payload()
    off0, hdr = cases["copy-2 offset 0"][0], cases["preamble chunk + 1"][0]
    assert cases["copy-2 offset 0"][1] == snappy_amd.ERR_OFFSET and cases["preamble chunk + 1"][1] == snappy_amd.ERR_HEADER
    units = [good[0], off0, good[1], hdr, good[2], off0, good[3]]
    want = np.frombuffer(b"".join(k4.oracle_accepts(u, C) or bytes(C) for u in units), dtype=np.uint8)
    comp = up(np.frombuffer(b"".join(units), dtype=np.uint8))
    offs, n = up(np.array(offsets_of(units), dtype=np.int64)), len(units) * C
    p = Packer()
    p.add(1 * C + 1, 3 * C - 2, 3)   # units 1 (ERR_OFFSET), 2, 3 (ERR_HEADER): edge, interior, edge
    p.add(3 * C + 1, 3 * C - 2, 9)   # units 3 (ERR_HEADER), 4, 5 (ERR_OFFSET)
    p.add(1 * C, 3 * C, 14)          # the same, every unit interior
    p.add(3 * C, 3 * C, 6)
    p.add(0, C, 1)                   # and the good units around them decode
    p.add(6 * C + 1, C - 1, 2)
    model = [snappy_amd.ERR_OFFSET, snappy_amd.ERR_HEADER, snappy_amd.ERR_OFFSET, snappy_amd.ERR_HEADER, OK, OK]
    decode_ranges(codec, comp, offs, n, C, snappy_amd.STREAMS, p.ranges, p.total, want, model, early=())

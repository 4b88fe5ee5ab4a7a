"""k1r_body's and K2's record forms on the planted inputs of the modules that own
them: kr1_match_records / kr1_match_records64 / kr2_emit_records through
compress_records_device (E) and kr1_match_lunits / kr1_match_lunits64 /
kr2_emit_lunits through compress_long_records_device (F).  The units are cut
exactly as test_k1r_flush_inloop.py, test_k1r64_ring.py and test_k2_emit.py cut
them, so their CPU proofs of what a unit reaches (flushes with 49-64 tokens
pending, escapes, tag collisions, far / wrap / edge ring candidates, K2's direct
passes) hold for the records; only where the bytes lie and where the tokens,
escapes and segment pairs go is new.  Layouts are record_layouts.py's.

E. One call per owning module (test_records_planted[flush | ring | k2]); a batch
   mixes all of the module's unit sizes, every record at its own source alignment.
   A matched record of L bytes owns records_need_words(L) words of scratch at the
   scanned offset of its place in the batch, the next record's words directly
   behind; the two classes (K1r: up to 32,768 bytes, K1r64: above) are matched by
   separate launches.  The largest units of the token-dense inputs (alpha2f,
   escapes, far_alpha, planted_dense; 16,384 bytes or more) are each followed in the
   batch by a record of the other class, borrowed where the module has none of it
   (33,025-byte units of small_input for K1r64, 4,096-byte units of alpha2f for
   K1r): an overrun of token, escape or segment words is then a wrong neighbour,
   not a word the same launch rewrites.
F. One call: every ring input as a record of four full blocks and as one of 3 *
   65,536 + 61,001 bytes at source alignments 0..3 (every block after the first
   is then unaligned), a record of planted_dense's first block followed by 4,097
   bytes of sparse20f (its last block takes the K1r list), records of 1, 100 and
   32,768 bytes between them.  Block tables against test_long_records.walk_table;
   every record decoded back into scattered ranges, with the table and without.

The bar: out[offs[i]:offs[i + 1]] == oracle.compress(record i), the offsets their
prefix sums, the sentinel intact past the total, every status 0.

test_layouts_have_their_properties (no GPU) prints:
* E flush: 1,827 records (1,815 of K1r, 12 borrowed of K1r64), 8 dense, each followed
  by a K1r64 record; ring: 112 records (80 of K1r64, 32 borrowed of K1r), 8 dense;
  k2: 106 records (90 of K1r, 4 + 12 borrowed of K1r64), 14 dense.  All four source
  alignments in both classes of each batch.
* F: 18 records, 9 of them long (alignments 0..3 at least twice), 43 blocks.
"""
import collections
import functools
import random

import numpy as np
import pytest

import record_layouts as rl
import snappy_amd
import test_k1r64_ring as ring
import test_k1r_flush_inloop as fl
import test_k2_emit as k2
from test_long_records import (compress_call as long_compress_call, decode_call as long_decode_call, expected_stream,
                               walk_table)
from test_records import compress_call

BLOCK = 65536
K1R_MAX = 32768  # SNAPPY_K1R_MAX_UNIT: K1r's largest record
DENSE_NAMES = ("alpha2f", "escapes", "far_alpha", "planted_dense")
DENSE_MIN = 16384
FAMILIES = ["flush", "ring", "k2"]
RING_SMALL = [32769, 33023, 33024, 33025]


def cut(a: np.ndarray, chunk: int):
    b = a.tobytes()
    return [b[i:i + chunk] for i in range(0, len(b), chunk)]


def cls(record: bytes) -> str:
    return "k1r" if len(record) <= K1R_MAX else "k1r64"


def borrowed(kind: str):
    """Records of the class a module has none (or too few) of, as followers of its dense records."""
    if kind == "k1r64":
        return [("small_input", r) for r in cut(ring.small_input(33025), 33025)]
    return [("alpha2f", r) for r in cut(fl.make("alpha2f", fl.TOTAL), 4096)]


def own_records(family: str):
    """[(input name, unit)] exactly as the owning module cuts them."""
    recs = []
    if family == "flush":
        for name in fl.INPUTS:
            for chunk in fl.CHUNKS:
                recs += [(name, r) for r in cut(fl.make(name, fl.TOTAL), chunk)]
    elif family == "ring":
        for name in ring.INPUTS:
            for L in (ring.BLOCK, ring.SHORT):
                recs += [(name, r) for r in cut(ring.data(name, ring.UNITS * L, L), L)]
        for chunk in RING_SMALL:
            recs += [("small_input", r) for r in cut(ring.small_input(chunk), chunk)]
    else:
        for name in k2.INPUTS:
            for chunk in k2.CHUNKS:
                recs += [(name, r) for r in cut(k2.make(name), chunk)]
    return recs


@functools.lru_cache(maxsize=None)
def e_batch(family: str):
    """-> records in batch order [(name, bytes, dense, borrowed)], blob, shift, descs."""
    own = own_records(family)
    have = collections.Counter(cls(r) for _, r in own)
    extra = []
    for kind in ("k1r", "k1r64"):
        if have[kind] < 16:
            extra += borrowed(kind)
    recs = [(n, r, n in DENSE_NAMES and len(r) >= DENSE_MIN, False) for n, r in own] + \
           [(n, r, False, True) for n, r in extra]
    rng = random.Random(2000 + FAMILIES.index(family))
    pool = {k: [i for i, x in enumerate(recs) if not x[2] and cls(x[1]) == k] for k in ("k1r", "k1r64")}
    for v in pool.values():
        rng.shuffle(v)
    seq = []
    for i, x in enumerate(recs):
        if x[2]:  # a dense record and, behind it, a record of the other class
            seq.append([i, pool["k1r64" if cls(x[1]) == "k1r" else "k1r"].pop()])
    seq += [[i] for v in pool.values() for i in v]
    rng.shuffle(seq)
    order = [i for s in seq for i in s]
    assert sorted(order) == list(range(len(recs)))
    recs = [recs[i] for i in order]
    shift = 1 + FAMILIES.index(family)
    blob, descs = rl.pack([[x[1]] for x in recs], [cls(x[1]) for x in recs], 2010 + FAMILIES.index(family), shift)
    return recs, blob, shift, descs


@pytest.mark.gpu
@pytest.mark.parametrize("family", FAMILIES)
def test_records_planted(codec, family):
    """E: kr1_match_records(64) and kr2_emit_records."""
    recs, blob, shift, descs = e_batch(family)
    rc, out, offs, status, out_len = compress_call(codec, rl.to_device(blob, shift), descs)
    assert rc == snappy_amd.OK and not status.any()
    want = [expected_stream(x[1]) for x in recs]
    sizes = [len(w) for w in want]
    assert offs.tolist() == [0] + np.cumsum(sizes).tolist(), "d_offsets is not the prefix sum of the oracle's sizes"
    assert out_len == sum(sizes)
    flat = out.tobytes()
    bad = [i for i, w in enumerate(want) if flat[offs[i]:offs[i + 1]] != w]
    assert not bad, [(i, recs[i][0], len(recs[i][1]), descs[i][0] % 4, i and recs[i - 1][0]) for i in bad[:6]]
    assert (out[out_len:] == rl.SENT).all(), "bytes written past the total"


# ---- F -----------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def f_batch():
    """-> records in batch order [(name, bytes, the oracle's stream or None: computed by
    expected_stream)], blob, shift, descs."""
    longs = []
    for name in ring.INPUTS:
        for n in (ring.UNITS * BLOCK, 3 * BLOCK + ring.SHORT):
            longs.append((name, ring.data(name, n, BLOCK).tobytes(), ("ring", name, n)))
    mixed = k2.make("planted_dense")[:BLOCK].tobytes() + fl.make("sparse20f", fl.TOTAL)[:4097].tobytes()
    longs.insert(5, ("planted_dense + sparse20f", mixed, None))
    esc = fl.make("escapes", fl.TOTAL).tobytes()
    recs = []
    for k, x in enumerate(longs):
        recs.append(x)
        n = (1, 100, 32768)[k % 3]
        recs.append((f"short {n}", esc[1000 * k:1000 * k + n], None))
    blob, descs = rl.pack([[x[1]] for x in recs], ["long" if len(x[1]) > BLOCK else "short" for x in recs], 2020, 3)
    return recs, blob, 3, descs


def f_want(x) -> bytes:
    if x[2] is not None:  # the owning module's cached stream
        return ring.want(x[2][1], "single", BLOCK, x[2][2], BLOCK)[0]
    return expected_stream(x[1])


@pytest.mark.gpu
def test_long_records_planted(codec):
    """F: kr1_match_lunits(64), kr2_emit_lunits, and the round trip."""
    recs, blob, shift, descs = f_batch()
    rc, out, offs, status, out_len, index = long_compress_call(codec, rl.to_device(blob, shift), descs)
    assert rc == snappy_amd.OK and not status.any()
    want = [f_want(x) for x in recs]
    sizes = [len(w) for w in want]
    assert offs.tolist() == [0] + np.cumsum(sizes).tolist(), "d_offsets is not the prefix sum of the oracle's sizes"
    assert out_len == sum(sizes)
    flat = out.tobytes()
    bad = [i for i, w in enumerate(want) if flat[offs[i]:offs[i + 1]] != w]
    assert not bad, [(i, recs[i][0], len(recs[i][1]), (shift + descs[i][0]) % 4) for i in bad[:6]]
    assert (out[out_len:] == rl.SENT).all(), "bytes written past the total"
    table = [e for w, x in zip(want, recs) for e in walk_table(w, len(x[1]))]
    assert index[:len(table)].tolist() == table, "block tables differ from the walk of the oracle's streams"
    assert (index[len(table):] == -7).all(), "entries written past the tables"
    # back into scattered ranges, from the oracle's streams at their own alignments
    lens = [len(x[1]) for x in recs]
    classes = ["long" if n > BLOCK else "short" for n in lens]
    comp_blob, c_descs = rl.pack([[w] for w in want], classes, 2021, 2)
    o_descs, size = rl.scatter(lens, classes, 2022)
    comp = rl.to_device(comp_blob, 2)
    img, care = rl.image(size, o_descs, [x[1] for x in recs])
    for idx in (table, None):
        buf = rl.sentinel_buffer(size)
        rc, status = long_decode_call(codec, comp, c_descs, buf, o_descs, index=idx)
        assert rc == snappy_amd.OK and not status.any()
        rl.assert_image(buf.cpu().numpy(), img, care, o_descs, ("round trip", idx is not None))


# ---- G: what the layouts claim (no GPU) ------------------------------------------------
def test_layouts_have_their_properties():
    for family in FAMILIES:
        recs, blob, shift, descs = e_batch(family)
        classes = [cls(x[1]) for x in recs]
        al = rl.source_alignments(descs, classes, shift)
        dense = [i for i, x in enumerate(recs) if x[2]]
        count = collections.Counter(classes)
        lent = collections.Counter((c, x[3]) for c, x in zip(classes, recs))
        print(f"E {family}: {len(recs)} records {dict(count)}, borrowed "
              f"{ {c: v for (c, b), v in lent.items() if b} }, base {shift} bytes into a dword, alignments "
              f"{ {k: sorted(v) for k, v in al.items()} }, dense {len(dense)}, sizes {len({len(x[1]) for x in recs})}")
        assert al == {"k1r": {0, 1, 2, 3}, "k1r64": {0, 1, 2, 3}}, (family, al)
        assert rl.shuffled_against_addresses(descs)
        assert len(dense) >= 8
        for i in dense:  # the scratch adjacency: the next record's words belong to the other class
            assert classes[i + 1] != classes[i] and not recs[i + 1][2], (family, i)
        for (o, ln), x in zip(descs, recs):
            assert blob[o:o + ln] == x[1]
        own = sorted((n, r) for n, r, _, b in recs if not b)
        assert own == sorted(own_records(family)), "every unit of the owning module, as it cuts them"
    names = {x[0] for x in e_batch("ring")[0] if x[2]} | {x[0] for x in e_batch("flush")[0] if x[2]} | \
            {x[0] for x in e_batch("k2")[0] if x[2]}
    assert names == set(DENSE_NAMES)
    recs, blob, shift, descs = f_batch()
    lens = [len(x[1]) for x in recs]
    classes = ["long" if n > BLOCK else "short" for n in lens]
    al = collections.Counter((shift + o) % 4 for (o, n), c in zip(descs, classes) if c == "long")
    blocks = sum((n + BLOCK - 1) // BLOCK for n in lens)
    print(f"F: {len(recs)} records, {classes.count('long')} long at alignments {dict(al)}, {blocks} blocks, "
          f"short lengths {sorted({n for n in lens if n <= BLOCK})}")
    assert set(al) == {0, 1, 2, 3} and min(al.values()) >= 2
    assert {n for n in lens if n <= BLOCK} == {1, 100, 32768}
    assert sorted(n for n in lens if n > BLOCK) == sorted([4 * BLOCK, 3 * BLOCK + ring.SHORT] * 4 + [BLOCK + 4097])
    assert all(classes[i] != classes[i + 1] for i in range(len(classes) - 1)), "a short record between the long ones"
    mixed = next(x[1] for x in recs if x[0].startswith("planted_dense"))
    assert len(mixed) - BLOCK <= K1R_MAX and mixed[BLOCK:] == fl.make("sparse20f", fl.TOTAL)[:4097].tobytes()
    o_descs, size = rl.scatter(lens, classes, 2022)
    res = rl.dest_residues(o_descs, classes)
    gaps = rl.gaps_of(o_descs, size)
    assert all(len(v) == min(16, classes.count(k)) for k, v in res.items()) and 1 <= min(gaps) and max(gaps) <= 40

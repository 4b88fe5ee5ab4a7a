"""What one context carries from one device call to the next: the catalogue's calls
(device_calls.py) in an order the rest of the suite never makes.

One context shares its scratch between entry points (tokens / sizes / ntok: unit,
record and long-record compress; f_scr: frame payloads and range staging slots;
r_meta: record and range plans; status: one word per decode unit, only the two
ticket words cleared) and keeps status_pending / last_status / last_layout /
last_units across other calls and trim().  The session's codec fixture meets the
test files in alphabetical order only.

CPU:  the catalogue (every expectation computed without a GPU, every decoy told
      apart from its inputs, the helpers against the oracle and the models) and the
      walk's coverage.
GPU:  test_baseline -- every case on a fresh context of its own equals expect();
      test_walk -- one context makes 485 calls: every ordered pair of
      families adjacent, every failing case followed by a successful case of each
      family it shares a buffer or a status path with, every large case before and
      after its small case, trim() at a seeded tenth of the positions; each call
      equals its baseline, and the scratch accounting after it;
      test_status_* -- the decode status words across other calls and trim().

Walk (test_walk_coverage prints it): 485 calls, 9 of large cases and 37 of failing
ones, 48 trims; all 400 ordered family pairs, 37 failing-then-successful pairs,
10 large/small transitions.
Module time on the MI355X: 87 tests in about 7 s; test_walk 0.9 s, each baseline
under 0.2 s; the slowest are CPU tests (the CRC model: frame_decode/large 1.6 s).

Mutants (scratch libraries through SNAPPY_AMD_LIB, none committed; the table with
all five is in test_stream_order.py).  Of this module's tests, mutant 4
(decompress_launch keeps last_status / status_pending) failed
test_empty_decode_clears_the_last_status, mutant 5 (trim frees the status words of
a pending status) failed both cases of test_status_survives_other_calls_and_trim;
every test here passed with mutants 1 and 2, which test_stream_order.py catches.
Mutant 3 ended in a GPU memory fault in test_stream_order.py and was dropped."""
import ctypes
import functools
import random

import numpy as np
import pytest

import device_calls as dc
import oracle
import snappy_amd
import frame_model as fm

SEED = 20
E = snappy_amd


# ---- the catalogue, on the CPU -----------------------------------------------------
def test_names_are_the_catalogue():
    assert dc.NAMES == [c.name for c in dc.catalogue()]
    assert dc.ASYNC_NAMES == [c.name for c in dc.catalogue() if c.async_form]
    assert sorted({c.family for c in dc.catalogue()}) == sorted(dc.FAMILIES) and len(dc.FAMILIES) == 20
    for c in dc.catalogue():
        if c.kind != "ok":
            assert dc.small_of(c.family).kind == "ok"
        assert (c.kind == "fail") == bool(c.shares) and set(c.shares) <= set(dc.FAMILIES)


@pytest.mark.parametrize("name", dc.NAMES)
def test_expectations_need_no_gpu(name):
    c = dc.by_name(name)
    ins, dec, exp, exp_d = c.inputs(), c.decoy(), c.expect(), c.expect_decoy()
    assert list(ins) == list(dec)
    for k in ins:
        assert ins[k].shape == dec[k].shape and ins[k].dtype == dec[k].dtype
    assert dc.differs(exp, exp_d), "the decoy's result cannot be told from the inputs'"
    for k, (n, dtype) in c.outputs().items():
        for e in (exp, exp_d):
            if k in e:
                assert e[k].shape == (n,) and e[k].dtype == dtype
    if c.kind == "large":
        assert sum(v.nbytes for v in ins.values()) + sum(n for n, _ in c.outputs().values()) >= 8 << 20
    else:
        assert max(v.nbytes for v in ins.values()) <= (256 << 10) + 16
    if c.kind == "fail":
        assert any(v != 0 for k, v in exp.items() if k in ("rc", "status") and np.isscalar(v))


def test_helpers_against_the_oracle_and_the_models():
    a = dc.T(2 * dc.B + 777, 5)
    stream, ent = dc.streams_as_single(a)
    assert stream == oracle.compress(a.tobytes())
    assert dc.single_index(stream) == (a.size, ent)
    rows = a[:2 * dc.B].reshape(2, dc.B)
    assert [int(x) for x in dc.crc32c_rows(rows)] == [fm.mask(fm.crc32c(r.tobytes())) for r in rows]
    payload, offs = oracle.compress_streams(a, dc.B)
    assert dc.frame_of(a) == fm.frame_streams(a.tobytes(), payload.tobytes(), offs)


# ---- the walk ----------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def walk():
    """-> (steps, counts): steps = [(case name, trim before it)].  A deterministic greedy
    walk: from the current case go to the case that meets the most requirements not met
    yet (a small case before a large one, then the catalogue's order); when none does,
    to the start of the first open requirement."""
    cases = dc.catalogue()
    need = set()
    for fa in dc.FAMILIES:
        for fb in dc.FAMILIES:
            need.add(("pair", fa, fb))
    for c in cases:
        for f in c.shares:
            need.add(("after_fail", c.name, f))
        if c.kind == "large":
            s = dc.small_of(c.family).name
            need.add(("then", c.name, s))
            need.add(("then", s, c.name))
    total = {k: sum(1 for r in need if r[0] == k) for k in ("pair", "after_fail", "then")}

    def met(a, b):
        out = {("pair", a.family, b.family), ("then", a.name, b.name)}
        if a.kind == "fail" and b.kind == "ok":
            out.add(("after_fail", a.name, b.family))
        return out & need

    def starts(r):
        return r[1] if r[0] != "pair" else dc.small_of(r[1]).name

    seq = [cases[0]]
    while need:
        cur = seq[-1]
        best = max(cases, key=lambda c: (len(met(cur, c)), c.kind != "large", -cases.index(c)))
        if not met(cur, best):
            first = min(need, key=lambda r: (("after_fail", "then", "pair").index(r[0]), r[1:]))
            best = dc.by_name(starts(first))
        need -= met(cur, best)
        seq.append(best)
    seq += [c for c in cases if c not in seq]  # (a second case of a family that no requirement asked for)
    rnd = random.Random(SEED)
    trims = set(rnd.sample(range(1, len(seq)), len(seq) // 10))
    return [(c.name, i in trims) for i, c in enumerate(seq)], total


def test_walk_coverage():
    steps, total = walk()
    names = [n for n, _ in steps]
    cases = [dc.by_name(n) for n in names]
    adjacent = list(zip(cases, cases[1:]))
    pairs = {(a.family, b.family) for a, b in adjacent}
    assert pairs == {(x, y) for x in dc.FAMILIES for y in dc.FAMILIES}
    fails = 0
    for c in dc.catalogue():
        for f in c.shares:
            assert any(a is c and b.family == f and b.kind == "ok" for a, b in adjacent), (c.name, f)
            fails += 1
        if c.kind == "large":
            s = dc.small_of(c.family)
            assert any(a is c and b is s for a, b in adjacent) and any(a is s and b is c for a, b in adjacent), c.name
    assert set(names) == set(dc.NAMES)
    trims = sum(1 for _, t in steps if t)
    assert trims == len(steps) // 10
    large = sum(1 for c in cases if c.kind == "large")
    print(f"walk: {len(steps)} calls ({large} large, {sum(1 for c in cases if c.kind == 'fail')} failing), {trims} trims; "
          f"{len(pairs)} family pairs, {fails} failing-then-successful, {total['then']} large/small transitions")
    assert total == {"pair": 400, "after_fail": fails, "then": 10}
    assert len(steps) <= 700  # (roughly 20 x 20 calls of a few milliseconds)


# ---- GPU ---------------------------------------------------------------------------
def torch_():
    import torch
    return torch


_BUFFERS = {}


def buffers(name):
    if name not in _BUFFERS:
        _BUFFERS[name] = dc.Buffers(dc.by_name(name))
    return _BUFFERS[name]


@functools.lru_cache(maxsize=None)
def baseline(name):
    """the case on a fresh context of its own, checked against expect()"""
    assert torch_().cuda.is_available(), "GPU test without a GPU"
    c = snappy_amd.Codec(0)
    try:
        return dc.run_plain(c, dc.by_name(name), buffers=buffers(name))
    finally:
        c.close()


def same_as_baseline(name, outs, res, where):
    want_outs, want_res = baseline(name)
    assert res == want_res, f"{where}: {name}: {res}, alone {want_res}"
    exp = dc.by_name(name).expect()
    for k, w in want_outs.items():
        care = exp.get(k + "#care")  # (a failing unit's own output range is not promised)
        bad = np.nonzero((outs[k] != w) & care if care is not None else outs[k] != w)[0]
        assert bad.size == 0, f"{where}: {name}: {k}[{bad[0]}] = {outs[k][bad[0]]}, alone {w[bad[0]]} ({bad.size} differ)"


@pytest.mark.gpu
@pytest.mark.parametrize("name", dc.NAMES)
def test_baseline(name):
    baseline(name)


@pytest.mark.gpu
def test_walk():
    torch = torch_()
    steps, _ = walk()
    for name in dc.NAMES:
        baseline(name)
    fresh = snappy_amd.Codec(0)
    c = snappy_amd.Codec(0)
    try:
        empty = fresh.device_bytes()
        for i, (name, trim) in enumerate(steps):
            if trim:
                c.trim()
            outs, res = dc.run_plain(c, dc.by_name(name), buffers=buffers(name))
            prev = steps[i - 1][0] if i else None
            same_as_baseline(name, outs, res, f"call {i} (after {prev}{', trim' if trim else ''})")
        # scratch accounting
        # the walk's last decode is still the context's status; reading it leaves none pending
        last = next(dc.by_name(n) for n, _ in reversed(steps) if dc.by_name(n).family in ("decode_streams",
                                                                                          "decode_single"))
        want = last.expect()
        assert c.decompress_status() == want.get("status", want["rc"])
        c.trim()
        assert c.device_bytes() == empty
        large, small = dc.by_name("compress_streams/large"), dc.by_name("compress_streams")
        dc.run_plain(c, large, buffers=buffers(large.name))
        held = c.device_bytes()
        # the token scratch alone: 8 (chunk / 4 + 2) bytes a unit, 2 bytes per input byte
        assert held >= 2 * (16 << 20)
        c.trim()
        dc.run_plain(c, small, buffers=buffers(small.name))
        assert empty < c.device_bytes() < held
    finally:
        c.close()
        fresh.close()


def queued_decode(c, name, decoy=False):
    """the queued decode of a catalogue case; nothing read back"""
    torch = torch_()
    case, b = dc.by_name(name), buffers(name)
    assert case.async_form and case.family in ("decode_streams", "decode_single")
    b.fill()
    b.load(b.alt if decoy else b.src)
    assert case.run(c, b.dev) == {"rc": 0}
    return case, b


OTHERS = ["compress_streams", "records_compress", "frame_decode", "ranges", "container_decode/hadoop"]


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["decode_streams/fail_async", "decode_single/fail_async"])
def test_status_survives_other_calls_and_trim(name):
    c = snappy_amd.Codec(0)
    try:
        assert c.decompress_status() == 0  # a context that has never decoded
        empty = c.device_bytes()
        queued_decode(c, name)
        for other in OTHERS:
            dc.run_plain(c, dc.by_name(other), buffers=buffers(other))
        c.trim()
        assert c.decompress_status() == E.ERR_OFFSET
        assert c.decompress_status() == E.ERR_OFFSET
        c.trim()
        assert c.device_bytes() == empty and c.decompress_status() == E.ERR_OFFSET
    finally:
        c.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["decode_streams/fail_async", "decode_single/fail_async"])
def test_status_words_of_good_units_are_written(name):
    """a successful queued decode of the same unit count directly after a failing one: the
    unit that failed last time must report OK (one status word per unit, never cleared)"""
    torch = torch_()
    c = snappy_amd.Codec(0)
    try:
        case, b = queued_decode(c, name)
        case, b = queued_decode(c, name, decoy=True)  # (the failing one's status is never read)
        assert c.decompress_status() == 0
        torch.cuda.synchronize()
        dc.compare(case, case.expect_decoy(), b.read(), {"rc": 0, "status": 0})
    finally:
        c.close()


@pytest.mark.gpu
@pytest.mark.parametrize("first,then", [("decode_streams/fail_async", "decode_single"),
                                        ("decode_single/fail_async", "decode_streams")])
def test_status_follows_the_last_launch(first, then):
    """a failure in one layout, a success in the other, and the reverse: the status is
    the last launch's, read with the last launch's unit count and mapping"""
    c = snappy_amd.Codec(0)
    try:
        queued_decode(c, first)
        queued_decode(c, then)
        assert c.decompress_status() == 0
        queued_decode(c, then)
        queued_decode(c, first)
        assert c.decompress_status() == E.ERR_OFFSET
        assert c.decompress_status() == E.ERR_OFFSET
    finally:
        c.close()


@pytest.mark.gpu
def test_empty_decode_clears_the_last_status():
    """a decode of no bytes is a decode: the failure read before it is not reported again"""
    c = snappy_amd.Codec(0)
    try:
        case, b = queued_decode(c, "decode_streams/fail_async")
        assert c.decompress_status() == E.ERR_OFFSET
        c.decompress_ptr(b.dev["comp"].data_ptr(), b.dev["offs"].data_ptr(), 0, 8192, E.STREAMS,
                         b.dev["out"].data_ptr(), check=False)
        assert c.decompress_status() == 0
        queued_decode(c, "decode_streams/fail_async")  # pending, then an empty decode: nothing left to read
        c.decompress_ptr(b.dev["comp"].data_ptr(), b.dev["offs"].data_ptr(), 0, 8192, E.STREAMS,
                         b.dev["out"].data_ptr(), check=False)
        assert c.decompress_status() == 0
    finally:
        c.close()

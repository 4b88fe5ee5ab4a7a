"""GPU: range decode of Hadoop and snappy-java containers -- the
device call through Codec.decompress_container_ranges_tensor, the host twin of the
walk (snappy_container_tables) and the host forms.

The containers are container_ranges_cases' (hand-written payloads) and the model's
wrapping of the oracle's streams, the tables container_model's walk, the wanted
bytes slices of the plain bytes the containers were made from.  Every call decodes
into a buffer filled with a sentinel and the whole buffer is compared: the accepted
ranges' bytes where they belong, the sentinel everywhere else."""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

import container_cases as cc
import container_model as cm
import container_ranges_cases as rc
import container_ranges_model as crm
import datagen
import oracle
import snappy_amd

pytestmark = pytest.mark.gpu

FORMATS = [cm.HADOOP, cm.XERIAL]
SENT = rc.SENT
BLOCK = 65536


def dev(b) -> torch.Tensor:
    return torch.from_numpy(np.frombuffer(bytes(b), dtype=np.uint8).copy()).cuda() if len(b) else \
        torch.empty(0, dtype=torch.uint8, device="cuda")


def flat(p) -> torch.Tensor:
    v = [x - (1 << 64) if x >= 1 << 63 else x for q in p for x in q]
    return torch.tensor(v, dtype=torch.int64, device="cuda")


def pairs(t):
    v = t.cpu().tolist()
    return list(zip(v[0::2], v[1::2]))


def decode(codec, window, origin, comp, outp, ranges, out_bytes):
    """-> (the call's status, the ranges' statuses, the whole output buffer)"""
    out = torch.full((max(out_bytes, 1),), SENT, dtype=torch.uint8, device="cuda")
    _, st = codec.decompress_container_ranges_tensor(window, origin, flat(comp), flat(outp), ranges, out=out[:out_bytes])
    return codec.last_ranges_status, [int(x) for x in st.cpu().numpy()], out.cpu().numpy().tobytes()


def compare(got, raw, ranges, st, out_bytes, partial=()):
    """the buffer against the slices of the ranges with status 0; a failing range leaves
    the sentinel, unless it is in `partial` (it failed while decoding: its own output
    range may be partly written and is not compared)"""
    want = bytearray(rc.expected(raw, ranges, out_bytes, {i for i, s in enumerate(st) if s == 0}))
    for i in partial:
        a, ln, oo = ranges[i]
        want[oo:oo + ln] = got[oo:oo + ln]
    if got != bytes(want):
        bad = next(i for i in range(len(got)) if got[i] != want[i])
        raise AssertionError(f"output differs at byte {bad}: {got[bad]:#x} for {want[bad]:#x}")


def first_failure(st):
    return next((s for s in st if s != 0), 0)


def code(fn, *a, **k):
    try:
        fn(*a, **k)
        return 0
    except snappy_amd.SnappyError as e:
        return e.code


# ---- every slice of small containers ----------------------------------------
@pytest.mark.parametrize("name", list(rc.SLICE))
def test_every_slice(codec, name):
    fmt, stream, raw, comp, outp, ranges, out_bytes = rc.slice_case(name)
    cont = dev(stream)
    n, dcomp, doutp = codec.container_index_tensor(cont, fmt)
    assert (n, pairs(dcomp), pairs(doutp)) == (len(raw), comp, outp)
    rcode, st, got = decode(codec, cont, 0, comp, outp, ranges, out_bytes)
    assert rcode == 0 and st == [0] * len(ranges)
    compare(got, raw, ranges, st, out_bytes)


# ---- long chunks ------------------------------------------------------------
def text(n, seed):
    return datagen.make("T", n, seed).tobytes()


@functools.lru_cache(maxsize=None)
def long_case(fmt):
    """chunks 1 and 4 the oracle's streams of text, chunk 3 stored random bytes, chunk 2 the foreign one"""
    stream, raw = rc.long_case(fmt, compress=lambda r: oracle.compress(r) if len(r) != BLOCK else cc.stored(r),
                               content=lambda n, seed: text(n, seed) if n != BLOCK else cc.content(n, seed))
    comp, outp, total = crm.tables(stream, fmt)
    return stream, raw, comp, outp


@pytest.mark.parametrize("fmt", FORMATS)
def test_long_chunks(codec, fmt):
    stream, raw, comp, outp = long_case(fmt)
    assert [size for _, size in outp] == rc.LONG_SIZES
    at, c = comp[2]
    assert crm.defers_in_pass_one(stream[at:at + c]) and oracle.decompress(stream[at:at + c]) == \
        raw[outp[2][0]:outp[2][0] + outp[2][1]]
    ranges, out_bytes = rc.lay_out(rc.long_spans(outp))
    cont = dev(stream)
    assert codec.decompress_container_tensor(cont, fmt, flat(comp), flat(outp), cap=len(raw)).cpu().numpy().tobytes() == raw
    rcode, st, got = decode(codec, cont, 0, comp, outp, ranges, out_bytes)
    assert rcode == 0 and st == [0] * len(ranges)
    compare(got, raw, ranges, st, out_bytes)


# ---- staging ----------------------------------------------------------------
def grown(need):
    return need + need // 8 + 4096


def scratch_bound(budget, outp, units, count):
    """the header's bound on what a call adds to device_bytes()"""
    live = [u for u in units if u[4] not in (0, crm.BAD)]
    edge = [crm.stage_size(outp[u[0]][1]) for u in live if u[5]]
    total = sum(outp[u[0]][1] for u in live)
    return grown(max([budget] + edge) + 16) + grown(68 * len(units)) + grown(100 * count + 88) + \
        snappy_amd.max_long_records_scratch(total, len(units))


def test_edge_chunks_reuse_a_staging_area_of_three_blocks(codec, monkeypatch):
    monkeypatch.setenv("SNAPPY_AMD_RANGE_SLOTS", "3")
    budget = 3 * BLOCK
    stream, raw = rc.uniform(cm.XERIAL, 8, 4096, 80)
    comp, outp, total = crm.tables(stream, cm.XERIAL)
    ranges, out_bytes = rc.lay_out(rc.staging_spans(total, 40, 3))
    _, units = crm.plan(outp, ranges, out_bytes)
    assert sum(1 for u in units if u[5]) >= 67 and len(crm.pack(outp, units, budget)[1]) == 2
    codec.trim()
    base = codec.device_bytes()
    rcode, st, got = decode(codec, dev(stream), 0, comp, outp, ranges, out_bytes)
    assert rcode == 0 and st == [0] * 40
    compare(got, raw, ranges, st, out_bytes)
    assert codec.device_bytes() - base <= scratch_bound(budget, outp, units, 40)


def test_an_edge_chunk_above_the_staging_budget(codec, monkeypatch):
    monkeypatch.setenv("SNAPPY_AMD_RANGE_SLOTS", "3")
    budget = 3 * BLOCK
    p = [cc.content(100, 90), text(262144, 91), cc.content(100, 92)]
    stream = rc.container(cm.HADOOP, [cc.stored(p[0]), oracle.compress(p[1]), cc.stored(p[2])], [100, 262144, 100])
    raw = b"".join(p)
    comp, outp, total = crm.tables(stream, cm.HADOOP)
    ranges, out_bytes = rc.lay_out([(1, 99), (50, 200), (150, 262344 - 50), (262244, 262343), (99, 262245)])
    _, units = crm.plan(outp, ranges, out_bytes)
    places, gstart, stage = crm.pack(outp, units, budget)
    assert stage == 262144 > budget and len(gstart) >= 3
    codec.trim()
    base = codec.device_bytes()
    rcode, st, got = decode(codec, dev(stream), 0, comp, outp, ranges, out_bytes)
    assert rcode == 0 and st == [0] * len(ranges)
    compare(got, raw, ranges, st, out_bytes)
    grew = codec.device_bytes() - base
    assert grown(262144 + 16) <= grew <= scratch_bound(budget, outp, units, len(ranges))


# ---- the window -------------------------------------------------------------
@pytest.mark.parametrize("fmt", FORMATS)
def test_window_and_sub_tables(codec, fmt):
    stream, raw, comp, outp = long_case(fmt)
    ranges = [(outp[1][0] + 7, outp[4][0] - 9 - (outp[1][0] + 7), 3), (outp[2][0] + 10, 500, 270000)]
    out_bytes = 271000
    whole = decode(codec, dev(stream), 0, comp, outp, ranges, out_bytes)
    assert whole[:2] == (0, [0, 0])
    compare(whole[2], raw, ranges, whole[1], out_bytes)
    w0, w1 = comp[1][0], comp[3][0] + comp[3][1]       # the payloads of chunks 1 .. 3, exactly
    sub_c, sub_o = comp[1:4], outp[1:4]
    for res in range(4):
        buf = torch.full((w1 - w0 + 64,), 0xFF, dtype=torch.uint8, device="cuda")
        buf[res:res + w1 - w0] = dev(stream[w0:w1])
        win = buf[res:res + w1 - w0]
        assert win.data_ptr() % 4 == res
        assert decode(codec, win, w0, sub_c, sub_o, ranges, out_bytes) == whole
        # one byte short at the end: chunk 3 is not resident; the range inside chunk 2 does not notice
        rcode, st, got = decode(codec, win[:-1], w0, sub_c, sub_o, ranges, out_bytes)
        assert st == [snappy_amd.ERR_TRUNCATED, 0] and rcode == snappy_amd.ERR_TRUNCATED
        compare(got, raw, ranges, st, out_bytes)
        # starting one byte late: chunk 1 is not resident
        rcode, st, got = decode(codec, win[1:], w0 + 1, sub_c, sub_o, ranges, out_bytes)
        assert st == [snappy_amd.ERR_TRUNCATED, 0] and rcode == snappy_amd.ERR_TRUNCATED
        compare(got, raw, ranges, st, out_bytes)
    # a range that leaves the sub-table is refused by the plan, at either end
    a, b = outp[1][0], outp[3][0] + outp[3][1]
    rcode, st, got = decode(codec, dev(stream[w0:w1]), w0, sub_c, sub_o,
                            [(a - 1, 2, 0), (b - 1, 2, 8), (a, 1, 16), (b - 1, 1, 24)], 32)
    assert st == [snappy_amd.ERR_ARG, snappy_amd.ERR_ARG, 0, 0]
    assert got[16] == raw[a] and got[24] == raw[b - 1]


# ---- the status rule --------------------------------------------------------
P5 = [cc.content(n, 30 + n) for n in (3000, 500, 2000, 700, 900)]
CUT_LITERAL = cm.varint(2000) + bytes([61 << 2, 0xCF, 0x07])      # a literal with no bytes behind it
FAR_COPY = cm.varint(2000) + bytes([3 << 2]) + b"abcd" + bytes([0x01, 5])   # a copy from before its chunk


def five(fmt, third=None):
    """(container, comp, outp) of the five chunks, chunk 2's payload replaced by `third`"""
    payloads = [oracle.compress(P5[0]), cc.stored(P5[1]), third or oracle.compress(P5[2]), cc.stored(P5[3]),
                oracle.compress(P5[4])]
    stream = rc.container(fmt, payloads, [len(x) for x in P5], header_before=(3,))
    comp, outp, total = crm.tables(stream, fmt)
    assert total == 7100
    return stream, comp, outp


def contract_status(codec, fmt, stream, comp, outp, chunks, window=None):
    """what decompress_container_device (tables given) returns for a container of exactly
    these chunks of `stream`, their table entries carried over"""
    payloads = [stream[comp[u][0]:comp[u][0] + max(comp[u][1], 1)] for u in chunks]
    small = rc.container(fmt, payloads, [outp[u][1] for u in chunks])
    at, c2, o2, total = [], [], [], 0
    pos = 0 if fmt == cm.HADOOP else 16
    for k, u in enumerate(chunks):
        pos += 4 + (4 if fmt == cm.HADOOP and k == 0 else 0)
        c2.append((pos, comp[u][1]))
        o2.append((total, outp[u][1]))
        pos += len(payloads[k])
        total += outp[u][1]
    clen = len(small)
    if window is not None:                              # the container cut where the window cuts the last payload
        clen = c2[-1][0] + window
    return code(codec.decompress_container_tensor, dev(small), fmt, flat(c2), flat(o2), cap=total, clen=clen)


STATUS_CASES = {
    # name -> (chunk 2's payload, what is done to the tables, the status, fails while decoding)
    "cut literal": (CUT_LITERAL, None, snappy_amd.ERR_TRUNCATED, True),
    "copy before the chunk": (FAR_COPY, None, snappy_amd.ERR_OFFSET, True),
    "a preamble that is not the table's length": (None, "len + 1", snappy_amd.ERR_HEADER, False),
    "comp_len 0": (None, "comp_len 0", snappy_amd.ERR_HEADER, False),
}


@pytest.mark.parametrize("name", list(STATUS_CASES))
@pytest.mark.parametrize("fmt", FORMATS)
def test_status_of_a_bad_chunk(codec, fmt, name):
    third, tamper, want, decoding = STATUS_CASES[name]
    stream, comp, outp = five(fmt, third)
    raw = P5[0] + P5[1] + (bytes(2000) if third else P5[2]) + P5[3] + P5[4]
    o = [a for a, _ in outp] + [7100]
    spans = [(o[2], o[3]),                 # chunk 2 alone, whole
             (o[1] + 9, o[4] - 9),         # chunks 1 .. 3: chunk 2 interior
             (5, o[2]), (o[3], o[5] - 1), (o[1] + 1, o[2] - 1),   # healthy neighbours
             (o[2] + 1, o[3] - 1),         # chunk 2 as a staged unit
             (o[1] + 9, o[2] + 2)]         # ... and as a range's last edge
    spans_chunks = [[2], [1, 2, 3], None, None, None, [2], [1, 2]]
    if tamper == "len + 1":
        # the table claims one byte more for chunk 2 and moves the later chunks up: sorted and contiguous
        outp = outp[:2] + [(o[2], 2001)] + [(a + 1, n) for a, n in outp[3:]]
        spans = [(o[2], o[3] + 1), (o[1] + 9, o[4] - 8), (5, o[2]), (o[3] + 1, o[5]), (o[1] + 1, o[2] - 1),
                 (o[2] + 1, o[3]), (o[1] + 9, o[2] + 2)]
        raw = raw[:o[3]] + b"?" + raw[o[3]:]
    elif tamper == "comp_len 0":
        comp = comp[:2] + [(comp[2][0], 0)] + comp[3:]
    ranges, out_bytes = rc.lay_out(spans)
    for chunks in spans_chunks:
        if chunks:
            assert contract_status(codec, fmt, stream, comp, outp, chunks) == want
    assert contract_status(codec, fmt, stream, comp, outp, [0, 1]) == 0
    rcode, st, got = decode(codec, dev(stream), 0, comp, outp, ranges, out_bytes)
    assert st == [want, want, 0, 0, 0, want, want] and rcode == want
    ok = lambda payload: {CUT_LITERAL: snappy_amd.ERR_TRUNCATED, FAR_COPY: snappy_amd.ERR_OFFSET}.get(payload, 0)  # noqa: E731
    assert [crm.range_status(stream, comp, outp, r, out_bytes, ok) for r in ranges] == \
        [(s, not decoding) if s else (0, False) for s in st]
    compare(got, raw, ranges, st, out_bytes, partial=(0, 1, 5, 6) if decoding else ())


@pytest.mark.parametrize("fmt", FORMATS)
def test_status_of_a_payload_cut_by_the_window(codec, fmt):
    stream, comp, outp = five(fmt)
    raw = b"".join(P5)
    o = [a for a, _ in outp] + [7100]
    ranges, out_bytes = rc.lay_out([(o[1] + 9, o[3]), (o[2] + 1, o[3] - 1), (5, o[2]), (o[1], o[2])])
    cut = comp[2][1] - 1                                # the window ends one byte inside chunk 2's payload
    assert contract_status(codec, fmt, stream, comp, outp, [1, 2], window=cut) == snappy_amd.ERR_TRUNCATED
    assert contract_status(codec, fmt, stream, comp, outp, [2], window=cut) == snappy_amd.ERR_TRUNCATED
    win = dev(stream[:comp[2][0] + cut])
    rcode, st, got = decode(codec, win, 0, comp, outp, ranges, out_bytes)
    assert st == [snappy_amd.ERR_TRUNCATED, snappy_amd.ERR_TRUNCATED, 0, 0] and rcode == snappy_amd.ERR_TRUNCATED
    compare(got, raw, ranges, st, out_bytes)


@pytest.mark.parametrize("fmt", FORMATS)
def test_lowest_failing_chunk_wins(codec, fmt):
    for a, b, want in ((CUT_LITERAL, FAR_COPY, snappy_amd.ERR_TRUNCATED), (FAR_COPY, CUT_LITERAL, snappy_amd.ERR_OFFSET)):
        payloads = [oracle.compress(P5[0]), a, cc.stored(P5[4]), b]
        stream = rc.container(fmt, payloads, [3000, 2000, 900, 2000])
        comp, outp, total = crm.tables(stream, fmt)
        assert contract_status(codec, fmt, stream, comp, outp, [0, 1, 2, 3]) == want
        ranges = [(1, total - 2, 7), (0, 3000, 8000)]
        rcode, st, got = decode(codec, dev(stream), 0, comp, outp, ranges, 11100)
        assert st == [want, 0] and rcode == want
        compare(got, P5[0] + bytes(4900), ranges, st, 11100, partial=(0,))
    # a table failure in a later chunk refuses the range before the earlier chunk's element error is met
    stream = rc.container(fmt, [oracle.compress(P5[0]), CUT_LITERAL, cc.stored(P5[4])], [3000, 2000, 900])
    comp, outp, total = crm.tables(stream, fmt)
    comp[2] = (comp[2][0], 0)
    ranges = [(1, total - 2, 7), (0, 3000, 8000), (10, 4000, 12000)]
    rcode, st, got = decode(codec, dev(stream), 0, comp, outp, ranges, 17000)
    assert st == [snappy_amd.ERR_HEADER, 0, snappy_amd.ERR_TRUNCATED] and rcode == snappy_amd.ERR_HEADER
    compare(got, P5[0] + bytes(2900), ranges, st, 17000, partial=(2,))   # nothing of range 0 is stored


# ---- hostile tables -----------------------------------------------------------
def model_status(stream, comp, outp, ranges, out_bytes):
    ok = lambda payload: 0  # noqa: E731  (these containers' payloads are sound)
    return [crm.range_status(stream, comp, outp, r, out_bytes, ok) for r in ranges]


def boundary_spans(outp):
    """every range whose ends fall on a chunk boundary +- 1"""
    n = outp[-1][0] + outp[-1][1]
    pts = sorted({p for b, size in outp for p in (b - 1, b, b + 1, b + size) if 0 <= p <= n})
    return [(a, b) for i, a in enumerate(pts) for b in pts[i + 1:]]


@pytest.mark.parametrize("what", ["offsets swapped", "an offset raised by 1", "a length raised by 1",
                                  "a length above 2^30", "payloads swapped"])
def test_hostile_tables(codec, what):
    fmt, stream, raw = rc.SLICE["hadoop: one block of five chunks (1, 17, 64, 200, 3)"]()
    comp, outp, total = crm.tables(stream, fmt)
    ranges, out_bytes = rc.lay_out(boundary_spans(outp))
    if what == "offsets swapped":
        outp[2], outp[3] = (outp[3][0], outp[2][1]), (outp[2][0], outp[3][1])
    elif what == "an offset raised by 1":
        outp[2] = (outp[2][0] + 1, outp[2][1])
    elif what == "a length raised by 1":
        outp[2] = (outp[2][0], outp[2][1] + 1)
    elif what == "a length above 2^30":
        outp[3] = (outp[3][0], (1 << 30) + 1)
    else:
        comp[1], comp[2] = comp[2], comp[1]
    model = model_status(stream, comp, outp, ranges, out_bytes)
    want = [m[0] for m in model]
    assert all(early for s, early in model if s != 0)   # every refusal comes before any decode
    assert 0 in want and {"offsets swapped": snappy_amd.ERR_INDEX, "an offset raised by 1": snappy_amd.ERR_INDEX,
                          "a length raised by 1": snappy_amd.ERR_INDEX, "a length above 2^30": snappy_amd.ERR_UNSUPPORTED,
                          "payloads swapped": snappy_amd.ERR_HEADER}[what] in want
    rcode, st, got = decode(codec, dev(stream), 0, comp, outp, ranges, out_bytes)
    assert st == want and rcode == first_failure(want)
    # an accepted range has passed every unit's check against the chunk's own preamble and its
    # neighbours' offsets: its bytes are what its table entries' payloads decode to, placed by
    # the tables' offsets (success does not prove that the tables are the container's); the
    # sentinel everywhere else
    accepted = {i for i, s in enumerate(st) if s == 0}
    assert got == rc.planned(stream, comp, outp, ranges, out_bytes, accepted)
    if "offset" not in what:       # (a wrong length or payload is caught by the preamble: what is accepted is right)
        compare(got, raw, ranges, st, out_bytes)


# ---- refusals -----------------------------------------------------------------
def test_refusals_in_a_batch(codec):
    fmt, stream, raw = rc.SLICE["xerial: chunks of 200, 0, 1, 16, 33, the header again inside"]()
    comp, outp, n = crm.tables(stream, fmt)
    ranges = [(0, 6, 0), (n - 5, 6, 16), (70, 100, 32), (n + 1, 0, 0), (3, 0, 140), (n, 0, 140), (0, 100, 950),
              (0, 10, 1 << 63), (1 << 63, 1 << 63, 0), (2, n - 2, 200)]
    out_bytes = 200 + n - 2 + 20
    ranges[6] = (0, 100, out_bytes - 99)
    want = [0, snappy_amd.ERR_ARG, 0, snappy_amd.ERR_ARG, 0, 0, snappy_amd.ERR_CAPACITY, snappy_amd.ERR_CAPACITY,
            snappy_amd.ERR_ARG, 0]
    rcode, st, got = decode(codec, dev(stream), 0, comp, outp, ranges, out_bytes)
    assert st == want and rcode == snappy_amd.ERR_ARG
    compare(got, raw, ranges, st, out_bytes)
    # no ranges at all; no chunks at all
    assert decode(codec, dev(stream), 0, comp, outp, [], 16)[:2] == (0, [])
    rcode, st, got = decode(codec, dev(stream), 0, [], [], [(0, 0, 3), (0, 1, 3), (5, 0, 17)], 16)
    assert st == [0, snappy_amd.ERR_ARG, snappy_amd.ERR_CAPACITY] and got == bytes([SENT]) * 16


# ---- host forms ----------------------------------------------------------------
LIBC = ctypes.CDLL(None)
LIBC.fopen.restype = ctypes.c_void_p
LIBC.fopen.argtypes = [ctypes.c_char_p, ctypes.c_char_p]
LIBC.fdopen.restype = ctypes.c_void_p
LIBC.fdopen.argtypes = [ctypes.c_int, ctypes.c_char_p]
LIBC.fclose.argtypes = [ctypes.c_void_p]
LIBC.fseek.argtypes = [ctypes.c_void_p, ctypes.c_long, ctypes.c_int]


def file_range(path, fmt, a, ln, out_path, skip=0):
    """snappy_decompress_file_container_range on the file at `path` from byte `skip` -> (status, bytes written)"""
    fin, fout = LIBC.fopen(str(path).encode(), b"rb"), LIBC.fopen(str(out_path).encode(), b"wb")
    assert fin and fout
    if skip:
        LIBC.fseek(fin, skip, 0)
    rcode = snappy_amd.lib().snappy_decompress_file_container_range(fin, fmt, a, ln, fout)
    LIBC.fclose(fin)
    LIBC.fclose(fout)
    with open(out_path, "rb") as f:
        return rcode, f.read()


@pytest.mark.parametrize("name", list(rc.SLICE) + list(cc.FOREIGN))
def test_container_tables_is_the_device_walk(codec, name):
    fmt, stream, raw = (rc.SLICE.get(name) or cc.FOREIGN[name])()
    n, comp, outp = codec.container_index_tensor(dev(stream), fmt)
    assert snappy_amd.container_tables(stream, fmt) == (comp.cpu().tolist(), outp.cpu().tolist(), n)
    assert n == len(raw) and pairs(comp) == crm.tables(stream, fmt)[0]


def test_container_tables_capacity_and_errors():
    fmt, stream, raw = cc.FOREIGN["hadoop: chunks of no bytes inside a block"]()
    p = (ctypes.c_uint8 * len(stream)).from_buffer_copy(stream)
    room = (ctypes.c_uint64 * 8)()
    nch, total = ctypes.c_size_t(0), ctypes.c_uint64(0)
    f = snappy_amd.lib().snappy_container_tables
    assert f(p, len(stream), fmt, room, None, 3, ctypes.byref(nch), ctypes.byref(total)) == snappy_amd.ERR_CAPACITY
    assert nch.value == 4
    assert f(p, len(stream), fmt, None, room, 4, ctypes.byref(nch), ctypes.byref(total)) == 0
    assert list(room) == [0, 0, 0, 10, 10, 0, 10, 20] and total.value == 30
    assert f(p, len(stream), fmt, None, None, 0, ctypes.byref(nch), None) == 0 and nch.value == 4
    assert f(p, len(stream), 7, None, None, 0, None, None) == snappy_amd.ERR_ARG
    for name, (fmt, stream, want) in cc.walk_error_cases().items():
        with pytest.raises(snappy_amd.SnappyError) as e:
            snappy_amd.container_tables(stream, fmt)
        assert e.value.code == want, name


@pytest.mark.parametrize("fmt", FORMATS)
def test_host_forms(fmt, tmp_path):
    stream, raw, comp, outp = long_case(fmt)
    n = len(raw)
    snp, out = tmp_path / "in.snappy", tmp_path / "out.bin"
    snp.write_bytes(b"junk" + stream)                   # the FILE* form starts at the current position
    o = [a for a, _ in outp]
    for a, ln in ((0, n), (70001, 100000), (n - 1, 1), (5, 0), (n, 0), (o[2], outp[2][1]), (o[3] - 1, 2), (0, 1)):
        assert snappy_amd.decompress_container_range(stream, fmt, a, ln) == raw[a:a + ln], (a, ln)
        assert file_range(snp, fmt, a, ln, out, skip=4) == (0, raw[a:a + ln]), (a, ln)
    for a, ln in ((n - 5, 6), (n + 1, 0), (1 << 63, 1 << 63)):
        if ln < 1 << 32:
            assert code(snappy_amd.decompress_container_range, stream, fmt, a, ln) == snappy_amd.ERR_ARG
        assert file_range(snp, fmt, a, ln, out, skip=4)[0] == snappy_amd.ERR_ARG

    # only the 16 bytes of each step up to the range's last chunk and the range's payloads are used
    a, ln = o[2] + 5, o[4] - 9 - (o[2] + 5)             # chunks 2 and 3
    holed = bytearray(stream)
    for u, (at, c) in enumerate(comp):
        if u not in (2, 3) and c > 8:
            holed[at + 8:at + c] = b"\xee" * (c - 8)
    hs = tmp_path / "holed.snappy"
    hs.write_bytes(bytes(holed))
    assert snappy_amd.decompress_container_range(bytes(holed), fmt, a, ln) == raw[a:a + ln]
    assert file_range(hs, fmt, a, ln, out) == (0, raw[a:a + ln])
    # a chunk after the range destroyed (its length field): never seen
    after = bytearray(holed)
    after[comp[4][0] - 4:comp[4][0]] = b"\x00\x00\x00\x00"
    hs.write_bytes(bytes(after))
    assert code(snappy_amd.decompress_container, bytes(after), fmt) == snappy_amd.ERR_HEADER
    assert snappy_amd.decompress_container_range(bytes(after), fmt, a, ln) == raw[a:a + ln]
    assert file_range(hs, fmt, a, ln, out) == (0, raw[a:a + ln])
    # a chunk before the range destroyed: the walk's error
    before = bytearray(holed)
    before[comp[1][0] - 4:comp[1][0]] = b"\x00\x00\x00\x00"
    hs.write_bytes(bytes(before))
    assert code(snappy_amd.decompress_container_range, bytes(before), fmt, a, ln) == snappy_amd.ERR_HEADER
    assert file_range(hs, fmt, a, ln, out)[0] == snappy_amd.ERR_HEADER
    # a payload byte of the range's own chunk changed into a broken element: reported, not returned
    broken = bytearray(stream)
    broken[comp[3][0] + 3:comp[3][0] + 7] = b"\xff\xff\xff\xff"   # chunk 3's literal claims 2^32 bytes
    assert code(snappy_amd.decompress_container_range, bytes(broken), fmt, a, ln) != 0
    # a stream that ends behind chunk 1, before the range: what the whole decode says of it -- in
    # snappy-java a shorter stream, so the range leaves it; in Hadoop a block cut short
    short = stream[:comp[1][0] + comp[1][1]]
    want = snappy_amd.ERR_ARG if fmt == cm.XERIAL else snappy_amd.ERR_TRUNCATED
    assert code(snappy_amd.decompress_container, short, fmt) == (0 if fmt == cm.XERIAL else want)
    assert code(snappy_amd.decompress_container_range, short, fmt, a, ln) == want


def test_host_forms_on_small_containers(tmp_path):
    for name in rc.SLICE:
        fmt, stream, raw = rc.SLICE[name]()
        n = len(raw)
        snp, out = tmp_path / "in.snappy", tmp_path / "out.bin"
        snp.write_bytes(stream)
        for a, ln in ((0, n), (1, max(n - 2, 0)), (n // 2, n - n // 2), (n, 0)):
            assert snappy_amd.decompress_container_range(stream, fmt, a, ln) == raw[a:a + ln], (name, a, ln)
            assert file_range(snp, fmt, a, ln, out) == (0, raw[a:a + ln]), (name, a, ln)


def test_file_form_refuses_a_pipe(tmp_path):
    r, w = os.pipe()
    os.write(w, cc.HELLO_HADOOP)
    os.close(w)
    fin, fout = LIBC.fdopen(r, b"rb"), LIBC.fopen(str(tmp_path / "out.bin").encode(), b"wb")
    assert fin and fout
    assert snappy_amd.lib().snappy_decompress_file_container_range(fin, cm.HADOOP, 0, 5, fout) == snappy_amd.ERR_UNSUPPORTED
    LIBC.fclose(fin)
    LIBC.fclose(fout)
    assert snappy_amd.decompress_container_range(cc.HELLO_HADOOP, cm.HADOOP, 1, 3) == b"ell"
    assert snappy_amd.decompress_container_range(cc.HELLO_XERIAL, "xerial", 0, 5) == b"hello"

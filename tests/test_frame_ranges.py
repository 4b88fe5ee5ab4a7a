"""GPU: range decode of framed streams -- the seek table
(snappy_amd_frame_seek_device, snappy_frame_tables), the device call through
Codec.decompress_frame_ranges_tensor, the host forms and `snappy -d -f -R`.

The streams are test_frame's (the model's framing of the oracle's payloads), the
tables frame_model's walk and frame_ranges_model's seek table, the wanted bytes
slices of the plain bytes the streams were made from.  Every call decodes into a
buffer filled with a sentinel and the whole buffer is compared: the accepted
ranges' bytes where they belong, the sentinel everywhere else."""
import os
import random
import subprocess

import numpy as np
import pytest
import torch

import datagen
import frame_model as fm
import frame_ranges_cases as fc
import frame_ranges_model as frm
import oracle
import snappy_amd
from test_frame import FOREIGN, comp, pieces

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "lightweight-snappy_amd", "snappy")
CH = 65536
SENT = fc.SENT


def dev(b) -> torch.Tensor:
    return torch.from_numpy(np.frombuffer(bytes(b), dtype=np.uint8).copy()).cuda() if len(b) else \
        torch.empty(0, dtype=torch.uint8, device="cuda")


def i64(v) -> torch.Tensor:
    return torch.tensor([x - (1 << 64) if x >= 1 << 63 else x for x in v], dtype=torch.int64, device="cuda")


def decode(codec, window, origin, chunks, starts, ranges, out_bytes):
    """-> (the call's status, the ranges' statuses, the whole output buffer)"""
    out = torch.full((max(out_bytes, 1),), SENT, dtype=torch.uint8, device="cuda")
    _, st = codec.decompress_frame_ranges_tensor(window, origin, i64(chunks), i64(starts), ranges, out=out[:out_bytes])
    return codec.last_ranges_status, [int(x) for x in st.cpu().numpy()], out.cpu().numpy().tobytes()


def compare(got, raw, ranges, st, out_bytes, partial=()):
    """the buffer against the slices of the ranges with status 0; a failing range leaves
    the sentinel, unless it is in `partial` (it failed while decoding: its own output
    range may be partly written and is not compared)"""
    want = bytearray(fc.expected(raw, ranges, out_bytes, {i for i, s in enumerate(st) if s == 0}))
    for i in partial:
        a, ln, oo = ranges[i]
        want[oo:oo + ln] = got[oo:oo + ln]
    if got != bytes(want):
        bad = next(i for i in range(len(got)) if got[i] != want[i])
        raise AssertionError(f"output differs at byte {bad}: {got[bad]:#x} for {want[bad]:#x}")


def first_failure(st):
    return next((s for s in st if s != 0), 0)


# ---- the seek table ---------------------------------------------------------
@pytest.mark.parametrize("name", list(FOREIGN))
def test_seek_table_of_foreign_streams(codec, name):
    stream, raw = FOREIGN[name]()
    chunks, starts = fc.tables(stream)
    frame = dev(stream)
    n, table = codec.frame_index_tensor(frame)
    assert table.cpu().tolist() == chunks
    n2, got = codec.frame_seek_tensor(frame, table.contiguous())
    assert n2 == n == len(raw) and got.cpu().tolist() == starts
    assert snappy_amd.frame_tables(stream) == (chunks, starts, len(raw))  # the host twin


@pytest.mark.parametrize("n", [0, 1, 65536, 65537, 5 * 65536 + 17])
def test_seek_table_of_own_streams(codec, n):
    x = torch.from_numpy(datagen.make("T", max(n, 1), 4321)[:n].copy()).cuda() if n else dev(b"")
    frame, chunks = codec.compress_frame_tensor(x)
    total, starts = codec.frame_seek_tensor(frame, chunks)
    assert total == n and starts.cpu().tolist() == [min(CH * i, n) for i in range(chunks.numel())]
    assert frm.seek_table(frame.cpu().numpy().tobytes(), chunks.cpu().tolist()) == (0, starts.cpu().tolist())


def test_seek_table_refuses_entries_that_are_no_data_chunks(codec):
    stream, raw = FOREIGN["padding of 0 and of 7 bytes"]()
    chunks, starts = fc.tables(stream)
    frame = dev(stream)
    pad = stream.index(fm.padding(7), 10)           # the padding chunk of 7 bytes
    for table, want in (([chunks[0], pad, chunks[2], chunks[3]], snappy_amd.ERR_INDEX),
                        ([chunks[0], chunks[1], len(stream), chunks[3]], snappy_amd.ERR_TRUNCATED),
                        ([chunks[0], len(stream) + 100, pad, chunks[3]], snappy_amd.ERR_TRUNCATED)):  # the first wins
        assert frm.seek_table(stream, table)[0] == want
        with pytest.raises(snappy_amd.SnappyError) as e:
            codec.frame_seek_tensor(frame, i64(table))
        assert e.value.code == want
    assert codec.frame_seek_tensor(frame, i64(chunks))[1].cpu().tolist() == starts  # the context goes on working


# ---- every slice of small streams -------------------------------------------
@pytest.mark.parametrize("name", fc.SLICE_STREAMS)
def test_every_slice(codec, name):
    stream, raw = FOREIGN[name]()
    chunks, starts, ranges, out_bytes = fc.slice_case(stream)
    rc, st, got = decode(codec, dev(stream), 0, chunks, starts, ranges, out_bytes)
    assert rc == 0 and st == [0] * len(ranges)
    compare(got, raw, ranges, st, out_bytes)


# ---- stored chunks ----------------------------------------------------------
def stored_stream():
    """stored chunks of 1, 60, 61 and 65,536 bytes, each with its payload at each of
    the 4 address residues, between compressed chunks"""
    sizes = [s for s in (1, 60, 61, CH) for _ in range(4)]
    p = pieces([500] + sizes + [700], "R", seed=23)
    stream = bytearray(fm.IDENTIFIER + comp(p[0]))
    at = []
    for k, s in enumerate(sizes):
        stream += fm.padding((k % 4 - (len(stream) + 4 + 8)) % 4)
        at.append(len(stream))
        stream += fm.stored(p[1 + k])
    stream += comp(p[-1])
    assert sorted({(a + 8) % 4 for a in at[:4]}) == [0, 1, 2, 3]
    return bytes(stream), b"".join(p)


def test_stored_chunks(codec):
    stream, raw = stored_stream()
    chunks, starts = fc.tables(stream)
    spans = []
    for j in range(1, len(starts) - 2):               # the stored chunks
        b0, b1 = starts[j], starts[j + 1]
        size = b1 - b0
        spans.append((b0 - 1, b1 + 1))                # an interior unit
        spans.append((b0, b1))                        # the range's only unit, whole
        if size > 1:
            spans += [(b0 + 1, b1 + 1), (b0 - 1, b1 - 1)]           # first edge, last edge
            spans.append((b0 + size // 3, b0 + max(size // 3 + 1, size - size // 4)))  # a single edge unit
    ranges, out_bytes = fc.lay_out(spans)
    st_model, units = frm.plan(starts, ranges, out_bytes)
    stored = set(range(1, len(starts) - 2))
    assert any(u[0] in stored and u[5] == 0 for u in units) and sum(u[0] in stored and u[5] != 0 for u in units) >= 36
    rc, st, got = decode(codec, dev(stream), 0, chunks, starts, ranges, out_bytes)
    assert rc == 0 and st == [0] * len(ranges)
    compare(got, raw, ranges, st, out_bytes)


# ---- slot reuse -------------------------------------------------------------
def test_edge_units_reuse_three_slots(codec, monkeypatch):
    monkeypatch.setenv("SNAPPY_AMD_RANGE_SLOTS", "3")
    stream, raw = FOREIGN["uniform chunks of 4,096"]()
    chunks, starts = fc.tables(stream)
    chunks, starts = chunks[:9], starts[:9]           # 8 chunks of 4,096 (the tables of a prefix)
    rnd = random.Random(3)
    spans = []
    for k in range(40):                               # 40 edge ranges: inside one chunk, or across one to three boundaries
        a = rnd.randrange(1, 8 * 4096 - 2)
        b = min(a + rnd.choice([1, 100, 4096, 5000, 9000, 13000]), 8 * 4096 - 1)
        spans.append((a, b))
    ranges, out_bytes = fc.lay_out(spans)
    _, units = frm.plan(starts, ranges, out_bytes)
    assert sum(1 for u in units if u[5]) > 40 and any(u[5] == 0 for u in units)
    rc, st, got = decode(codec, dev(stream), 0, chunks, starts, ranges, out_bytes)
    assert rc == 0 and st == [0] * 40
    compare(got, raw, ranges, st, out_bytes)


# ---- the window -------------------------------------------------------------
def test_window_and_sub_tables(codec):
    stream, raw = FOREIGN["three runs"]()             # 65536, 100, 65536, 65536, 1, 40000
    chunks, starts = fc.tables(stream)
    w0, w1 = chunks[1], chunks[4]                     # chunks 1 .. 3, exactly
    sub_c, sub_s = chunks[1:5], starts[1:5]
    ranges = [(starts[1] + 7, starts[4] - 9 - (starts[1] + 7), 3), (starts[2] + 10, 500, 140000)]
    for res in range(4):
        buf = torch.full((w1 - w0 + 64,), 0xFF, dtype=torch.uint8, device="cuda")
        buf[res:res + w1 - w0] = dev(stream[w0:w1])
        win = buf[res:res + w1 - w0]
        assert win.data_ptr() % 4 == res
        rc, st, got = decode(codec, win, w0, sub_c, sub_s, ranges, 141000)
        assert rc == 0 and st == [0, 0]
        compare(got, raw, ranges, st, 141000)
        # one byte short at the end: chunk 3 is not resident; the range inside chunk 2 does not notice
        rc, st, got = decode(codec, win[:-1], w0, sub_c, sub_s, ranges, 141000)
        assert st == [snappy_amd.ERR_TRUNCATED, 0] and rc == snappy_amd.ERR_TRUNCATED
        compare(got, raw, ranges, st, 141000)
        # starting one byte late: chunk 1 is not resident
        rc, st, got = decode(codec, win[1:], w0 + 1, sub_c, sub_s, ranges, 141000)
        assert st == [snappy_amd.ERR_TRUNCATED, 0] and rc == snappy_amd.ERR_TRUNCATED
        compare(got, raw, ranges, st, 141000)
    # a range that leaves the sub-table is refused by the plan, at either end
    rc, st, got = decode(codec, dev(stream[w0:w1]), w0, sub_c, sub_s,
                         [(starts[1] - 1, 2, 0), (starts[4] - 1, 2, 8), (starts[1], 1, 16), (starts[4] - 1, 1, 24)], 32)
    assert st == [snappy_amd.ERR_ARG, snappy_amd.ERR_ARG, 0, 0]


# ---- the status rule ----------------------------------------------------------
def whole_status(codec, body_chunks):
    """what the whole-stream framed decode reports for the identifier and these chunks"""
    stream, table = bytearray(fm.IDENTIFIER), []
    for c in body_chunks:
        table.append(len(stream))
        stream += c
    table.append(len(stream))
    try:
        codec.decompress_frame_tensor(dev(stream), i64(table), 5 * CH)
        return 0
    except snappy_amd.SnappyError as e:
        return e.code


P5 = pieces([3000, 500, 2000, 700, 900], "R", seed=31)


def good5():
    return [comp(P5[0]), fm.stored(P5[1]), comp(P5[2]), fm.stored(P5[3]), comp(P5[4])]


def flipped(crc_of):
    return fm.mask(fm.crc32c(crc_of)) ^ 1


# name -> (the chunk, the decoded length the seek table claims for it, the status, fails while decoding)
BAD_CHUNKS = {
    "bad element": (fm.compressed(P5[2], fm.varint(2000) + bytes([61 << 2, 0xCF, 0x07])), 2000,
                    snappy_amd.ERR_TRUNCATED, True),
    "copy before the chunk": (fm.compressed(b"abcdabcd", fm.varint(8) + bytes([3 << 2]) + b"abcd" + bytes([0x01, 5])), 8,
                              snappy_amd.ERR_OFFSET, True),
    "flipped CRC, compressed": (fm.compressed(P5[2], oracle.compress(P5[2]), crc=flipped(P5[2])), 2000,
                                snappy_amd.ERR_CHECKSUM, True),
    "flipped CRC, stored": (fm.stored(P5[2], crc=flipped(P5[2])), 2000, snappy_amd.ERR_CHECKSUM, True),
    "len < 4": (b"\x00\x03\x00\x00abc", 5, snappy_amd.ERR_HEADER, False),
    "reserved type": (fm.chunk(0x02, b"abcdef"), 5, snappy_amd.ERR_UNSUPPORTED, False),
    "oversize preamble": (fm.chunk(0x00, bytes(4) + fm.varint(65537) + b"\x00a"), 5, snappy_amd.ERR_OVERRUN, False),
}


def assemble(body, sizes):
    """(stream, chunk table, seek table, plain bytes by the seek table's positions)"""
    stream, chunks, starts, total = bytearray(fm.IDENTIFIER), [], [], 0
    for c, s in zip(body, sizes):
        chunks.append(len(stream))
        starts.append(total)
        stream += c
        total += s
    return bytes(stream), chunks + [len(stream)], starts + [total]


@pytest.mark.parametrize("name", list(BAD_CHUNKS))
def test_status_of_a_bad_chunk(codec, name):
    bad, size, want, decoding = BAD_CHUNKS[name]
    body = good5()
    body[2] = bad
    sizes = [3000, 500, size, 700, 900]
    stream, chunks, starts = assemble(body, sizes)
    raw = P5[0] + P5[1] + bytes(size) + P5[3] + P5[4]
    ranges, out_bytes = fc.lay_out([(starts[2], starts[3]),              # chunk 2 alone
                                    (starts[1] + 9, starts[4] - 9),      # chunks 1 .. 3
                                    (5, starts[2]), (starts[3], starts[5] - 1), (starts[1] + 1, starts[2] - 1),
                                    (starts[2] + 1, starts[3] - 1),      # chunk 2 as a staged unit
                                    (starts[1] + 9, starts[2] + 2)])     # ... and as a range's last edge
    assert whole_status(codec, [bad]) == want and whole_status(codec, body[1:4]) == want
    rc, st, got = decode(codec, dev(stream), 0, chunks, starts, ranges, out_bytes)
    assert st == [want, want, 0, 0, 0, want, want] and rc == want
    compare(got, raw, ranges, st, out_bytes, partial=(0, 1, 5, 6) if decoding else ())


def test_lowest_failing_chunk_wins(codec):
    elem, crc = BAD_CHUNKS["bad element"][0], BAD_CHUNKS["flipped CRC, stored"][0]
    for body, want in (([comp(P5[0]), elem, comp(P5[4]), crc], snappy_amd.ERR_TRUNCATED),
                       ([comp(P5[0]), crc, comp(P5[4]), elem], snappy_amd.ERR_CHECKSUM)):
        stream, chunks, starts = assemble(body, [3000, 2000, 900, 2000])
        assert whole_status(codec, body) == want
        ranges = [(1, starts[4] - 2, 7), (0, 3000, 8000)]
        rc, st, got = decode(codec, dev(stream), 0, chunks, starts, ranges, 11100)
        assert st == [want, 0] and rc == want
        compare(got, P5[0] + bytes(5000), ranges, st, 11100, partial=(0,))


def test_header_failure_later_wins_over_a_crc_failure_earlier(codec):
    body = good5()
    body[1] = fm.stored(P5[1], crc=flipped(P5[1]))
    body[3] = BAD_CHUNKS["reserved type"][0]
    stream, chunks, starts = assemble(body, [3000, 500, 2000, 5, 900])
    assert whole_status(codec, body) == snappy_amd.ERR_UNSUPPORTED
    ranges = [(1, starts[5] - 2, 7), (0, 3000, 8000), (10, starts[3] - 10, 12000)]
    rc, st, got = decode(codec, dev(stream), 0, chunks, starts, ranges, 18000)
    assert st == [snappy_amd.ERR_UNSUPPORTED, 0, snappy_amd.ERR_CHECKSUM] and rc == snappy_amd.ERR_UNSUPPORTED
    # nothing of range 0 is stored: not even chunk 0, which is sound
    compare(got, P5[0] + P5[1] + P5[2] + bytes(905), ranges, st, 18000, partial=(2,))


# ---- hostile tables -----------------------------------------------------------
def model_status(stream, chunks, starts, ranges, out_bytes):
    ok = lambda body: (0, oracle.decompress(body))  # noqa: E731  (these streams' payloads are sound)
    return [frm.range_status(stream, chunks, starts, r, out_bytes, ok) for r in ranges]


@pytest.mark.parametrize("what", ["starts swapped", "starts raised by 1", "chunks entry inside a payload"])
def test_hostile_tables(codec, what):
    stream, raw = FOREIGN["three runs"]()
    chunks, starts = fc.tables(stream)
    ranges, out_bytes = fc.lay_out(fc.slice_spans(starts))
    if what == "starts swapped":
        starts[2], starts[3] = starts[3], starts[2]
    elif what == "starts raised by 1":
        starts[2] += 1
    else:
        chunks[3] += 12                               # 4 bytes into the payload
    model = model_status(stream, chunks, starts, ranges, out_bytes)
    want = [m[0] for m in model]
    assert all(early for s, early in model if s != 0)  # every refusal comes before any decode
    assert 0 in want and snappy_amd.ERR_INDEX in want if what != "chunks entry inside a payload" else len(set(want)) > 1
    rc, st, got = decode(codec, dev(stream), 0, chunks, starts, ranges, out_bytes)
    assert st == want and rc == first_failure(want)
    # an accepted range has passed every unit's check against the chunk's own header, so it
    # lies where the tables are still right: its bytes are the stream's; the sentinel elsewhere
    compare(got, raw, ranges, st, out_bytes)


# ---- refusals -----------------------------------------------------------------
def test_refusals_in_a_batch(codec):
    stream, raw = FOREIGN["rising sizes (a run each)"]()
    chunks, starts = fc.tables(stream)
    n = starts[-1]
    ranges = [(0, 6, 0), (n - 5, 6, 16), (700, 100, 32), (n + 1, 0, 0), (3, 0, 140), (n, 0, 140), (0, 100, 950),
              (0, 10, 1 << 63), (1 << 63, 1 << 63, 0), (2, n - 2, 200)]
    out_bytes = 200 + n - 2 + 20
    ranges[6] = (0, 100, out_bytes - 99)
    want = [0, snappy_amd.ERR_ARG, 0, snappy_amd.ERR_ARG, 0, 0, snappy_amd.ERR_CAPACITY, snappy_amd.ERR_CAPACITY,
            snappy_amd.ERR_ARG, 0]
    rc, st, got = decode(codec, dev(stream), 0, chunks, starts, ranges, out_bytes)
    assert st == want and rc == snappy_amd.ERR_ARG
    compare(got, raw, ranges, st, out_bytes)
    # no ranges at all
    assert decode(codec, dev(stream), 0, chunks, starts, [], 16)[:2] == (0, [])


# ---- host forms and the CLI -----------------------------------------------------
def text5():
    a = datagen.make("T", 4 * CH + 1234, 77)
    payload, offs = oracle.compress_streams(a, CH)
    return fm.frame_streams(a.tobytes(), payload.tobytes(), offs), a.tobytes()


def cli_range(path, a, ln, out):
    return subprocess.run([CLI, "-d", "-f", "-R", f"{a}:{ln}", str(path), str(out)], capture_output=True)


@pytest.mark.parametrize("which", ["text", "three runs"])
def test_host_forms_and_cli(which, tmp_path):
    stream, raw = text5() if which == "text" else FOREIGN["three runs"]()
    n = len(raw)
    snp, out = tmp_path / "in.sz", tmp_path / "out.bin"
    snp.write_bytes(stream)
    for a, ln in ((0, n), (70001, 100000), (n - 1, 1), (5, 0), (n, 0), (CH, CH), (CH - 1, 2), (0, 1)):
        assert snappy_amd.decompress_frame_range(stream, a, ln) == raw[a:a + ln], (a, ln)
        r = cli_range(snp, a, ln, out)
        assert r.returncode == 0 and out.read_bytes() == raw[a:a + ln], (a, ln, r.stderr)
    for a, ln in ((n - 5, 6), (n + 1, 0), (1 << 63, 1 << 63)):
        if ln < 1 << 32:
            with pytest.raises(snappy_amd.SnappyError) as e:
                snappy_amd.decompress_frame_range(stream, a, ln)
            assert e.value.code == snappy_amd.ERR_ARG
        r = cli_range(snp, a, ln, out)
        assert r.returncode == 1 and b"error -1" in r.stderr

    # only the headers up to the range's last chunk and the range's chunks are used
    chunks, starts = fc.tables(stream)
    a, ln = starts[2] + 5, starts[4] - 9 - (starts[2] + 5)   # chunks 2 and 3
    # (a chunk's decoded length is its payload's preamble: the walk's 16 bytes per chunk hold it)
    holed = bytearray(stream)
    for u in range(len(chunks) - 1):
        if u not in (2, 3) and chunks[u + 1] - chunks[u] > 16:
            holed[chunks[u] + 16:chunks[u + 1]] = b"\xee" * (chunks[u + 1] - chunks[u] - 16)
    hs = tmp_path / "holed.sz"
    hs.write_bytes(bytes(holed))
    assert snappy_amd.decompress_frame_range(bytes(holed), a, ln) == raw[a:a + ln]
    r = cli_range(hs, a, ln, out)
    assert r.returncode == 0 and out.read_bytes() == raw[a:a + ln], r.stderr
    # a header after the range destroyed: never seen
    after = bytearray(holed)
    after[chunks[4]:chunks[4] + 4] = b"\x00\x03\x00\x00"
    hs.write_bytes(bytes(after))
    assert snappy_amd.decompress_frame_range(bytes(after), a, ln) == raw[a:a + ln]
    r = cli_range(hs, a, ln, out)
    assert r.returncode == 0 and out.read_bytes() == raw[a:a + ln], r.stderr
    # a header before the range destroyed: the walk's error
    before = bytearray(holed)
    before[chunks[1]:chunks[1] + 4] = b"\x00\x03\x00\x00"
    hs.write_bytes(bytes(before))
    with pytest.raises(snappy_amd.SnappyError) as e:
        snappy_amd.decompress_frame_range(bytes(before), a, ln)
    assert e.value.code == snappy_amd.ERR_HEADER
    r = cli_range(hs, a, ln, out)
    assert r.returncode == 1 and b"error -2" in r.stderr
    # a payload byte of the range's own chunk changed: the slice does not come back unverified
    broken = bytearray(holed)
    broken[chunks[3] - 1] ^= 0x40                      # chunk 2's last payload byte
    with pytest.raises(snappy_amd.SnappyError):
        snappy_amd.decompress_frame_range(bytes(broken), a, ln)


def test_cli_refuses_pipes_and_containers(tmp_path):
    stream, raw = FOREIGN["three runs"]()
    snp, out = tmp_path / "in.sz", tmp_path / "out.bin"
    snp.write_bytes(stream)
    r = subprocess.run([CLI, "-d", "-F", "hadoop", "-R", "0:1", str(snp), str(out)], capture_output=True)
    assert r.returncode == 1 and b"snappy [-c|-d|-b]" in r.stderr
    r = subprocess.run([CLI, "-c", "-f", "-R", "0:1", str(snp), str(out)], capture_output=True)
    assert r.returncode == 1 and b"snappy [-c|-d|-b]" in r.stderr
    # a bare stream has no identifier
    bare = tmp_path / "in.snp"
    bare.write_bytes(oracle.compress(raw[:1000]))
    r = cli_range(bare, 0, 1, out)
    assert r.returncode == 1 and b"error -2" in r.stderr
    # a pipe cannot seek
    fifo = tmp_path / "pipe.sz"
    os.mkfifo(fifo)
    p = subprocess.Popen([CLI, "-d", "-f", "-R", "0:10", str(fifo), str(out)], stderr=subprocess.PIPE)
    try:
        with open(fifo, "wb") as w:                   # (returns once the CLI has opened its end)
            w.write(stream)
    except BrokenPipeError:
        pass                                          # the CLI refused the pipe without reading it
    err = p.communicate()[1]
    assert p.returncode != 0 and b"error -9" in err, err

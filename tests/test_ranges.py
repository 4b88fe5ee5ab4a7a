"""GPU: range decode -- snappy_amd_decompress_ranges_device
through Codec.decompress_ranges_tensor, the host forms and `snappy -d -R`.

Unless a test says otherwise the input is datagen text of 4 * 65,536 + 1,234
bytes compressed as one SINGLE stream, every range is decoded into a buffer
filled with a sentinel, and the whole buffer is compared: the range's bytes
where they belong, the sentinel everywhere else."""
import os
import struct
import subprocess

import numpy as np
import pytest

import datagen
import oracle
import ranges_cases as rc
import ranges_model as rm
import snappy_amd
from golden_inputs import build_stream, random_ops

pytestmark = pytest.mark.gpu

B = 65536
N = 4 * B + 1234
SENT = 0xA5
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "lightweight-snappy_amd", "snappy")
EDGES = [(0, 0), (0, 1), (0, N), (N - 1, N), (65535, 65537), (65536, 131072), (1, 65536), (65541, 196608),
         (100, 262144), (4 * B + 100, 4 * B + 900)]


def up(data):
    import torch
    a = np.frombuffer(bytes(data), dtype=np.uint8).copy() if not isinstance(data, np.ndarray) else np.array(data)
    return torch.from_numpy(a).cuda() if a.size else torch.empty(0, dtype=torch.uint8, device="cuda")


class Stream:
    def __init__(self, codec, data, chunk=B, layout=snappy_amd.SINGLE):
        self.data = np.frombuffer(bytes(data), dtype=np.uint8)
        self.n, self.chunk, self.layout = self.data.size, chunk, layout
        self.comp, self.offs = codec.compress_tensor(up(self.data), chunk=chunk, layout=layout)
        self.entries = [int(x) for x in self.offs.cpu().numpy()]


@pytest.fixture(scope="module")
def text(codec):
    return Stream(codec, datagen.make("T", N, 77).tobytes())


def decode(codec, s, ranges, out_bytes, comp=None, origin=0, offs=None, want=None):
    """-> (rc, statuses, the output buffer); the buffer is checked against the
    ranges in `want` (default: those with status 0): their bytes, the sentinel
    elsewhere.  A range that fails while it decodes may leave part of its own
    output range written: those bytes are not compared; one refused before any
    load or store (ERR_ARG, ERR_CAPACITY, ERR_TRUNCATED) must leave the sentinel."""
    import torch
    out = torch.full((max(out_bytes, 1),), SENT, dtype=torch.uint8, device="cuda")
    _, st = codec.decompress_ranges_tensor(s.comp if comp is None else comp, s.offs if offs is None else offs, s.n,
                                           ranges, out=out[:out_bytes], chunk=s.chunk, layout=s.layout,
                                           comp_origin=origin)
    st = [int(x) for x in st.cpu().numpy()]
    got = out.cpu().numpy()
    exp = np.full(max(out_bytes, 1), SENT, dtype=np.uint8)
    for i, (a, ln, oo) in enumerate(ranges):
        if (want is None and st[i] == 0) or (want is not None and i in want):
            exp[oo:oo + ln] = s.data[a:a + ln]
    early = (snappy_amd.ERR_ARG, snappy_amd.ERR_CAPACITY, snappy_amd.ERR_TRUNCATED)
    for i, (a, ln, oo) in enumerate(ranges):
        if st[i] != 0 and st[i] not in early:
            exp[oo:oo + ln] = got[oo:oo + ln]
    bad = np.nonzero(got != exp)[0]
    assert bad.size == 0, (bad[:8], ranges[:4])
    return codec.last_ranges_status, st, got


def residues(a, b, gap=3):
    """16 copies of the range [a, b), one at each output residue mod 16, sentinels between"""
    out, oo = [], 0
    for k in range(16):
        oo += gap
        oo += (k - oo) % 16
        out.append((a, b - a, oo))
        oo += b - a
    return out, oo + gap


@pytest.mark.parametrize("a,b", EDGES)
def test_edges_at_every_output_residue(codec, text, a, b):
    ranges, need = residues(a, b)
    rcode, st, _ = decode(codec, text, ranges, need, want=set(range(16)))
    assert rcode == 0 and st == [0] * 16


def test_batch_with_refused_ranges(codec, text):
    ranges, oo = [], 5
    for k, (a, b) in enumerate(EDGES):
        ranges.append((a, b - a, oo))
        oo += b - a + k + 1
    out_bytes = oo
    ranges.insert(3, (N - 5, 6, 0))                   # leaves n
    ranges.insert(6, (100, 50, out_bytes - 49))       # its output leaves out_bytes
    ranges.append((N + 1, 0, 0))                      # starts past n, even though empty
    ranges.append((0, 10, 1 << 63))
    want = [0] * len(ranges)
    want[3], want[6], want[-2], want[-1] = snappy_amd.ERR_ARG, snappy_amd.ERR_CAPACITY, snappy_amd.ERR_ARG, \
        snappy_amd.ERR_CAPACITY
    rcode, st, _ = decode(codec, text, ranges, out_bytes)
    assert st == want
    assert rcode == snappy_amd.ERR_ARG  # the first failure


def test_first_failure_is_the_first_failing_range(codec, text):
    rcode, st, _ = decode(codec, text, [(0, 10, 0), (0, 10, 1 << 40), (N, 1, 0)], 64)
    assert st == [0, snappy_amd.ERR_CAPACITY, snappy_amd.ERR_ARG] and rcode == snappy_amd.ERR_CAPACITY


def test_many_one_byte_ranges_reuse_the_slots(codec, text, monkeypatch):
    monkeypatch.setenv("SNAPPY_AMD_RANGE_SLOTS", "7")
    rng = np.random.default_rng(5)
    starts = rng.integers(0, N, 3000)
    ranges = [(int(s), 1, 2 * i + 1) for i, s in enumerate(starts)]
    rcode, st, _ = decode(codec, text, ranges, 6001)
    assert rcode == 0 and st == [0] * 3000


def test_async_call_without_statuses(codec, text):
    import torch
    out = torch.full((1000,), SENT, dtype=torch.uint8, device="cuda")
    got, st = codec.decompress_ranges_tensor(text.comp, text.offs, N, [(70000, 900, 50)], out=out, want_status=False)
    assert st is None and codec.last_ranges_status == 0
    torch.cuda.synchronize()
    g = got.cpu().numpy()
    assert np.array_equal(g[50:950], text.data[70000:70900]) and (g[:50] == SENT).all() and (g[950:] == SENT).all()


@pytest.mark.parametrize("kind", ["repeat8k", "random"])
def test_staged_history_and_long_literals(codec, kind):
    """an edge block whose copies reach further back than the 4,096-byte ring (they
    read the staging slot), and one that is a single 65,536-byte literal (HBM to HBM)"""
    piece = datagen.make("R", 8192, 9).tobytes()
    mid = piece * 8 if kind == "repeat8k" else datagen.make("R", B, 10).tobytes()
    s = Stream(codec, datagen.make("T", B, 1).tobytes() + mid + datagen.make("T", 3000, 2).tobytes())
    size = s.entries[2] - s.entries[1]
    assert size < B // 2 if kind == "repeat8k" else size >= B  # (copies 8,192 back; one stored literal)
    ranges, oo = [], 0
    for lo, hi in ((1, B), (4097, B), (0, 65535), (1, 65535), (4097, 65535)):
        for res in (0, 5, 11):
            oo += 16 + (res - oo) % 16
            ranges.append((B + lo, hi - lo, oo))
            oo += hi - lo
    rcode, st, _ = decode(codec, s, ranges, oo + 7)
    assert rcode == 0 and st == [0] * len(ranges)


def test_window_of_the_compressed_stream(codec, text):
    import torch
    e = text.entries
    a, b = 65541, 196608                     # blocks 1 and 2
    w0, w1 = e[1], e[3]
    comp = text.comp.cpu().numpy()
    for res in range(4):
        buf = torch.full((w1 - w0 + 64,), 0xFF, dtype=torch.uint8, device="cuda")
        buf[res:res + w1 - w0] = up(comp[w0:w1])
        win = buf[res:res + w1 - w0]
        assert win.data_ptr() % 4 == res
        rcode, st, _ = decode(codec, text, [(a, b - a, 3), (B, 100, 140000)], 150000, comp=win, origin=w0)
        assert rcode == 0 and st == [0, 0]
        # one byte short: block 2 is not resident; the range inside block 1 does not notice
        rcode, st, _ = decode(codec, text, [(a, b - a, 3), (B, 100, 140000)], 150000, comp=win[:-1], origin=w0)
        assert st == [snappy_amd.ERR_TRUNCATED, 0] and rcode == snappy_amd.ERR_TRUNCATED
        # a window that starts one byte late: block 1 is not resident
        rcode, st, _ = decode(codec, text, [(2 * B, 50, 0), (B, 100, 64)], 200, comp=win[1:], origin=w0 + 1)
        assert st == [0, snappy_amd.ERR_TRUNCATED]
    # blocks outside the window are never looked at: ranges there are refused, nothing is read
    rcode, st, _ = decode(codec, text, [(0, 10, 0), (3 * B, 10, 16)], 32, comp=up(comp[w0:w1]), origin=w0)
    assert st == [snappy_amd.ERR_TRUNCATED] * 2


def test_tampered_entry_is_an_index_error(codec, text):
    offs = text.offs.clone()
    offs[2] += 1                                  # block 1's chain no longer ends at the next entry
    rcode, st, _ = decode(codec, text, [(B + 10, 100, 0), (3 * B, 2000, 128)], 4096, offs=offs)
    assert st == [snappy_amd.ERR_INDEX, 0] and rcode == snappy_amd.ERR_INDEX
    # a wrong preamble is seen only by a range that decodes block 0
    s2 = Stream(codec, text.data[:N - 1].tobytes())
    s2.n, s2.data = N, text.data                  # claim one byte more than the preamble says
    rcode, st, _ = decode(codec, s2, [(B, 10, 0), (5, 10, 16)], 32)
    assert st == [0, snappy_amd.ERR_HEADER]


@pytest.mark.parametrize("chunk,n", [(17, 5000), (4096, 5 * 4096 + 123), (65536, 2 * B + 77)])
def test_streams_layout(codec, chunk, n):
    s = Stream(codec, datagen.make("T", n, 3).tobytes(), chunk=chunk, layout=snappy_amd.STREAMS)
    spans = [(0, n), (chunk - 1, chunk + 1), (chunk, 2 * chunk), (1, chunk), (chunk + 5, 3 * chunk - 1 if 3 * chunk - 1 < n else n),
             (n - 1, n), ((n - 1) // chunk * chunk, n), (0, 1), (n - chunk - 3, n)]
    ranges, oo = [], 0
    for k, (a, b) in enumerate(spans):
        oo += 1 + k
        ranges.append((a, b - a, oo))
        oo += b - a
    ranges.append((n, 1, 0))
    rcode, st, _ = decode(codec, s, ranges, oo + 9)
    assert st == [0] * len(spans) + [snappy_amd.ERR_ARG]


def sidecar(n, entries):
    return struct.pack("<QQQ", snappy_amd.IDX_MAGIC, n, len(entries)) + struct.pack(f"<{len(entries)}Q", *entries)


@pytest.mark.parametrize("name", sorted(rc.FOREIGN))
def test_foreign_streams(codec, name):
    """streams no encoder here writes: the device call gives exactly the model's
    status for every range, the host forms the slice for every one"""
    ops = rc.FOREIGN[name]
    stream = build_stream(ops)
    whole = oracle.decompress(stream)
    cases = rc.foreign_ranges(name)
    if name == "straddles":
        assert sum(c[2] == 0 for c in cases) >= 6 and sum(c[2] == snappy_amd.ERR_DEPENDENT for c in cases) >= 4
    comp = up(stream)
    n, offs = codec.index_tensor(comp)
    assert n == len(whole) == rc.FOREIGN_LEN[name]
    s = Stream.__new__(Stream)
    s.data, s.n, s.chunk, s.layout = np.frombuffer(whole, dtype=np.uint8), n, B, snappy_amd.SINGLE
    s.comp, s.offs = comp, offs.contiguous()
    ranges, oo = [], 0
    for k, (a, ln, _) in enumerate(cases):
        oo += 1 + k % 16
        ranges.append((a, ln, oo))
        oo += ln
    rcode, st, _ = decode(codec, s, ranges, oo + 3)
    model = [rm.range_status(ops, a, ln) for a, ln, _ in cases]
    assert model == [c[2] for c in cases]
    assert st == model
    side = sidecar(n, [int(x) for x in offs.cpu().numpy()])
    for a, ln, _ in cases:
        assert snappy_amd.decompress_range(stream, a, ln) == whole[a:a + ln], (name, a, ln)
        assert snappy_amd.decompress_range(stream, a, ln, index_file=side) == whole[a:a + ln], (name, a, ln)


def test_xblock_vectors_through_the_host_form(codec, golden):
    for v in golden["xblock_vectors"]:
        if "random" in v:
            r = v["random"]
            stream = build_stream(random_ops(r["seed"], r["n_out"], r["max_off"]))
        else:
            stream = build_stream(v["ops"])
        whole = snappy_amd.decompress(stream)
        n = len(whole)
        assert n == v["out_len"]
        comp = up(stream)
        side = sidecar(n, [int(x) for x in codec.index_tensor(comp)[1].cpu().numpy()])
        a0, b0 = min(B - 3, n), min(B + 40, n)
        for a, b in ((0, n), (a0, b0), (max(n, 1) - 1, n), (min(n, B), n), (n // 2, n // 2)):
            assert snappy_amd.decompress_range(stream, a, b - a, index_file=side) == whole[a:b], (v["name"], a, b)
        assert snappy_amd.decompress_range(stream, a0, b0 - a0) == whole[a0:b0], v["name"]


def test_host_forms_and_cli(codec, text, tmp_path):
    data = text.data.tobytes()
    raw, snp, out = tmp_path / "in.bin", tmp_path / "in.snp", tmp_path / "out.bin"
    raw.write_bytes(data)
    subprocess.run([CLI, "-c", "-i", str(raw), str(snp)], check=True)
    stream, side = snp.read_bytes(), (tmp_path / "in.snp.idx").read_bytes()
    assert stream == text.comp.cpu().numpy().tobytes()
    for a, ln in ((0, N), (70001, 100000), (N - 1, 1), (5, 0), (N, 0), (B, B)):
        assert snappy_amd.decompress_range(stream, a, ln) == data[a:a + ln]
        assert snappy_amd.decompress_range(stream, a, ln, index_file=side) == data[a:a + ln]
    for idx in (None, side):
        with pytest.raises(snappy_amd.SnappyError) as e:
            snappy_amd.decompress_range(stream, N - 5, 6, index_file=idx)
        assert e.value.code == snappy_amd.ERR_ARG

    a, ln = 70001, 100000                         # blocks 1 and 2
    subprocess.run([CLI, "-d", "-i", "-R", f"{a}:{ln}", str(snp), str(out)], check=True)
    assert out.read_bytes() == data[a:a + ln]
    subprocess.run([CLI, "-d", "-R", f"{a}:{ln}", str(snp), str(out)], check=True)
    assert out.read_bytes() == data[a:a + ln]
    # only the preamble and the blocks' window are used: everything else overwritten
    _, ent = snappy_amd.read_index(side)
    w0, w1 = ent[1], ent[3]
    holed = bytearray(b"\xff" * len(stream))
    holed[:3] = stream[:3]                         # (varint of 263,378: 3 bytes)
    holed[w0:w1] = stream[w0:w1]
    hs = tmp_path / "holed.snp"
    hs.write_bytes(bytes(holed))
    (tmp_path / "holed.snp.idx").write_bytes(side)
    subprocess.run([CLI, "-d", "-i", "-R", f"{a}:{ln}", str(hs), str(out)], check=True)
    assert out.read_bytes() == data[a:a + ln]
    assert snappy_amd.decompress_range(bytes(holed), a, ln, index_file=side) == data[a:a + ln]
    # -R is refused with -c, and a malformed range
    for bad in (["-c", "-R", "0:1"], ["-d", "-f", "-R", "0:1"], ["-d", "-R", "5"], ["-d", "-R", "1:2:3"], ["-d", "-R", "-1:2"]):
        assert subprocess.run([CLI] + bad + [str(snp), str(out)], capture_output=True).returncode != 0
    # a pipe cannot seek
    fifo = tmp_path / "pipe.snp"
    os.mkfifo(fifo)
    (tmp_path / "pipe.snp.idx").write_bytes(side)
    p = subprocess.Popen([CLI, "-d", "-i", "-R", "0:10", str(fifo), str(out)], stderr=subprocess.PIPE)
    try:
        with open(fifo, "wb") as w:               # (returns once the CLI has opened its end)
            w.write(stream)
    except BrokenPipeError:
        pass                                      # the CLI refused the pipe without reading it
    err = p.communicate()[1]
    assert p.returncode != 0 and b"error -9" in err, err


def test_sidecar_of_another_stream(codec, text):
    other = Stream(codec, datagen.make("T", N, 78).tobytes())       # the same length, other bytes
    shorter = Stream(codec, datagen.make("T", N - B, 77).tobytes())
    stream = text.comp.cpu().numpy().tobytes()
    for o in (other, shorter):
        with pytest.raises(snappy_amd.SnappyError) as e:
            snappy_amd.decompress_range(stream, B + 1, 100, index_file=sidecar(o.n, o.entries))
        assert e.value.code == snappy_amd.ERR_INDEX
    # an index of the right shape whose entry inside the range is off an element boundary
    ent = list(text.entries)
    ent[2] += 1
    with pytest.raises(snappy_amd.SnappyError) as e:
        snappy_amd.decompress_range(stream, B + 1, 100, index_file=sidecar(N, ent))
    assert e.value.code == snappy_amd.ERR_INDEX

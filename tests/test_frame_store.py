"""GPU: framed compress with a chunk size and stored chunks
(snappy_amd_compress_frame_device_ex, SNAPPY_AMD_FRAME_STORE; kf2_choose,
k2_emit_units_sel, kf2_store), bit for bit against the model of
frame_store_cases.py: the store rule at its threshold, the store copy at every
pair of source and destination alignments, mixed streams, both match finders,
round trips through every framed decoder, the unchanged default path, the host
forms with the CLI, and a bound side stream."""
import ctypes
import functools
import os
import subprocess

import numpy as np
import pytest
import torch

import frame_model as fm
import frame_store_cases as fs
import oracle
import snappy_amd

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "lightweight-snappy_amd", "snappy")
SENT = 0xA5
STORE, NOID = snappy_amd.FRAME_STORE, snappy_amd.FRAME_NO_IDENTIFIER
K3_WAVE_MAX = 8192


def host(t) -> bytes:
    return t.cpu().numpy().tobytes()


def dev(b) -> torch.Tensor:
    return torch.from_numpy(np.frombuffer(bytes(b), dtype=np.uint8).copy()).cuda() if len(b) else \
        torch.empty(0, dtype=torch.uint8, device="cuda")


@functools.lru_cache(maxsize=None)
def model(a: bytes, chunk: int, store: bool):
    return fs.model(a, chunk, store)


def expected(a, chunk, flags):
    stream, table, kinds = model(a, chunk, bool(flags & STORE))
    if flags & NOID:
        return stream[10:], [t - 10 for t in table], kinds
    return stream, table, kinds


def run(codec, a: bytes, chunk, flags, in_off=0, out_off=0, legacy=False):
    """The device call on a[...] at address residue in_off into a sentinel-filled buffer at
    residue out_off -> (stream, chunk table); every byte outside [0, out_len) is checked."""
    n = len(a)
    units = (n + chunk - 1) // chunk
    src = torch.full((n + 32,), 0x3C, dtype=torch.uint8, device="cuda")
    if n:
        src[in_off:in_off + n] = dev(a)
    cap = snappy_amd.max_frame_output(n, chunk)
    buf = torch.full((out_off + cap + 64,), SENT, dtype=torch.uint8, device="cuda")
    chunks = torch.full((units + 2,), -1, dtype=torch.int64, device="cuda")
    codec._bind_stream()
    got = codec.compress_frame_ptr(src.data_ptr() + in_off if n else 0, n, flags, buf.data_ptr() + out_off,
                                   chunks.data_ptr(), None if legacy else chunk)
    assert got <= cap
    b = host(buf)
    assert b[:out_off] == bytes([SENT]) * out_off, "bytes in front of the output were written"
    assert b[out_off + got:] == bytes([SENT]) * (len(b) - out_off - got), "bytes past out_len were written"
    table = chunks.cpu().tolist()
    assert table[-1] == -1, "the chunk table has an entry too many"
    return b[out_off:out_off + got], table[:-1]


def check(codec, a, chunk, flags, in_off=0, out_off=0):
    want, table, kinds = expected(a, chunk, flags)
    got, gtab = run(codec, a, chunk, flags, in_off, out_off)
    assert gtab == table, (chunk, flags, in_off, out_off)
    assert got == want, (chunk, flags, in_off, out_off)
    return kinds


# ---- 1 threshold --------------------------------------------------------------
@pytest.mark.parametrize("R", fs.PLANT_R)
def test_threshold(codec, R):
    p = fs.plants(R)
    a = p[-1] + p[0] + p[1]
    got, table = run(codec, a, R, STORE)
    assert [got[t] for t in table[:-1]] == [0, 1, 1]
    assert check(codec, a, R, STORE) == "CSS"
    assert check(codec, a, R, 0) == "CCC"
    if R == 65536:
        payload, offs = oracle.compress_streams(np.frombuffer(a, dtype=np.uint8), R)
        assert run(codec, a, R, 0)[0] == fm.frame_streams(a, payload.tobytes(), offs)


# ---- 2 the store copy at every alignment pair ---------------------------------
@pytest.mark.parametrize("ident", [True, False])
@pytest.mark.parametrize("out_off", [0, 3])
def test_store_copy_chunk_17_every_alignment_pair(codec, out_off, ident):
    # stored chunks advance the destination by 25 and the source by 17: every destination
    # residue mod 16 in one call, against every source residue over the 16 base offsets
    a = fs.noise()[:40 * 17 + 5]
    flags = STORE | (0 if ident else NOID)
    assert expected(a, 17, flags)[2] == "S" * 41
    for in_off in range(16):
        check(codec, a, 17, flags, in_off, out_off)


@pytest.mark.parametrize("chunk", [1, 64, 257, 4096])
def test_store_copy_small_chunks(codec, chunk):
    a = fs.noise()[:40 * chunk + (5 if chunk > 5 else 0)] if chunk < 4096 else fs.noise()[:5 * chunk + 5]
    assert set(expected(a, chunk, STORE)[2]) == {"S"}
    for in_off in (0, 1, 15):
        for out_off in (0, 3):
            for flags in (STORE, STORE | NOID):
                check(codec, a, chunk, flags, in_off, out_off)


@pytest.mark.parametrize("chunk", [65535, 65536])
def test_store_copy_largest_chunks(codec, chunk):
    a = fs.rand(3 * chunk)
    assert expected(a, chunk, STORE)[2] == "SSS"
    for in_off in (0, 7):
        for out_off in (0, 7):
            check(codec, a, chunk, STORE, in_off, out_off)


# ---- 3 mixed streams ------------------------------------------------------------
MIXED = [("CCCCCC", 0), ("SSSSSS", 0), ("CSCSCSC", 0), ("SSCCSSCC", 0), ("C", 0), ("S", 0)] + \
        [(p, t) for p in ("SCSC", "CSCS") for t in (1, 16, 17, 4095)]


@pytest.mark.parametrize("pattern,tail", MIXED)
def test_mixed_streams(codec, pattern, tail):
    a = fs.mixed(4096, pattern, tail)
    kinds = check(codec, a, 4096, STORE)
    # the inputs are what they are meant to be: text chunks compress, noise is stored
    # (a last chunk of at most 16 bytes is stored whatever it holds; 17 bytes of text: as the rule says)
    assert kinds[:-1] == pattern[:-1]
    if tail != 17:
        assert kinds[-1] == ("S" if 0 < tail <= 16 else pattern[-1])
    assert check(codec, a, 4096, 0) == "C" * len(pattern)


def k3_input(units: int) -> bytes:
    """64-byte chunks: zeros (compressed), noise (stored), two of three stored"""
    z, r = bytes(64), fs.rand(64 * (K3_WAVE_MAX + 1))
    return b"".join(z if u % 3 == 0 else r[64 * u:64 * u + 64] for u in range(units))


@pytest.mark.parametrize("units", [K3_WAVE_MAX, K3_WAVE_MAX + 1])
def test_mixed_stream_on_each_side_of_the_scan_kernels(codec, units):
    a = k3_input(units)
    kinds = check(codec, a, 64, STORE)
    assert len(kinds) == units and kinds[:6] == "CSSCSS"


# ---- 4 both match finders -------------------------------------------------------
@pytest.mark.parametrize("chunk", [32768, 32769, 65535])
def test_both_match_finders(codec, chunk):
    a = fs.mixed(chunk, "CSSC", 1234)
    assert check(codec, a, chunk, STORE) == "CSSC"
    assert check(codec, a, chunk, 0) == "CCCC"


# ---- 5 round trips of our own streams -------------------------------------------
STREAMS = {
    "chunk 17, noise": lambda: (fs.noise()[:40 * 17 + 5], 17),
    "chunk 1": lambda: (fs.noise()[:40], 1),
    "chunk 257": lambda: (fs.noise()[:40 * 257 + 5], 257),
    "chunk 65536, noise": lambda: (fs.rand(3 * 65536), 65536),
    "chunk 4096, SSCCSSCC": lambda: (fs.mixed(4096, "SSCCSSCC"), 4096),
    "chunk 4096, CSCSCSC": lambda: (fs.mixed(4096, "CSCSCSC"), 4096),
    "chunk 4096, short stored tail": lambda: (fs.mixed(4096, "CSCS", 17), 4096),
    "chunk 4096, short compressed tail": lambda: (fs.mixed(4096, "SCSC", 4095), 4096),
    "chunk 64, 8193 chunks": lambda: (k3_input(K3_WAVE_MAX + 1), 64),
    "chunk 32768": lambda: (fs.mixed(32768, "CSSC", 1234), 32768),
    "chunk 32769": lambda: (fs.mixed(32769, "CSSC", 1234), 32769),
    "chunk 65535": lambda: (fs.mixed(65535, "CSSC", 1234), 65535),
}


def boundary_ranges(n, chunk, units):
    """(start, length) across every chunk boundary (at most 40 of them), inside chunks, and long ones"""
    step = max(units // 40, 1)
    r = [(0, n), (n - 1, 1), (0, 1)]
    for u in range(1, units, step):
        at = u * chunk
        r.append((at - 1, 2))                              # the last byte of one chunk, the first of the next
        r.append((max(at - 5, 0), min(11, n - max(at - 5, 0))))
        if chunk > 4:
            r.append((at + 1, min(chunk - 2, n - at - 1)))  # inside chunk u
    if units > 2:
        r.append((chunk // 2, min(n - chunk // 2, 2 * chunk)))  # from the middle of chunk 0 into chunk 2
    return [(s, ln) for s, ln in r if ln > 0]


def check_ranges(codec, frame, chunks, starts, a, ranges):
    plan, at = [], 0
    for s, ln in ranges:
        plan.append((s, ln, at))
        at += ln + 3  # (outputs apart, at changing alignments)
    out = torch.full((at + 16,), SENT, dtype=torch.uint8, device="cuda")
    out, status = codec.decompress_frame_ranges_tensor(frame, 0, chunks, starts, plan, out=out)
    assert codec.last_ranges_status == 0 and not status.any()
    b = host(out)
    for s, ln, o in plan:
        assert b[o:o + ln] == a[s:s + ln], (s, ln)
        assert b[o + ln:o + ln + 3] == bytes([SENT]) * 3, (s, ln)


@pytest.mark.parametrize("name", list(STREAMS))
def test_round_trips(codec, name):
    a, chunk = STREAMS[name]()
    n = len(a)
    units = (n + chunk - 1) // chunk
    want, table, kinds = expected(a, chunk, STORE)
    frame, chunks = codec.compress_frame_tensor(dev(a), flags=STORE, chunk=chunk)
    assert host(frame) == want and chunks.cpu().tolist() == table
    # the device walk finds the table compress returned
    total, walked = codec.frame_index_tensor(frame)
    assert total == n and walked.cpu().tolist() == table
    assert host(codec.decompress_frame_tensor(frame, chunks, n)) == a
    total, starts = codec.frame_seek_tensor(frame, chunks)
    assert total == n and starts.cpu().tolist() == [min(chunk * i, n) for i in range(units + 1)]
    check_ranges(codec, frame, chunks, starts, a, boundary_ranges(n, chunk, units))
    # the strict reader of the model, and the host decoder
    assert fm.read(want, oracle.decompress) == a
    assert snappy_amd.decompress_frame(want) == a


def test_ranges_by_the_kind_of_their_edge_chunks(codec):
    a, chunk = fs.mixed(4096, "SCCSSC"), 4096
    assert expected(a, chunk, STORE)[2] == "SCCSSC"
    frame, chunks = codec.compress_frame_tensor(dev(a), flags=STORE, chunk=chunk)
    _, starts = codec.frame_seek_tensor(frame, chunks)
    check_ranges(codec, frame, chunks, starts, a, [
        (100, 3 * chunk + 50 - 100),        # both edge chunks stored (0 and 3), compressed ones between
        (chunk + 9, chunk + 500),           # both edge chunks compressed (1 and 2)
        (chunk + 9, 4 * chunk),             # compressed edges (1 and 5), stored chunks between
        (4 * chunk + 17, 1000),             # inside one stored chunk
        (3 * chunk, chunk), (4 * chunk, chunk),  # whole stored chunks
        (chunk - 5, 10), (3 * chunk - 1, 2), (5 * chunk - 100, 300),  # across S/C, C/S and S/C boundaries
    ])


# ---- 6 the default path is unchanged -----------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 65536, 65537, 300000])
@pytest.mark.parametrize("kind", ["text", "noise", "zeros"])
def test_default_path_unchanged(codec, kind, n):
    a = {"text": fs.text, "noise": fs.rand, "zeros": bytes}[kind](n)
    for flags in (0, NOID):
        assert run(codec, a, 65536, flags) == run(codec, a, 65536, flags, legacy=True)
    if n == 65537:
        payload, offs = oracle.compress_streams(np.frombuffer(a, dtype=np.uint8), 65536)
        assert run(codec, a, 65536, 0)[0] == fm.frame_streams(a, payload.tobytes(), offs)


def _refused(codec, a, flags, chunk):
    x = dev(a)
    buf = torch.full((snappy_amd.max_frame_output(len(a)) + 64,), SENT, dtype=torch.uint8, device="cuda")
    chunks = torch.full((8,), -1, dtype=torch.int64, device="cuda")
    codec._bind_stream()
    with pytest.raises(snappy_amd.SnappyError) as e:
        codec.compress_frame_ptr(x.data_ptr(), len(a), flags, buf.data_ptr(), chunks.data_ptr(), chunk)
    assert e.value.code == snappy_amd.ERR_ARG
    torch.cuda.synchronize()
    assert host(buf) == bytes([SENT]) * buf.numel() and chunks.cpu().tolist() == [-1] * 8


def test_refused_arguments_write_nothing(codec):
    a = fs.text(70000)
    _refused(codec, a, STORE, None)          # the call without a chunk size keeps refusing flag 2
    _refused(codec, a, STORE | NOID, None)
    for chunk in (0, 65537, 1 << 31):
        _refused(codec, a, 0, chunk)
        _refused(codec, a, STORE, chunk)
    _refused(codec, a, 4, 65536)
    _refused(codec, a, 4 | STORE, 4096)
    assert run(codec, a, 4096, STORE)[0] == expected(a, 4096, STORE)[0]  # the context goes on working


def test_device_bytes_and_trim_cover_the_stored_words(codec):
    codec.trim()
    base = codec.device_bytes()
    a = fs.mixed(4096, "CSCS")
    check(codec, a, 4096, STORE)
    assert codec.device_bytes() > base
    codec.trim()
    assert codec.device_bytes() == base


# ---- 7 host forms and the CLI -----------------------------------------------------
def host_input(chunk):
    return fs.mixed(chunk, "CSSCS", 100)


def file_form(a: bytes, chunk: int, flags: int, tmp_path) -> bytes:
    """snappy_compress_file_framed_ex on FILE*s of the C library"""
    libc = ctypes.CDLL(None)
    libc.fopen.restype = ctypes.c_void_p
    libc.fopen.argtypes = [ctypes.c_char_p, ctypes.c_char_p]
    libc.fclose.argtypes = [ctypes.c_void_p]
    src, dst = str(tmp_path / "in"), str(tmp_path / "out")
    open(src, "wb").write(a)
    fi, fo = libc.fopen(src.encode(), b"rb"), libc.fopen(dst.encode(), b"wb")
    assert fi and fo
    try:
        rc = snappy_amd.lib().snappy_compress_file_framed_ex(fi, len(a), chunk, flags, fo)
    finally:
        libc.fclose(fi)
        libc.fclose(fo)
    assert rc == 0
    return open(dst, "rb").read()


@pytest.mark.parametrize("chunk", [24576, 65536])
def test_host_forms_equal_the_device_call(codec, chunk, tmp_path):
    a = host_input(chunk)
    want = run(codec, a, chunk, STORE)[0]
    assert want == expected(a, chunk, STORE)[0]
    assert snappy_amd.compress_frame(a, chunk=chunk, store=True) == want
    assert file_form(a, chunk, STORE, tmp_path) == want
    assert snappy_amd.compress_frame(a, chunk=chunk) == expected(a, chunk, 0)[0]
    # the host forms place the identifier themselves
    out = ctypes.create_string_buffer(snappy_amd.max_frame_output(len(a), chunk))
    got = ctypes.c_size_t(0)
    for flags in (NOID, NOID | STORE, 4):
        assert snappy_amd.lib().snappy_compress_frame_buffer_ex(a, len(a), chunk, flags, out, len(out),
                                                                ctypes.byref(got)) == snappy_amd.ERR_ARG


def test_host_forms_cut_pieces_at_chunk_multiples(codec, monkeypatch, tmp_path):
    # a 64 KiB piece size with chunks of 24,576: pieces of 49,152 bytes (two chunks).  A piece of
    # 65,536 would end a chunk after 16,384 bytes and give other chunks than the whole input's
    chunk = 24576
    a = host_input(chunk)
    want = run(codec, a, chunk, STORE)[0]
    monkeypatch.setenv("SNAPPY_AMD_FRAME_PIECE_KB", "64")
    assert snappy_amd.compress_frame(a, chunk=chunk, store=True) == want
    assert file_form(a, chunk, STORE, tmp_path) == want
    assert snappy_amd.compress_frame(a, chunk=chunk) == expected(a, chunk, 0)[0]


def test_cli_chunk_size_and_store(tmp_path):
    a = fs.mixed(4096, "CSSCSC", 1000)
    want = expected(a, 4096, STORE)[0]
    src, snp, dec, part = (str(tmp_path / x) for x in ("in", "in.sz", "in.dec", "in.part"))
    open(src, "wb").write(a)
    subprocess.run([EXE, "-c", "-f", "-s", "-k", "4096", src, snp], check=True, capture_output=True)
    assert open(snp, "rb").read() == want
    subprocess.run([EXE, "-d", "-f", snp, dec], check=True, capture_output=True)
    assert open(dec, "rb").read() == a
    subprocess.run([EXE, "-d", "-f", "-R", "4000:9000", snp, part], check=True, capture_output=True)
    assert open(part, "rb").read() == a[4000:13000]
    # each option alone
    subprocess.run([EXE, "-c", "-f", "-k", "4096", src, snp], check=True, capture_output=True)
    assert open(snp, "rb").read() == expected(a, 4096, 0)[0]
    subprocess.run([EXE, "-c", "-f", "-s", src, snp], check=True, capture_output=True)
    assert open(snp, "rb").read() == expected(a, 65536, STORE)[0]


def test_cli_chunk_size_and_store_go_with_c_f_only(tmp_path):
    src, snp = str(tmp_path / "in"), str(tmp_path / "out")
    open(src, "wb").write(b"x" * 100)
    for flags in (["-c", "-s"], ["-c", "-k", "4096"], ["-d", "-f", "-s"], ["-d", "-f", "-k", "4096"], ["-f", "-s"],
                  ["-b", "-s"], ["-c", "-i", "-s"], ["-c", "-F", "hadoop", "-k", "4096"],
                  ["-c", "-f", "-k", "0"], ["-c", "-f", "-k", "65537"], ["-c", "-f", "-k", "4k"]):
        r = subprocess.run([EXE] + flags + [src, snp], capture_output=True)
        assert r.returncode == 1 and r.stderr.startswith(b"snappy [-c|-d|-b]"), flags


# ---- 8 stream order -----------------------------------------------------------------
SPIN = 5_000_000  # about 2 ms on the MI355X (test_stream_order.py)


def test_on_a_bound_side_stream(codec):
    """The queued form (out_len NULL) on a non-blocking side stream that is still busy, the input
    written on that stream just before the call: every launch of the call (kf2_choose,
    k2_emit_units_sel, the CRC, kf2_store, the headers) must be ordered behind that copy, or it
    reads the decoy -- the same chunks in another order, whose stream differs."""
    chunk = 4096
    a = fs.mixed(chunk, "CSSCSC", 777)
    decoy = fs.mixed(chunk, "SCCSCS", 777)
    want, table, _ = expected(a, chunk, STORE)
    assert expected(decoy, chunk, STORE)[0] != want
    n, units = len(a), len(table) - 1
    src, alt = dev(a), dev(decoy)
    x = torch.empty_like(src)
    cap = snappy_amd.max_frame_output(n, chunk)
    buf = torch.full((cap + 64,), SENT, dtype=torch.uint8, device="cuda")
    chunks = torch.full((units + 1,), -1, dtype=torch.int64, device="cuda")

    def call():
        codec._bind_stream()
        rc = snappy_amd.lib().snappy_amd_compress_frame_device_ex(
            codec._h, ctypes.c_void_p(x.data_ptr()), n, chunk, STORE, ctypes.c_void_p(buf.data_ptr()),
            ctypes.c_void_p(chunks.data_ptr()), None)
        assert rc == 0

    # once on the default stream: the context's scratch has its size, so the call below frees nothing
    x.copy_(src)
    call()
    torch.cuda.synchronize()
    assert host(buf[:len(want)]) == want
    buf.fill_(SENT)
    chunks.fill_(-1)
    x.copy_(alt)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    try:
        with torch.cuda.stream(side):
            torch.cuda._sleep(SPIN)
            x.copy_(src, non_blocking=True)
            before = not side.query()
            call()
            after = not side.query()
        side.synchronize()
    finally:
        codec.set_stream(0)
    assert before, "the side stream was idle when the call was made: the test shows nothing"
    assert after, "the queued form returned only after the stream had drained"
    assert chunks.cpu().tolist() == table
    b = host(buf)
    assert b[:len(want)] == want and b[len(want):] == bytes([SENT]) * (len(b) - len(want))

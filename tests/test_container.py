"""GPU: the Hadoop SnappyCodec and snappy-java SnappyOutputStream containers --
compress (bit for bit the model's wrapping of the oracle's stream of each
piece), the walks (KC1, the host walk, the model), decode of this library's and
of foreign streams, the error table and the host / CLI forms.  Conformance rests
on the model in tests/container_model.py, pinned to hand-written vectors by
test_container_model.py."""
import ctypes
import functools
import os
import subprocess
import tempfile

import numpy as np
import pytest
import torch

import container_cases as cc
import container_model as cm
import datagen
import oracle
import snappy_amd
from golden_inputs import build_stream

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "lightweight-snappy_amd", "snappy")
FORMATS = [cm.HADOOP, cm.XERIAL]
NAMES = {cm.HADOOP: "hadoop", cm.XERIAL: "xerial"}
DEFAULT = {cm.HADOOP: 131072, cm.XERIAL: 32768}
SENT = 0xA5


def dev(b) -> torch.Tensor:
    return torch.from_numpy(np.frombuffer(bytes(b), dtype=np.uint8).copy()).cuda() if len(b) else \
        torch.empty(0, dtype=torch.uint8, device="cuda")


def host(t) -> bytes:
    return t.cpu().numpy().tobytes()


def pairs(t):
    v = t.cpu().tolist()
    return list(zip(v[0::2], v[1::2]))


def flat(p):
    return torch.tensor([x for q in p for x in q], dtype=torch.int64, device="cuda")


def code(fn, *a, **k):
    try:
        return 0, fn(*a, **k)
    except snappy_amd.SnappyError as e:
        return e.code, None


# ---- compress -----------------------------------------------------------------
BLOCKS = [4096, 65536, 65537, 131072, 0]


def sizes(block):
    return [0, 1, block - 1, block, block + 1, 5 * block + 17]


@functools.lru_cache(maxsize=None)
def source(kind):
    return datagen.make(kind, 5 * 131072 + 17, 4321).tobytes()


@functools.lru_cache(maxsize=None)
def piece_stream(kind, at, n):
    """the oracle's stream of source(kind)[at:at + n] (what snappy_compress() writes for it)"""
    return oracle.compress(source(kind)[at:at + n])


@functools.lru_cache(maxsize=None)
def case(kind, n, block, fmt):
    """input bytes and the model's wrapping of the oracle's streams of its pieces"""
    a = source(kind)[:n]
    b = block or DEFAULT[fmt]
    cut = [(at, min(b, n - at)) for at in range(0, n, b)]
    want = cm.wrap([a[at:at + m] for at, m in cut], [piece_stream(kind, at, m) for at, m in cut], fmt)
    return a, want


def compress_into(codec, x, fmt, block, align, cap, flags=0):
    """compress_container_device with d_out `align` bytes into a sentinel-filled buffer
    -> (container bytes, payload pairs, output pairs); the bytes around it checked"""
    buf = torch.full((align + cap + 64,), SENT, dtype=torch.uint8, device="cuda")
    out, comp, outp = codec.compress_container_tensor(x, fmt, block, flags=flags, out=buf[align:align + cap])
    got = out.numel()
    b = host(buf)
    assert b[:align] == bytes([SENT]) * align, "bytes in front of d_out were written"
    assert b[align + got:] == bytes([SENT]) * (len(b) - align - got), "bytes from out_len on were written"
    return b[align:align + got], pairs(comp), pairs(outp)


@pytest.mark.parametrize("block", BLOCKS)
@pytest.mark.parametrize("kind", ["T", "R"])
@pytest.mark.parametrize("fmt", FORMATS)
def test_compress_bit_for_bit_at_every_alignment(codec, fmt, kind, block):
    for n in sizes(block or DEFAULT[fmt]):
        a, want = case(kind, n, block, fmt)
        st, comp_want, outp_want, total = cm.walk(want, fmt)
        assert st == cm.OK and total == n
        x = dev(a)
        cap = snappy_amd.max_container_output(n, block, fmt)
        assert len(want) <= cap
        for align in range(8):
            got, comp, outp = compress_into(codec, x, fmt, block, align, cap)
            assert got == want, (n, align)
            assert comp == comp_want and outp == outp_want, (n, align)


@pytest.mark.parametrize("fmt", FORMATS)
def test_compress_block_of_one_byte(codec, fmt):
    a = b"abc"
    want = cm.wrap([b"a", b"b", b"c"], [oracle.compress(x) for x in (b"a", b"b", b"c")], fmt)
    got, comp, outp = compress_into(codec, dev(a), fmt, 1, 3, snappy_amd.max_container_output(3, 1, fmt))
    assert got == want
    assert (cm.OK, comp, outp, 3) == cm.walk(want, fmt)


@pytest.mark.parametrize("fmt", FORMATS)
def test_no_header_pieces_concatenate_to_the_one_call_output(codec, fmt):
    block, n = 4096, 5 * 4096 + 17
    a, want = case("T", n, block, fmt)
    cut = 2 * block
    cap = snappy_amd.max_container_output(n, block, fmt)
    first, _, _ = compress_into(codec, dev(a[:cut]), fmt, block, 0, cap)
    rest, comp, outp = compress_into(codec, dev(a[cut:]), fmt, block, 5, cap, flags=snappy_amd.CONTAINER_NO_HEADER)
    assert first + rest == want
    # the continuation's tables count from its own first byte
    st, comp_want, outp_want, _ = cm.walk(want, fmt)
    k = len(comp_want) - len(comp)
    assert k == 2
    assert comp == [(o - len(first), c) for o, c in comp_want[k:]]
    assert outp == [(o - cut, m) for o, m in outp_want[k:]]
    if fmt == cm.HADOOP:  # no header to drop: the flag changes nothing
        again, _, _ = compress_into(codec, dev(a), fmt, block, 0, cap, flags=snappy_amd.CONTAINER_NO_HEADER)
        assert again == want


def raw_compress(codec, x, n, block, fmt, flags, out, out_cap, comp, outp, chunks_cap):
    nch, got = ctypes.c_size_t(0), ctypes.c_size_t(0)
    codec._bind_stream()
    rc = snappy_amd.lib().snappy_amd_compress_container_device(
        codec._h, ctypes.c_void_p(x.data_ptr()), n, block, fmt, flags, ctypes.c_void_p(out.data_ptr()), out_cap,
        ctypes.c_void_p(comp.data_ptr() if comp is not None else 0),
        ctypes.c_void_p(outp.data_ptr() if outp is not None else 0), chunks_cap, ctypes.byref(nch), ctypes.byref(got))
    return rc, nch.value, got.value


@pytest.mark.parametrize("fmt", FORMATS)
def test_compress_refusals_write_nothing(codec, fmt):
    block, n = 4096, 5 * 4096 + 17
    a, want = case("T", n, block, fmt)
    x = dev(a)
    cap = snappy_amd.max_container_output(n, block, fmt)
    out = torch.full((cap + 64,), SENT, dtype=torch.uint8, device="cuda")
    comp = torch.full((12,), -1, dtype=torch.int64, device="cuda")
    outp = torch.full((12,), -1, dtype=torch.int64, device="cuda")
    untouched = lambda: host(out) == bytes([SENT]) * (cap + 64) and comp.cpu().tolist() == [-1] * 12 and \
        outp.cpu().tolist() == [-1] * 12
    assert raw_compress(codec, x, n, block, fmt, 0, out, cap - 1, comp, outp, 6)[0] == snappy_amd.ERR_CAPACITY
    assert untouched()
    assert raw_compress(codec, x, n, block, fmt, 0, out, cap, comp, outp, 5)[0] == snappy_amd.ERR_CAPACITY
    assert untouched()
    assert raw_compress(codec, x, n, block, 2, 0, out, cap, comp, outp, 6)[0] == snappy_amd.ERR_ARG
    assert raw_compress(codec, x, n, block, fmt, 2, out, cap, comp, outp, 6)[0] == snappy_amd.ERR_ARG
    assert raw_compress(codec, x, n, (1 << 30) + 1, fmt, 0, out, cap, comp, outp, 6)[0] == snappy_amd.ERR_ARG
    assert untouched()
    # and with room, with and without tables
    assert raw_compress(codec, x, n, block, fmt, 0, out, cap, comp, outp, 6) == (0, 6, len(want))
    assert host(out[:len(want)]) == want
    out.fill_(SENT)
    assert raw_compress(codec, x, n, block, fmt, 0, out, cap, None, None, 0) == (0, 6, len(want))
    assert host(out[:len(want)]) == want


# ---- round trip and walk --------------------------------------------------------
ROUND = [("T", 5 * 131072 + 17, 0), ("R", 5 * 65537 + 17, 65537), ("T", 5 * 4096 + 17, 4096), ("R", 1, 0), ("T", 0, 0)]


@pytest.mark.parametrize("kind,n,block", ROUND)
@pytest.mark.parametrize("fmt", FORMATS)
def test_round_trip_and_walks_agree(codec, fmt, kind, n, block):
    a, want = case(kind, n, block, fmt)
    st, comp_want, outp_want, total = cm.walk(want, fmt)
    assert st == cm.OK
    # garbage behind clen: a second header, lengths, a chunk -- none of it may be read as the stream's
    garbage = cm.header() + cm.be32(7) + cc.HELLO + b"\xff" * 32
    cont = dev(want + garbage)
    clen = len(want)
    total_d, comp, outp = codec.container_index_tensor(cont, fmt, clen=clen)
    assert total_d == n == snappy_amd.container_uncompressed_length(want, fmt)
    assert pairs(comp) == comp_want and pairs(outp) == outp_want
    out = torch.full((n + 64,), SENT, dtype=torch.uint8, device="cuda")
    back = codec.decompress_container_tensor(cont, fmt, comp, outp, cap=n, out=out, clen=clen)
    assert host(back) == a and host(out[n:]) == bytes([SENT]) * 64
    out.fill_(SENT)
    back = codec.decompress_container_tensor(cont, fmt, cap=n, out=out, clen=clen)  # walks itself
    assert host(back) == a and host(out[n:]) == bytes([SENT]) * 64
    # the same container at an odd address
    odd = dev(b"\x00" * 3 + want + garbage)[3:]
    assert host(codec.decompress_container_tensor(odd, fmt, cap=n, clen=clen)) == a
    # host buffer forms
    assert snappy_amd.compress_container(a, fmt, block) == want
    assert snappy_amd.decompress_container(want, fmt) == a
    assert snappy_amd.decompress_container(want, NAMES[fmt]) == a


# ---- foreign streams ---------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def xblock(name):
    import json
    with open(os.path.join(ROOT, "tests", "golden", "golden.json")) as f:
        v = {x["name"]: x for x in json.load(f)["xblock_vectors"]}[name]
    s = build_stream(v["ops"])
    raw = oracle.decompress(s)
    assert len(raw) == v["out_len"]
    return s, raw


XBLOCK = ["xblock_copy2", "straddle_copy_overlap", "straddle_literal_tail", "literal_spans_3_blocks", "xblock_copy4_64k"]


def _xblock_hadoop():
    v = [xblock(n) for n in XBLOCK]
    small = oracle.compress(b"between")
    # one block holds the first two (with an ordinary chunk between them), one each the others
    s = cm.hadoop_block(len(v[0][1]) + 7 + len(v[1][1]), [v[0][0], small, v[1][0]])
    raw = v[0][1] + b"between" + v[1][1]
    for stream, r in v[2:]:
        s += cm.hadoop_block(len(r), [stream])
        raw += r
    return cm.HADOOP, s, raw


def _xblock_xerial():
    v = [xblock(n) for n in XBLOCK]
    return cm.XERIAL, cm.header() + b"".join(cm.chunk(s) for s, _ in v), b"".join(r for _, r in v)


def _unequal_compressed(fmt):
    a = source("T")
    p = [a[:1], a[1:65538], a[65538:365538]]
    streams = [oracle.compress(x) for x in p]
    if fmt == cm.HADOOP:
        return fmt, cm.hadoop_block(365538, streams), b"".join(p)
    return fmt, cm.header() + b"".join(cm.chunk(s) for s in streams), b"".join(p)


GPU_FOREIGN = dict(cc.FOREIGN)
GPU_FOREIGN.update({
    "hadoop: chunks whose elements straddle and copy across 65,536": _xblock_hadoop,
    "xerial: chunks whose elements straddle and copy across 65,536": _xblock_xerial,
    "hadoop: a block of three compressed chunks (1; 65,537; 300,000)": lambda: _unequal_compressed(cm.HADOOP),
    "xerial: three compressed chunks (1; 65,537; 300,000)": lambda: _unequal_compressed(cm.XERIAL),
})


@pytest.mark.parametrize("name", list(GPU_FOREIGN))
def test_decode_foreign_stream(codec, name):
    fmt, stream, want = GPU_FOREIGN[name]()
    st, comp_want, outp_want, total = cm.walk(stream, fmt)
    assert st == cm.OK and total == len(want) <= 5 * 131072 + 17
    assert cm.unwrap(stream, fmt, oracle.decompress) == want  # the model reads its own stream
    # host walk + buffer decode
    assert snappy_amd.container_uncompressed_length(stream, fmt) == len(want)
    assert snappy_amd.decompress_container(stream, fmt) == want
    # device walk == model, then the device decode with these tables and without
    cont = dev(stream)
    n, comp, outp = codec.container_index_tensor(cont, fmt)
    assert n == len(want) and pairs(comp) == comp_want and pairs(outp) == outp_want
    assert host(codec.decompress_container_tensor(cont, fmt, comp, outp, cap=n)) == want
    assert host(codec.decompress_container_tensor(cont, fmt, cap=n)) == want
    # the tables go straight to the long-record call
    out = torch.empty(max(n, 1), dtype=torch.uint8, device="cuda")
    codec.decompress_long_records_tensor(cont, comp.view(-1, 2), out, outp.view(-1, 2), check=True)
    assert host(out[:n]) == want


# ---- the error table ---------------------------------------------------------------
def device_walk(codec, stream, fmt):
    rc, res = code(codec.container_index_tensor, dev(stream), fmt)
    return (rc, None) if rc else (0, (res[0], pairs(res[1]), pairs(res[2])))


def host_walk(stream, fmt):
    rc, n = code(snappy_amd.container_uncompressed_length, stream, fmt)
    return rc, n


@pytest.mark.parametrize("fmt", FORMATS)
def test_every_prefix_of_a_three_chunk_container(codec, fmt):
    s = cc.abc_hadoop() if fmt == cm.HADOOP else cc.abc_xerial()
    for i in range(len(s) + 1):
        st, comp, outp, n = cm.walk(s[:i], fmt)
        rc, res = device_walk(codec, s[:i], fmt)
        assert rc == st, (i, rc, st)
        if st == cm.OK:
            assert res == (n, comp, outp), i
        assert host_walk(s[:i], fmt) == (st, n if st == cm.OK else None), i
        # the decoders report the walk's failure (or decode the whole prefix)
        rc, out = code(codec.decompress_container_tensor, dev(s[:i]), fmt, cap=8)
        assert rc == st and (st != cm.OK or host(out) == b"abc"[:n]), i
        rc, out = code(snappy_amd.decompress_container, s[:i], fmt, 8)
        assert rc == st and (st != cm.OK or out == b"abc"[:n]), i


@pytest.mark.parametrize("name", list(cc.walk_error_cases()))
def test_one_case_per_line_of_the_walk_rule(codec, name):
    fmt, stream, want = cc.walk_error_cases()[name]
    assert cm.walk(stream, fmt)[0] == want
    assert device_walk(codec, stream, fmt)[0] == want
    assert host_walk(stream, fmt)[0] == want
    assert decode_with_sentinel(codec, stream, fmt, 64)[0] == want
    assert code(snappy_amd.decompress_container, stream, fmt, 64)[0] == want
    # the context (and the pooled host context) go on working
    good = cc.HELLO_HADOOP if fmt == cm.HADOOP else cc.HELLO_XERIAL
    assert decode_with_sentinel(codec, good, fmt, 5) == (0, b"hello")
    assert snappy_amd.decompress_container(good, fmt) == b"hello"


def decode_with_sentinel(codec, stream, fmt, cap, tables=False):
    """decode through the device API into cap bytes between two sentinel runs;
    returns (status, output bytes), the sentinels checked"""
    cont = dev(stream)
    buf = torch.full((256 + cap + 256,), SENT, dtype=torch.uint8, device="cuda")
    comp = outp = None
    if tables:
        _, comp, outp = codec.container_index_tensor(cont, fmt)
    rc, got = code(codec.decompress_container_tensor, cont, fmt, comp, outp, cap=cap, out=buf[256:256 + cap])
    b = host(buf)
    assert b[:256] == bytes([SENT]) * 256, "bytes in front of d_out were written"
    assert b[256 + cap:] == bytes([SENT]) * 256, "bytes past cap were written"
    return rc, (host(got) if rc == 0 else None)


def wrapn(payloads, lens, fmt):
    if fmt == cm.HADOOP:
        return cm.hadoop_block(sum(lens), payloads)
    return cm.header() + b"".join(cm.chunk(p) for p in payloads)


@pytest.mark.parametrize("tables", [False, True])
@pytest.mark.parametrize("fmt", FORMATS)
def test_precedence_and_element_errors(codec, fmt, tables):
    p = [cc.content(200, 21), cc.content(200, 22), cc.content(200, 23)]
    good = [cc.stored(x) for x in p]
    cut_literal = cm.varint(200) + bytes([60 << 2, 199])           # a literal with no bytes behind it: TRUNCATED
    far_copy = cm.varint(200) + bytes([3 << 2]) + b"abcd" + bytes([0x01, 5])  # copies from before its chunk: OFFSET
    cap = 600
    ok = wrapn(good, [200] * 3, fmt)
    assert decode_with_sentinel(codec, ok, fmt, cap, tables) == (0, b"".join(p))
    # among element errors the first failing chunk wins
    s = wrapn([good[0], cut_literal, far_copy], [200] * 3, fmt)
    assert decode_with_sentinel(codec, s, fmt, cap, tables)[0] == snappy_amd.ERR_TRUNCATED
    s = wrapn([good[0], far_copy, cut_literal], [200] * 3, fmt)
    assert decode_with_sentinel(codec, s, fmt, cap, tables)[0] == snappy_amd.ERR_OFFSET
    assert code(snappy_amd.decompress_container, s, fmt, cap)[0] == snappy_amd.ERR_OFFSET
    # ERR_CAPACITY wins over element errors, one byte short
    assert decode_with_sentinel(codec, s, fmt, cap - 1, tables)[0] == snappy_amd.ERR_CAPACITY
    assert code(snappy_amd.decompress_container, s, fmt, cap - 1)[0] == snappy_amd.ERR_CAPACITY
    assert decode_with_sentinel(codec, ok, fmt, cap - 1, tables)[0] == snappy_amd.ERR_CAPACITY
    if not tables:
        # a walk error in chunk 2 wins over an element error in chunk 0 (and over the capacity)
        bad_walk = wrapn([cut_literal, good[1]], [200] * 3, fmt) + cm.be32(0)
        assert cm.walk(bad_walk, fmt)[0] == cm.ERR_HEADER
        assert decode_with_sentinel(codec, bad_walk, fmt, cap)[0] == snappy_amd.ERR_HEADER
        assert decode_with_sentinel(codec, bad_walk, fmt, 10)[0] == snappy_amd.ERR_HEADER
        assert code(snappy_amd.decompress_container, bad_walk, fmt, cap)[0] == snappy_amd.ERR_HEADER
    else:
        # a preamble that is not the table's length (changed between the walk and the decode)
        cont = dev(ok)
        n, comp, outp = codec.container_index_tensor(cont, fmt)
        at = comp.cpu().tolist()[2]
        cont[at] = 199
        rc, _ = code(codec.decompress_container_tensor, cont, fmt, comp, outp, cap=cap)
        assert rc == snappy_amd.ERR_HEADER
        # a caller's table that leaves the container
        comp2 = comp.clone()
        comp2[5] = len(ok)
        rc, _ = code(codec.decompress_container_tensor, dev(ok), fmt, comp2, outp, cap=cap)
        assert rc == snappy_amd.ERR_TRUNCATED


def test_index_capacity(codec):
    fmt, stream, want = cc.FOREIGN["hadoop: chunks of no bytes inside a block"]()
    cont = dev(stream)
    n, comp, outp = codec.container_index_tensor(cont, fmt, max_chunks=4)
    assert n == 30 and comp.numel() == 8
    rc, _ = code(codec.container_index_tensor, cont, fmt, max_chunks=3)
    assert rc == snappy_amd.ERR_CAPACITY


# ---- host and CLI ---------------------------------------------------------------------
def cli_round_trip(a, want, fmt, env=None):
    with tempfile.TemporaryDirectory() as d:
        src, snp, dec = (os.path.join(d, x) for x in ("in", "in.snappy", "in.dec"))
        with open(src, "wb") as f:
            f.write(a)
        subprocess.run([EXE, "-c", "-F", NAMES[fmt], src, snp], check=True, capture_output=True, env=env)
        with open(snp, "rb") as f:
            assert f.read() == want
        subprocess.run([EXE, "-d", "-F", NAMES[fmt], snp, dec], check=True, capture_output=True, env=env)
        with open(dec, "rb") as f:
            assert f.read() == a


def cli_decode(stream, fmt, env=None):
    with tempfile.TemporaryDirectory() as d:
        snp, dec = os.path.join(d, "in.snappy"), os.path.join(d, "in.dec")
        with open(snp, "wb") as f:
            f.write(stream)
        r = subprocess.run([EXE, "-d", "-F", NAMES[fmt], snp, dec], capture_output=True, env=env)
        with open(dec, "rb") as f:
            return r.returncode, f.read()


@pytest.mark.parametrize("n", [0, 1, 5 * 131072 + 17])
@pytest.mark.parametrize("fmt", FORMATS)
def test_cli_round_trip(fmt, n):
    a, want = case("T", n, 0, fmt)
    cli_round_trip(a, want, fmt)


def test_cli_container_goes_with_c_and_d_only(tmp_path):
    src, snp = str(tmp_path / "in"), str(tmp_path / "out")
    with open(src, "wb") as f:
        f.write(b"x")
    for flags in (["-F", "hadoop", "-f", "-c"], ["-F", "xerial", "-b"], ["-F", "hadoop", "-c", "-i"],
                  ["-F", "xerial", "-d", "-i"], ["-F", "lz4", "-c"]):
        r = subprocess.run([EXE] + flags + [src, snp], capture_output=True)
        assert r.returncode == 1 and b"snappy [-c|-d|-b]" in r.stderr and b"-F hadoop|xerial" in r.stderr


# The buffer and FILE* forms take 64 MiB at a time; SNAPPY_AMD_CONTAINER_PIECE_KB
# makes the pieces small enough for a 320 KiB input to cross them.
@pytest.mark.parametrize("piece_kb", [48, 128])
@pytest.mark.parametrize("fmt", FORMATS)
def test_pieces_buffer_and_file_forms(monkeypatch, fmt, piece_kb):
    n = 320 << 10
    env = dict(os.environ, SNAPPY_AMD_CONTAINER_PIECE_KB=str(piece_kb))
    monkeypatch.setenv("SNAPPY_AMD_CONTAINER_PIECE_KB", str(piece_kb))
    for kind in "TR":  # random: every chunk of the default Hadoop block is larger than a read
        a, want = case(kind, n, 0, fmt)
        assert snappy_amd.compress_container(a, fmt) == want
        assert snappy_amd.decompress_container(want, fmt) == a
        cli_round_trip(a, want, fmt, env)
        a, want = case(kind, n, 4096, fmt)
        assert snappy_amd.compress_container(a, fmt, 4096) == want
        assert snappy_amd.decompress_container(want, fmt) == a
        assert cli_decode(want, fmt, env) == (0, a)


def test_pieces_cut_inside_a_multi_chunk_hadoop_block(monkeypatch):
    fmt, stream, raw = _unequal_compressed(cm.HADOOP)  # one block, chunks of 1; 65,537; 300,000
    for piece_kb in (16, 48, 128):
        env = dict(os.environ, SNAPPY_AMD_CONTAINER_PIECE_KB=str(piece_kb))
        assert cli_decode(stream, fmt, env) == (0, raw), piece_kb
        assert cli_decode(stream[:-1], fmt, env)[0] == 1  # a cut stream is reported
        monkeypatch.setenv("SNAPPY_AMD_CONTAINER_PIECE_KB", str(piece_kb))
        assert snappy_amd.decompress_container(stream, fmt) == raw
    # snappy-java: reads that end inside a chunk, and one that ends inside a repeated header
    fmt, stream, raw = _unequal_compressed(cm.XERIAL)
    assert cli_decode(stream, fmt, dict(os.environ, SNAPPY_AMD_CONTAINER_PIECE_KB="16")) == (0, raw)
    fmt, stream, raw = GPU_FOREIGN["xerial: the header again mid-stream and at the end"]()
    pad = 1024 - 93 - 8  # the second header starts 8 bytes in front of the first read's end
    stream = cm.header() + cm.chunk(cc.stored(bytes(pad - 16 - 4 - 5))) + stream
    assert cm.walk(stream, fmt)[0] == cm.OK and stream[pad + 93:pad + 97] == cm.MAGIC[:4]
    assert cli_decode(stream, fmt, dict(os.environ, SNAPPY_AMD_CONTAINER_PIECE_KB="1")) == \
        (0, bytes(pad - 16 - 4 - 5) + raw)


def test_device_bytes_and_trim_cover_container_scratch(codec):
    codec.trim()
    base = codec.device_bytes()
    a, want = case("T", 5 * 4096 + 17, 4096, cm.XERIAL)
    out, comp, outp = codec.compress_container_tensor(dev(a), cm.XERIAL, 4096)
    assert host(out) == want and codec.device_bytes() > base
    codec.trim()
    assert codec.device_bytes() == base

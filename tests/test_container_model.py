"""CPU: the container model (tests/container_model.py) pinned to vectors written
by hand -- the two `hello` streams of DESIGN.md 7.5, the foreign streams of
container_cases.py with their tables worked out on paper, one case per line of
the walk rule -- and the host walk of the library (no kernel) held against it."""
import pytest

import container_cases as cc
import container_model as cm
import snappy_amd


def test_hello_vectors_wrap_and_walk():
    assert cm.wrap([b"hello"], [cc.HELLO], cm.HADOOP) == cc.HELLO_HADOOP
    assert cm.wrap([b"hello"], [cc.HELLO], cm.XERIAL) == cc.HELLO_XERIAL
    assert cm.wrap([b"hello"], [cc.HELLO], cm.XERIAL, with_header=False) == cc.HELLO_XERIAL[16:]
    assert cm.walk(cc.HELLO_HADOOP, cm.HADOOP) == (cm.OK, [(8, 7)], [(0, 5)], 5)
    assert cm.walk(cc.HELLO_XERIAL, cm.XERIAL) == (cm.OK, [(20, 7)], [(0, 5)], 5)
    assert cm.wrap([], [], cm.HADOOP) == b""
    assert cm.wrap([], [], cm.XERIAL) == bytes.fromhex("82534e41505059000000000100000001")
    assert cm.walk(b"", cm.HADOOP) == (cm.OK, [], [], 0)
    assert cm.walk(bytes(4), cm.HADOOP) == (cm.OK, [], [], 0)
    assert cm.walk(cm.header(), cm.XERIAL) == (cm.OK, [], [], 0)
    assert cc.stored(b"hello") == bytes.fromhex("05 10 68 65 6c 6c 6f")


def test_hello_vectors_unwrap():
    def only_hello(s):
        assert s == cc.HELLO
        return b"hello"
    assert cm.unwrap(cc.HELLO_HADOOP, cm.HADOOP, only_hello) == b"hello"
    assert cm.unwrap(cc.HELLO_XERIAL + cc.HELLO_XERIAL, cm.XERIAL, only_hello) == b"hellohello"
    with pytest.raises(ValueError):
        cm.unwrap(cc.HELLO_HADOOP, cm.XERIAL, only_hello)


def literal_reader(s: bytes) -> bytes:
    """Decodes the literal-only streams of container_cases.stored."""
    n, shift, p = 0, 0, 0
    while True:
        b = s[p]
        p += 1
        n |= (b & 0x7F) << shift
        shift += 7
        if not b & 0x80:
            break
    out = bytearray()
    while p < len(s):
        k = s[p] >> 2
        assert s[p] & 3 == 0
        p += 1
        if k >= 60:
            extra = k - 59
            k = int.from_bytes(s[p:p + extra], "little")
            p += extra
        out += s[p:p + k + 1]
        p += k + 1
    assert len(out) == n
    return bytes(out)


@pytest.mark.parametrize("name", list(cc.FOREIGN))
def test_foreign_streams_have_the_tables_worked_out_by_hand(name):
    fmt, stream, raw = cc.FOREIGN[name]()
    comp, outp = cc.FOREIGN_TABLES[name]
    assert cm.walk(stream, fmt) == (cm.OK, comp, outp, len(raw))
    assert cm.unwrap(stream, fmt, literal_reader) == raw


@pytest.mark.parametrize("name", list(cc.walk_error_cases()))
def test_one_case_per_line_of_the_walk_rule(name):
    fmt, stream, status = cc.walk_error_cases()[name]
    assert cm.walk(stream, fmt)[0] == status


def test_prefixes_of_the_three_chunk_containers():
    T, H, K = cm.ERR_TRUNCATED, cm.ERR_HEADER, cm.OK
    # hadoop: 0000 0002 | 0000 0003 01 00 61 | 0000 0003 01 00 62 || 0000 0001 | 0000 0003 01 00 63
    a = cc.abc_hadoop()
    assert len(a) == 29
    want = [K] + [T] * 17 + [K] + [T] * 10 + [K]  # whole at 0, after the first block (18), at the end (29)
    assert [cm.walk(a[:i], cm.HADOOP)[0] for i in range(30)] == want
    assert cm.walk(a, cm.HADOOP) == (K, [(8, 3), (15, 3), (26, 3)], [(0, 1), (1, 1), (2, 1)], 3)
    # xerial: 16 bytes of header | 0000 0003 01 00 61 | ... 62 | ... 63
    x = cc.abc_xerial()
    assert len(x) == 37
    want = [H] + [T] * 15 + [K] + [T] * 6 + [K] + [T] * 6 + [K] + [T] * 6 + [K]
    assert [cm.walk(x[:i], cm.XERIAL)[0] for i in range(38)] == want
    assert cm.walk(x, cm.XERIAL) == (K, [(20, 3), (27, 3), (34, 3)], [(0, 1), (1, 1), (2, 1)], 3)
    # the tables of a failing walk hold the chunks in front of the failure
    assert cm.walk(a[:20], cm.HADOOP) == (T, [(8, 3), (15, 3)], [(0, 1), (1, 1)], 2)


# ---- the library's host walk (snappy_container_uncompressed_length: no kernel) ----
def host_walk(stream, fmt):
    try:
        return cm.OK, snappy_amd.container_uncompressed_length(stream, fmt)
    except snappy_amd.SnappyError as e:
        return e.code, None


def test_host_walk_follows_the_model():
    for name, make in cc.FOREIGN.items():
        fmt, stream, raw = make()
        assert host_walk(stream, fmt) == (cm.OK, len(raw)), name
    for name, (fmt, stream, status) in cc.walk_error_cases().items():
        assert host_walk(stream, fmt)[0] == status, name
    for fmt, s in ((cm.HADOOP, cc.abc_hadoop()), (cm.XERIAL, cc.abc_xerial()), (cm.HADOOP, cc.two_byte_varint())):
        for i in range(len(s) + 1):
            st, _, _, n = cm.walk(s[:i], fmt)
            assert host_walk(s[:i], fmt) == (st, n if st == cm.OK else None), (fmt, i)


def test_format_names_and_bounds():
    assert snappy_amd.container_format("hadoop") == snappy_amd.CONTAINER_HADOOP == cm.HADOOP
    assert snappy_amd.container_format("xerial") == snappy_amd.CONTAINER_XERIAL == cm.XERIAL
    assert snappy_amd.CONTAINER_HEADER == cm.header()
    with pytest.raises(snappy_amd.SnappyError):
        snappy_amd.container_format("framed")
    with pytest.raises(snappy_amd.SnappyError) as e:
        snappy_amd.container_uncompressed_length(b"", 2)
    assert e.value.code == snappy_amd.ERR_ARG
    # stream header + a header per chunk + the long-record bound of the pieces
    for fmt, hdr, ident, default in ((cm.HADOOP, 8, 0, 131072), (cm.XERIAL, 4, 16, 32768)):
        for n, block in ((0, 0), (1, 0), (5 * 131072 + 17, 0), (100, 7), (1 << 20, 4096)):
            chunks = -(-n // (block or default))
            assert snappy_amd.max_container_output(n, block, fmt) == \
                ident + hdr * chunks + snappy_amd.max_long_records_output(n, chunks)
    assert snappy_amd.max_container_output(10, (1 << 30) + 1, cm.HADOOP) == 0
    assert snappy_amd.max_container_output(10, 0, 2) == 0

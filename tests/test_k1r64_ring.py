"""K1r64's register ring: far, wrap and edge candidates, and the smallest units.

K1r64 keeps only a block's last 128 segments of 256 bytes in registers.  A
candidate older than that is fetched from memory (inside the asm statement, and
again at every step of a match extension, because the ring moves while a match
extends); a candidate in segment 127 (mod 128) reads the register pair that
wraps around the ring; the next segment is staged by LDS-DMA only when the
unit's base is 4-aligned and the segment is whole.  Text reaches these paths on
about one round in a hundred.  A candidate more than 32 KiB back only survives
in the 4,096-slot table when the bytes in between insert into few slots: one
long run, or two-symbol noise.  Each input below (four units, four seeds) is
dense in one kind of candidate that way:

* far_run: 12 KiB of `sparse` bytes, 36,000 equal bytes (one copy, whose
  extension replaces the whole ring), then plants of 4-399 bytes copied from the sparse
  part: candidates that left the ring, at every dword alignment, with matches
  short, past 64 bytes and past the token's long form.
* far_alpha: the same with 36,000 two-symbol bytes in between: the ring advances
  one segment per refresh, and thousands of near copies sit between the far ones.
* wrap: two-symbol noise, `sparse` bytes around segment 127, and plants copied
  from sources that walk through it: resident candidates whose 64 dwords span
  the ring's last and first register, at every lane offset.
* edge: two-symbol noise, 10 KiB of `sparse`, and plants whose source tracks the
  first resident byte as the position advances: candidates that are far or
  resident by a few bytes, and long matches that change sides while they extend.

A copy found at p with candidate c is classified without restating the ring:
with F(p) = ((p >> 8) - 126) << 8, the ring's first resident byte lies in
[F(p) - 256, F(p)] whenever the kernel looks at c, so c + 512 <= F(p) is surely
far, c >= F(p) surely resident (a wrap hit if c's segment is 127 mod 128), and
F(p) - 512 <= c < F(p) is the edge band.

Measured per unit (test_inputs_have_their_properties prints them), units of
65,536 / 61,001 bytes:

* far_run: 111-140 / 98-103 surely-far hits, 62-65 / 46-49 of them of 64 bytes
  or more, 31-33 / 20-24 of 259 or more, every c % 4 class 23 / 19 or more.
* far_alpha: 126-136 / 97-105, 62-66 / 48-50, 29-33 / 23-25, classes 27 / 17 or
  more, among 7,800 tokens.
* wrap: 190-206 / 162-174 wrap hits on 60-63 / 59-63 of the 64 lane offsets,
  50-59 / 46-53 of 64 bytes or more, every c % 4 class 43 / 37 or more.
* edge: 53-58 / 54-58 hits in the edge band, 9-12 / 10-12 of them of 320 bytes or
  more (42 / 43 over the four units).

What each is for showed on builds with one comparison changed: a residency test
in the match extension that is off by one segment changes the bytes of the edge
input alone (the far inputs' candidates lie deep, and the earlier K1r inputs
never leave the ring); the same slip in the asm statement's compare, or a wrap
select that is off by one lane, changes far_alpha, wrap, edge and the smallest
units.

The shapes run every input as one stream of 65,536-byte blocks (whole, and with
a last block of 61,001 bytes whose final segment is partial) and as streams of
65,536 and of 61,001 bytes (units 1-3 start at odd addresses: byte loads, no
staging).  Further: one stream at every input and output alignment, the first
unit sizes past K1r's 32,768 bytes (with far0 units, whose last positions find
candidates in segment 0 after it has left the ring), and the unit counts around the scan
kernel's switch at 8,192 units.  The bar is the oracle's bytes and unit
offsets, bit for bit, and the round trip."""
import functools
import math

import numpy as np
import pytest

import datagen
import oracle
import snappy_amd
from test_k1r_flush_inloop import probe_unit, sparse

BLOCK = 65536
SHORT = 61001
UNITS = 4
INPUTS = ["far_run", "far_alpha", "wrap", "edge"]
SEEDS = {"far_run": 410, "far_alpha": 420, "wrap": 430, "edge": 440}
# (layout, chunk, bytes, the length the units are built at)
SHAPES = [("single", BLOCK, UNITS * BLOCK, BLOCK), ("single", BLOCK, 3 * BLOCK + SHORT, BLOCK),
          ("streams", BLOCK, UNITS * BLOCK, BLOCK), ("streams", SHORT, UNITS * SHORT, SHORT)]
SMALL_CHUNKS = [32768, 32769, 33023, 33024, 33025]  # K1r's largest unit (the control), then K1r64's smallest
SCAN_UNITS = [8191, 8192, 8193, 16384, 16385]       # SNAPPY_K3_WAVE_MAX = 8,192
SCAN_CHUNK = 16

FAR_SRC, FAR_FILL = 12288, 36000
FAR_PLANTS = FAR_SRC + FAR_FILL
WRAP_PLANTS = 34000
EDGE_SRC = (3072, 13312)
EDGE_PLANTS = 36608
FAR0_PLANTS = 32560


def span(rng, lo: int, hi: int) -> int:
    return int(rng.integers(lo, hi + 1))


def far(seed: int, L: int, run: bool) -> np.ndarray:
    rng = np.random.default_rng([seed, 1])
    a = rng.integers(2, 256, L, dtype=np.uint8)
    a[:FAR_SRC] = sparse(seed, FAR_SRC)
    a[FAR_SRC:FAR_PLANTS] = 0 if run else rng.integers(0, 2, FAR_FILL, dtype=np.uint8)
    classes = ((4, 11), (12, 63), (64, 139), (259, 399))
    p, k = FAR_PLANTS, 0
    while True:
        p += span(rng, 2, 8)
        ln = span(rng, *classes[k % 4])
        if p + ln > L:
            return a
        s = int(rng.integers(16, FAR_SRC - 420))
        a[p:p + ln] = a[s:s + ln]
        p += ln
        k += 1


def wrap(seed: int, L: int) -> np.ndarray:
    rng = np.random.default_rng([seed, 1])
    a = rng.integers(0, 2, L, dtype=np.uint8)
    a[32256:33280] = sparse(seed, 1024)  # segment 127 is [32512, 32768)
    classes = ((4, 11), (12, 63), (64, 299))
    p, k = WRAP_PLANTS, 0
    while True:
        ln = span(rng, *classes[k % 3])
        if p + ln > L:
            return a
        s = 32504 + 5 * k % 272
        a[p:p + ln] = a[s:s + ln]
        p += ln + span(rng, 20, 59)
        k += 1


def first_resident(p: int) -> int:
    """F(p): the ring's first resident byte once the segment after p's is loaded."""
    return ((p >> 8) - 126) << 8


def edge(seed: int, L: int) -> np.ndarray:
    rng = np.random.default_rng([seed, 1])
    a = rng.integers(0, 2, L, dtype=np.uint8)
    a[EDGE_SRC[0]:EDGE_SRC[1]] = sparse(seed, EDGE_SRC[1] - EDGE_SRC[0])
    classes = ((4, 11), (12, 63), (64, 258), (259, 699))
    p, k = EDGE_PLANTS, 0
    while True:
        sep = span(rng, 2, 8)
        ln = span(rng, *classes[k % 4])
        if p + sep + ln > L:
            return a
        a[p:p + sep] = rng.integers(2, 256, sep, dtype=np.uint8)
        p += sep
        s = first_resident(p) - 256 + int(rng.integers(-260, 300))
        a[p:p + ln] = a[s:s + ln]
        p += ln
        k += 1


def unit_of(name: str, seed: int, L: int) -> np.ndarray:
    if name == "far_run":
        return far(seed, L, True)
    if name == "far_alpha":
        return far(seed, L, False)
    return wrap(seed, L) if name == "wrap" else edge(seed, L)


@functools.lru_cache(maxsize=None)
def make(name: str, L: int) -> np.ndarray:
    """Four units of L bytes, one seed each."""
    a = np.concatenate([unit_of(name, SEEDS[name] + u, L) for u in range(UNITS)])
    a.setflags(write=False)
    return a


def data(name: str, n: int, L: int) -> np.ndarray:
    return make(name, L)[:n]


@functools.lru_cache(maxsize=None)
def want(name: str, layout: str, chunk: int, n: int, L: int):
    """The oracle's bytes (and unit offsets for streams), computed once per case."""
    a = data(name, n, L)
    if layout == "single":
        return oracle.compress(a.tobytes()), None
    out, offs = oracle.compress_streams(a, chunk)
    return out.tobytes(), offs.copy()


@functools.lru_cache(maxsize=None)
def hits(name: str, n: int, L: int):
    """probe_unit() of every unit of L bytes (the last one may be shorter), its
    encoded size checked against the oracle's stream of that unit; per unit the
    copies as (p, c, length)."""
    a = data(name, n, L)
    _, offs = oracle.compress_streams(a, L)
    b = a.tobytes()
    res = []
    for u in range((n + L - 1) // L):
        unit = b[u * L:(u + 1) * L]
        toks, size = probe_unit(unit)[:2]
        hdr = 1 + (len(unit) >= 128) + (len(unit) >= 16384)
        assert hdr + size == int(offs[u + 1]) - int(offs[u]), (name, L, u)
        out, end = [], 0
        for gap, ln, off in toks:
            p = end + gap
            out.append((p, p - off, ln))
            end = p + ln
        res.append(out)
    return res


def classify(unit_hits):
    """(surely far, wrap, edge band) hits of one unit, each as (c, length)."""
    far_, wrap_, band = [], [], []
    for p, c, ln in unit_hits:
        f = first_resident(p)
        if c + 512 <= f:
            far_.append((c, ln))
        elif c >= f:
            if (c >> 8) & 127 == 127:
                wrap_.append((c, ln))
        elif c >= f - 512:
            band.append((c, ln))
    return far_, wrap_, band


def mod4(cs):
    return [sum(1 for c, _ in cs if c % 4 == r) for r in range(4)]


def need(bound: int, share: float) -> int:
    return math.ceil(bound * share)


def far0(seed: int, L: int) -> np.ndarray:
    """A unit a little over 32 KiB whose last positions find candidates in segment
    0, the one segment that can have left the ring: 512 `sparse` bytes, two-symbol
    noise, and from FAR0_PLANTS on plants of 4-24 bytes copied from [16, 256)."""
    rng = np.random.default_rng([seed, 1])
    a = rng.integers(0, 2, L, dtype=np.uint8)
    a[:512] = sparse(seed, 512)
    p = FAR0_PLANTS
    while True:
        sep = span(rng, 2, 4)
        ln = span(rng, 4, 24)
        if p + sep + ln > L:
            return a
        a[p:p + sep] = rng.integers(2, 256, sep, dtype=np.uint8)
        p += sep
        s = int(rng.integers(16, 256 - ln))
        a[p:p + ln] = a[s:s + ln]
        p += ln


@functools.lru_cache(maxsize=None)
def small_input(chunk: int) -> np.ndarray:
    """Four units of four-symbol noise and four of `sparse` (prefixes of the same
    bytes at every chunk), then four of far0."""
    top = UNITS * max(SMALL_CHUNKS)
    a = np.concatenate([np.random.default_rng(451).integers(0, 4, top, dtype=np.uint8)[:UNITS * chunk],
                        sparse(452, top)[:UNITS * chunk]] + [far0(460 + u, chunk) for u in range(UNITS)])
    a.setflags(write=False)
    return a


def small_far_hits(chunk: int):
    """Per far0 unit, the copies that surely took the far path.  A round's window
    starts at most 62 before its probe, so at p >= 32,575 the window lies in
    segment 127 or later and the ring holds segment 128: segment 0 has left it.
    The model's encoded size is checked against the oracle's stream here too."""
    a = small_input(chunk).tobytes()
    _, offs = small_want(chunk)
    res = []
    for u in range(2 * UNITS, 3 * UNITS):
        toks, size = probe_unit(a[u * chunk:(u + 1) * chunk])[:2]
        assert 3 + size == int(offs[u + 1]) - int(offs[u]), (chunk, u)
        n, end = 0, 0
        for gap, ln, off in toks:
            p = end + gap
            n += p >= 32575 and p - off < 256
            end = p + ln
        res.append(n)
    return res


@functools.lru_cache(maxsize=None)
def small_want(chunk: int):
    out, offs = oracle.compress_streams(small_input(chunk), chunk)
    return out.tobytes(), offs.copy()


@functools.lru_cache(maxsize=None)
def scan_input(units: int) -> np.ndarray:
    a = datagen.make("T", units * SCAN_CHUNK, 46)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def scan_want(units: int):
    out, offs = oracle.compress_streams(scan_input(units), SCAN_CHUNK)
    return out.tobytes(), offs.copy()


def test_inputs_have_their_properties():
    """No GPU: the probe model (its encoded sizes equal to the oracle's stream
    lengths, unit by unit) shows what each input is for.  The bounds are
    conditions on the generators, per unit.  At 61,001 bytes they are scaled by
    the share of the plant region that is left: (61,001 - 48,288) / (65,536 -
    48,288) for the far inputs, (61,001 - 34,000) / (65,536 - 34,000) for wrap,
    and 1 for edge, whose sources lie in the sparse bytes only for plants before
    45,056.  And the oracle decodes what it encoded, for every input and shape."""
    for name in INPUTS:
        for L in (BLOCK, SHORT):
            if name == "edge":
                share = 1.0
            else:
                start = WRAP_PLANTS if name == "wrap" else FAR_PLANTS
                share = (L - start) / (BLOCK - start)
            long_band = 0
            for u, uh in enumerate(hits(name, UNITS * L, L)):
                far_, wrap_, band = classify(uh)
                lanes = len({(c >> 2) & 63 for c, _ in wrap_})
                long_b = sum(1 for _, ln in band if ln >= 320)
                long_band += long_b
                print(name, L, u, "tokens", len(uh),
                      "far", len(far_), ">= 64", sum(1 for _, ln in far_ if ln >= 64),
                      ">= 259", sum(1 for _, ln in far_ if ln >= 259), "c % 4", mod4(far_),
                      "wrap", len(wrap_), "lanes", lanes, ">= 64", sum(1 for _, ln in wrap_ if ln >= 64),
                      "c % 4", mod4(wrap_), "band", len(band), ">= 320", long_b)
                if name.startswith("far"):
                    assert len(far_) >= need(90, share), (name, L, u)
                    assert sum(1 for _, ln in far_ if ln >= 64) >= need(40, share), (name, L, u)
                    assert sum(1 for _, ln in far_ if ln >= 259) >= need(20, share), (name, L, u)
                    assert min(mod4(far_)) >= need(10, share), (name, L, u)
                elif name == "wrap":
                    assert len(wrap_) >= need(150, share), (name, L, u)
                    assert lanes >= need(56, share), (name, L, u)
                    assert min(mod4(wrap_)) >= need(30, share), (name, L, u)
                    assert sum(1 for _, ln in wrap_ if ln >= 64) >= need(30, share), (name, L, u)
                else:
                    assert len(band) >= 15 and long_b >= 2, (name, L, u)
            if name == "edge":
                assert long_band >= 8, (name, L)
        # the short last block of the second shape: the model holds there too
        hits(name, 3 * BLOCK + SHORT, BLOCK)
        for layout, chunk, n, L in SHAPES:
            a = data(name, n, L)
            out, offs = want(name, layout, chunk, n, L)
            if layout == "single":
                assert oracle.decompress(out) == a.tobytes(), (name, layout, n)
            else:
                back = oracle.decompress_streams(np.frombuffer(out, dtype=np.uint8), offs, n, chunk)
                assert np.array_equal(back, a), (name, chunk)
    for chunk in SMALL_CHUNKS:
        a = small_input(chunk)
        out, offs = small_want(chunk)
        assert offs.size == 3 * UNITS + 1
        if chunk > 32768:  # K1r64: far candidates in each far0 unit, even with one byte past the ring
            far0_hits = small_far_hits(chunk)
            print("far0", chunk, "surely-far hits per unit", far0_hits)
            assert min(far0_hits) >= (4 if chunk == 32769 else 15), (chunk, far0_hits)
        back = oracle.decompress_streams(np.frombuffer(out, dtype=np.uint8), offs, a.size, chunk)
        assert np.array_equal(back, a), chunk
    for units in SCAN_UNITS:
        a = scan_input(units)
        out, offs = scan_want(units)
        assert offs.size == units + 1
        back = oracle.decompress_streams(np.frombuffer(out, dtype=np.uint8), offs, a.size, SCAN_CHUNK)
        assert np.array_equal(back, a), units


def to_dev(a: np.ndarray):
    import torch
    return torch.from_numpy(np.array(a)).cuda()


def check_streams(codec, a: np.ndarray, chunk: int, out: bytes, want_offs: np.ndarray):
    comp, offs = codec.compress_tensor(to_dev(a), chunk=chunk, layout=snappy_amd.STREAMS)
    assert np.array_equal(offs.cpu().numpy().astype(np.uint64), want_offs)
    assert comp.cpu().numpy().tobytes() == out
    back = codec.decompress_tensor(comp, offs, a.size, chunk=chunk, layout=snappy_amd.STREAMS)
    assert np.array_equal(back.cpu().numpy(), a)


@pytest.mark.gpu
@pytest.mark.parametrize("layout,chunk,n,L", SHAPES)
@pytest.mark.parametrize("name", INPUTS)
def test_ring_paths(codec, name, layout, chunk, n, L):
    a = data(name, n, L)
    out, want_offs = want(name, layout, chunk, n, L)
    if layout == "streams":
        check_streams(codec, a, chunk, out, want_offs)
        return
    comp, offs = codec.compress_tensor(to_dev(a), chunk=chunk, layout=snappy_amd.SINGLE)
    assert comp.cpu().numpy().tobytes() == out
    back = codec.decompress_tensor(comp, offs, n, chunk=chunk, layout=snappy_amd.SINGLE)
    assert np.array_equal(back.cpu().numpy(), a)


@pytest.mark.gpu
@pytest.mark.parametrize("s_in", range(4))
@pytest.mark.parametrize("name", ["far_alpha", "edge"])
def test_single_stream_any_alignment(codec, name, s_in):
    """One stream whose first byte sits s_in bytes past a dword boundary (every
    block's base is then unaligned: byte loads, no staging, unaligned far
    gathers), written to an output s_out bytes past one.  The stream is the
    oracle's; no byte before the output pointer changes, and none at or after
    max_output bytes past it, the capacity the header promises."""
    import torch
    n = UNITS * BLOCK
    a = data(name, n, BLOCK)
    out_want, _ = want(name, "single", BLOCK, n, BLOCK)
    cap = codec.max_output(n, BLOCK, snappy_amd.SINGLE)
    pad = 64
    xin = torch.zeros(pad + n + pad, dtype=torch.uint8, device="cuda")
    xin[pad + s_in:pad + s_in + n] = to_dev(a)
    for s_out in range(4):
        buf = torch.full((pad + cap + pad,), 0xA5, dtype=torch.uint8, device="cuda")
        offs = torch.empty(UNITS + 1, dtype=torch.int64, device="cuda")
        back = torch.full((n + 8,), 0xA5, dtype=torch.uint8, device="cuda")
        o = pad + s_out
        codec._bind_stream()  # torch's stream: the fills and copies above are ordered before the kernels
        length = codec.compress_ptr(xin.data_ptr() + pad + s_in, n, BLOCK, snappy_amd.SINGLE,
                                    buf.data_ptr() + o, offs.data_ptr())
        codec.decompress_ptr(buf.data_ptr() + o, offs.data_ptr(), n, BLOCK, snappy_amd.SINGLE, back.data_ptr())
        torch.cuda.synchronize()
        got = buf.cpu().numpy()
        assert length <= cap
        assert got[o:o + length].tobytes() == out_want, (name, s_in, s_out)
        assert (got[:o] == 0xA5).all() and (got[o + cap:] == 0xA5).all(), (name, s_in, s_out)
        assert np.array_equal(back.cpu().numpy()[:n], a), (name, s_in, s_out)


@pytest.mark.gpu
@pytest.mark.parametrize("chunk", SMALL_CHUNKS)
def test_smallest_k1r64_units(codec, chunk):
    """Units of 32,769, 33,023, 33,024 and 33,025 bytes: 1, 255, 256 and 257
    bytes beyond the ring's 128 initial segments, as noise, `sparse` bytes and
    far0 units (candidates in segment 0 once it has left the ring); 32,768 is K1r
    on the same noise and sparse bytes."""
    check_streams(codec, small_input(chunk), chunk, *small_want(chunk))


@pytest.mark.gpu
@pytest.mark.parametrize("units", SCAN_UNITS)
def test_scan_kernel_boundary(codec, units):
    """The one-wave scan up to 8,192 units, the block scan past them."""
    check_streams(codec, scan_input(units), SCAN_CHUNK, *scan_want(units))

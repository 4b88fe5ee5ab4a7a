"""K2 (k2_emit_units) on planted token streams: direct-to-HBM passes and edges.

K2 writes a unit's elements in passes of 128 (the tokens, then one pseudo-token
for the tail literal).  A pass whose bytes fit the 4,096-byte LDS stage is
assembled there (put_element_lds, the LDS k2_long_literals); a larger one goes
straight to HBM (put_element, put_copy, the HBM k2_long_literals with its byte
head, realigned dwords, byte tail and guarded read at the input's end).  Text,
noise and the K1r inputs give staged passes only, and random bytes a direct pass
of one pseudo-token.  The inputs here are built so that both paths see every
kind of element, and k2_passes() (the pass layout restated on probe_unit(), its
unit sizes equal to the oracle's) proves it without a GPU:

* planted: random bytes with planted copies.  A gap of fresh bytes, then bytes
  copied from the start of one of the last six gaps, then a byte that ends the
  match.  Gaps of 1-16, 17-60, 58-63, 252-260 and 300-700 bytes and copies of
  4-11, 12-63, 62-71, 124-136 and 255-262 mixed: every full 32 KiB unit has
  direct passes of 128 tokens with short literals (the 20-byte load), long ones
  (several per pass) and split copies, and the input has the gaps on both sides
  of every header width (16 / 17, 60 / 62, 256 / 260: the probe steps make 61
  and 257 unreachable after a copy) and the copies around put_copy's split
  (64-69) and the token word's escape (258, 259).
* planted_dense: the same with gaps of 1-48.  Its passes are staged at 2-4 KiB
  with hundreds of split copies: the staged counterpart.
* exact token counts: a 32,768-byte unit that is planted_dense up to the end of
  token k and random bytes after it, k on both sides of a pass (128) and of a
  segment (256): the pseudo-token is alone in its pass / segment, or the last
  live lane of a full pass.
* tail sweep: a short last unit cut after a token, then t random bytes, t
  around every header width and around the 16 / 20 bytes of the short-literal
  load.  Cut from planted_dense the last pass is staged, cut from planted it
  is direct.  61 and 257 (the first length of each header width) only occur
  this way.
* staging boundary: pass totals of exactly 4,096 (staged) and 4,097 (direct),
  with one live element and with 128.

Measured (test_inputs_have_their_properties prints them), 32 KiB units:

* planted: 227-266 tokens per unit; 2 direct passes of 64 or more live tokens
  per unit (totals of 6-14 KiB), holding per unit 82-95 literals of 16 bytes or
  fewer, 120-137 longer ones and 57-66 copies over 64 bytes.  Over the input:
  gaps of exactly 16 / 17 / 60 / 62 / 252 / 256 / 260: 25 / 5 / 60 / 32 / 7 / 27 /
  33; copies of exactly 64 / 65 / 67 / 68 / 69: 29 / 16 / 16 / 10 / 18, of 258 /
  259: 7 / 8, of 128-133: 30.  At 4,096-byte units every pass is staged; at
  16,384, 65,535 and 65,536 bytes 8 passes are direct.
* planted_dense: 575-626 tokens per unit, every pass staged at every unit size
  (full passes of 2,645-3,834 bytes), 437 split copies.
* exact counts: tails of 25,391 (k = 127) down to 3,523 bytes (512); up to 257
  the pseudo-token's pass is direct, at 512 it is staged.
* tail sweep: planted_dense is cut after token 171 (a staged last pass of 45
  elements), planted after token 181 (a direct one of 55, 4,258 bytes before
  the tail).

The bar is the oracle's bytes and unit offsets, bit for bit, a length within
max_output, the round trip, and an output buffer whose bytes before the
pointer and from the returned length on are untouched: K2 is the only kernel
that writes the stream, and it writes [o, o + total) in every path."""
import functools

import numpy as np
import pytest

import oracle
import snappy_amd
from test_k1r_flush_inloop import copy_bytes, literal_bytes, probe_unit

TOTAL = 128 << 10
UNIT = 32768
PASS, STAGE = 128, 4096  # SNAPPY_K2_PASS, SNAPPY_K2_STAGE
INPUTS = ["planted", "planted_dense"]
CHUNKS = [4096, 16384, 32768, 65535]
COUNTS = [127, 128, 129, 255, 256, 257, 384, 512]
TAILS = [0, 1, 2, 3, 4, 15, 16, 17, 19, 20, 21, 60, 61, 256, 257]
ALIGN_TAILS = [3, 16, 17, 61]
BOUNDARY = ["alone_4096", "alone_4097", "full_4096", "full_4097"]
SENTINEL = 0xA5

GAPS = ((1, 16), (17, 60), (58, 63), (252, 260), (300, 700))
DENSE_GAPS = ((1, 16), (17, 48))
LENS = ((4, 11), (12, 63), (62, 71), (124, 136), (255, 262))
# how often each class is drawn: short gaps and copies often enough for 128
# tokens to fit a few KiB, the long ones often enough for every exact value
GAP_W = (0.42, 0.26, 0.16, 0.10, 0.06)
DENSE_GAP_W = (0.6, 0.4)
LEN_W = (0.32, 0.26, 0.26, 0.08, 0.08)
DENSE_LEN_W = (0.54, 0.10, 0.26, 0.06, 0.04)


def span(rng, lo: int, hi: int) -> int:
    return int(rng.integers(lo, hi + 1))


def plant(seed: int, n: int, gaps, gap_w, len_w) -> np.ndarray:
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 256, n, dtype=np.uint8)  # every gap is fresh random bytes
    starts, p = [], 0
    while True:
        g = span(rng, *gaps[int(rng.choice(len(gaps), p=gap_w))])
        ln = span(rng, *LENS[int(rng.choice(len(LENS), p=len_w))])
        if p + g + ln + 1 > n:
            return a
        if starts:
            s = starts[int(rng.integers(len(starts)))]
            a[p + g:p + g + ln] = a[s:s + ln]
            if a[p + g + ln] == a[s + ln]:  # the match ends where it was planted
                a[p + g + ln] ^= 0x80
        starts = (starts + [p])[-6:]
        p += g + ln


@functools.lru_cache(maxsize=None)
def make(name: str) -> np.ndarray:
    if name == "planted":
        a = plant(501, TOTAL, GAPS, GAP_W, LEN_W)
    else:
        a = plant(502, TOTAL, DENSE_GAPS, DENSE_GAP_W, DENSE_LEN_W)
    a.setflags(write=False)
    return a


def k2_passes(unit: bytes):
    """K2's view of one unit: probe_unit()'s tokens plus the pseudo-token (token
    nt, a literal of L - end bytes, possibly none) in passes of 128.  Returns nt,
    the elements as (gap, length, offset, position of the literal's first byte),
    the passes as (live, total, staged) and the encoded size (probe_unit()'s,
    which the passes' totals must add up to)."""
    toks, size = probe_unit(unit)[:2]
    elems, end = [], 0
    for gap, ln, off in toks:
        elems.append((gap, ln, off, end))
        end += gap + ln
    elems.append((len(unit) - end, 0, 0, end))
    passes = []
    for c in range(0, len(elems), PASS):
        total = 0
        for gap, ln, off, _ in elems[c:c + PASS]:
            total += (literal_bytes(gap) if gap else 0) + (copy_bytes(ln, off) if ln else 0)
        passes.append((len(elems[c:c + PASS]), total, total <= STAGE))
    assert sum(t for _, t, _ in passes) == size
    return len(toks), elems, passes, size


def varint_len(n: int) -> int:
    return 1 + (n >= 128) + (n >= 16384)


@functools.lru_cache(maxsize=None)
def want(key, chunk: int):
    """The oracle's bytes and unit offsets of a STREAMS case, computed once."""
    out, offs = oracle.compress_streams(data(key), chunk)
    return out.tobytes(), offs.copy()


@functools.lru_cache(maxsize=None)
def want_single(key) -> bytes:
    return oracle.compress(data(key).tobytes())


@functools.lru_cache(maxsize=None)
def model(key, chunk: int):
    """k2_passes() of every unit, its size plus the varint checked against the oracle's offsets."""
    b = data(key).tobytes()
    _, offs = want(key, chunk)
    res = []
    for u in range((len(b) + chunk - 1) // chunk):
        unit = b[u * chunk:(u + 1) * chunk]
        r = k2_passes(unit)
        assert varint_len(len(unit)) + r[3] == int(offs[u + 1]) - int(offs[u]), (key, chunk, u)
        res.append(r)
    return res


def cut(base: bytes, k: int, t: int, seed: int) -> bytes:
    """base up to the end of its token k - 1, then t random bytes, the first of
    them different from the byte that would have continued the match."""
    gap, ln, off, pos = k2_passes(base)[1][k - 1]
    end = pos + gap + ln
    tail = np.random.default_rng([seed, k, t]).integers(0, 256, t, dtype=np.uint8)
    if t and tail[0] == base[end - off]:
        tail[0] ^= 0x80
    return base[:end] + tail.tobytes()


def front(name: str) -> bytes:
    return make(name)[:UNIT].tobytes()


@functools.lru_cache(maxsize=None)
def tail_k(name: str) -> int:
    """The token after which the tail sweep cuts unit 1 of `name`: inside the
    second pass (so a few dozen tokens share it with the pseudo-token), a copy of
    20 bytes or more (the matcher finds it whatever follows), and for planted a
    pass that is already direct without its tail."""
    elems = k2_passes(make(name)[UNIT:2 * UNIT].tobytes())[1]
    for k in range(PASS + 40, 2 * PASS):
        done = sum((literal_bytes(g) if g else 0) + copy_bytes(n, o) for g, n, o, _ in elems[PASS:k])
        if elems[k - 1][1] >= 20 and (name == "planted_dense" or done > STAGE + 64):
            return k
    raise AssertionError(name)


def boundary_tail(k: int, want_total: int) -> int:
    """The tail length at which the pseudo-token's pass of a unit cut after
    planted_dense's token k - 1 totals want_total bytes."""
    elems = k2_passes(front("planted_dense"))[1]
    c = k // PASS * PASS
    done = sum((literal_bytes(g) if g else 0) + copy_bytes(n, o) for g, n, o, _ in elems[c:k])
    for t in range(17, want_total):
        if done + literal_bytes(t) == want_total:
            return t
    raise AssertionError((k, want_total))


@functools.lru_cache(maxsize=None)
def data(key) -> np.ndarray:
    """Every input by key: a name; ("count", k); ("tail", name, t); ("last", name); ("boundary", which)."""
    if isinstance(key, str):
        return make(key)
    if key[0] == "count":  # a unit of planted in front, the exact-count unit ends the input
        k = key[1]
        base = front("planted_dense")
        head = cut(base, k, 0, 0)
        b = front("planted") + cut(base, k, UNIT - len(head), 510)
    elif key[0] == "tail":  # one full unit in front, then the swept unit
        _, name, t = key
        b = front(name) + cut(make(name)[UNIT:2 * UNIT].tobytes(), tail_k(name), t, 520)
    elif key[0] == "last":  # the same cut, then a last token of 2 + 16 bytes that ends the input
        base = make(key[1])[UNIT:2 * UNIT].tobytes()
        pos = k2_passes(base)[1][tail_k(key[1]) - 1][3]  # a first probe after a copy: in the table
        b = front(key[1]) + cut(base, tail_k(key[1]), 2, 521) + base[pos:pos + 16]
    else:
        k = PASS if key[1].startswith("alone") else PASS - 1
        t = boundary_tail(k, int(key[1][-4:]))
        b = front("planted") + cut(front("planted_dense"), k, t, 530)
    a = np.frombuffer(b, dtype=np.uint8)
    a.setflags(write=False)
    return a


def reachable_gaps(limit: int):
    """The gaps a copy can follow another copy at: probes at step skip >> 5, skip
    from 32 and one more after every miss."""
    out, p, skip = [], 0, 32
    while p <= limit:
        out.append(p)
        p += skip >> 5
        skip += 1
    return out


def direct_counts(elems, passes):
    """Over the direct passes of 64 or more live elements: their number, literals
    of 16 bytes or fewer, longer literals, copies over 64 bytes."""
    n = short = longer = split = 0
    for i, (live, _, staged) in enumerate(passes):
        if staged or live < 64:
            continue
        n += 1
        for gap, ln, _, _ in elems[i * PASS:(i + 1) * PASS]:
            short += 0 < gap <= 16
            longer += gap > 16
            split += ln > 64
    return n, short, longer, split


def test_inputs_have_their_properties():
    """No GPU: k2_passes() (unit sizes equal to the oracle's at every chunk size)
    shows what each input is for, and the oracle decodes what it encoded."""
    reach = reachable_gaps(400)
    first2 = min(g for g in reach if g > 60)
    first3 = min(g for g in reach if g > 256)
    print("smallest reachable gap with a 2-byte header", first2, "with a 3-byte header", first3,
          "reachable in 252-260", [g for g in reach if 252 <= g <= 260])
    assert (first2, first3) == (62, 260) and 61 not in reach and 255 not in reach and 257 not in reach
    assert 252 in reach and 256 in reach

    for name in INPUTS:
        for chunk in CHUNKS + [65536]:  # 65,536: the blocks of the SINGLE layout
            res = model(name, chunk)
            out, offs = want(name, chunk)
            back = oracle.decompress_streams(np.frombuffer(out, dtype=np.uint8), offs, TOTAL, chunk)
            assert np.array_equal(back, make(name)), (name, chunk)
            print(name, chunk, "passes staged / direct with one element / direct with more",
                  sum(s for r in res for _, _, s in r[2]),
                  sum(not s and live == 1 for r in res for live, _, s in r[2]),
                  sum(not s and live > 1 for r in res for live, _, s in r[2]))
        assert len(want_single(name)) == varint_len(TOTAL) + sum(r[3] for r in model(name, 65536))
        assert oracle.decompress(want_single(name)) == make(name).tobytes()

    res = model("planted", UNIT)
    for u, (nt, elems, passes, _) in enumerate(res):
        n, short, longer, split = direct_counts(elems, passes)
        print("planted", u, "tokens", nt, "direct passes of 64+", n, "in them literals <= 16", short,
              "longer", longer, "copies > 64", split, "pass totals", [t for _, t, _ in passes])
        assert n >= 2 and short >= 75 and longer >= 110 and split >= 50, (u, n, short, longer, split)
    gaps = [g for r in res for g, ln, _, _ in r[1] if ln]
    lens = [ln for r in res for _, ln, _, _ in r[1] if ln]
    gap_n = {g: gaps.count(g) for g in (16, 17, 60, first2, 252, 256, first3)}
    len_n = {n: lens.count(n) for n in (64, 65, 67, 68, 69, 258, 259)}
    mid = sum(1 for n in lens if 128 <= n <= 133)
    far_short = sum(1 for r in res for _, ln, off, _ in r[1] if 4 <= ln <= 11 and off >= 2048)
    print("planted gaps of exactly", gap_n, "copies of exactly", len_n, "of 128-133", mid,
          "of 4-11 at an offset >= 2048", far_short)
    assert min(gap_n.values()) >= 3, gap_n
    assert min(len_n[n] for n in (64, 65, 67, 68, 69)) >= 5 and min(len_n[258], len_n[259]) >= 3, len_n
    assert mid >= 3 and far_short >= 1
    assert not ({61, 255, 257} & set(gaps))

    res = model("planted_dense", UNIT)
    for u, (nt, elems, passes, _) in enumerate(res):
        totals = [t for _, t, _ in passes]
        print("planted_dense", u, "tokens", nt, "pass totals", min(totals[:-1]), "-", max(totals[:-1]),
              "copies > 64", sum(ln > 64 for _, ln, _, _ in elems))
        assert nt >= 4 * PASS and all(s for _, _, s in passes) and min(totals[:-1]) >= 2048, (u, totals)
    assert sum(ln > 64 for r in res for _, ln, _, _ in r[1]) >= 432

    for k in COUNTS:
        (_, _, _, _), (nt, elems, passes, _) = model(("count", k), UNIT)
        print("count", k, "tokens", nt, "tail", elems[-1][0], "last passes", passes[-2:])
        assert nt == k and len(data(("count", k))) == 2 * UNIT
        live, total, staged = passes[-1]
        assert live == k % PASS + 1 and (k > 257 or (elems[-1][0] > STAGE and not staged))
        if k in (127, 255):  # the pseudo-token is the last live lane of a full, direct pass
            assert live == PASS
        if k in (128, 256):  # alone in its pass (at 256: in its segment)
            assert live == 1 and total == 3 + elems[-1][0]

    for name in INPUTS:
        k = tail_k(name)
        for t in TAILS:
            _, (nt, elems, passes, _) = model(("tail", name, t), UNIT)
            assert nt == k and elems[-1][0] == t, (name, t, nt, elems[-1])
            live, total, staged = passes[-1]
            assert live == k % PASS + 1 and staged == (name == "planted_dense"), (name, t, passes[-1])
            if 0 < t <= 16:  # its 20-byte load would pass the input's end
                assert elems[-1][3] + 20 > len(data(("tail", name, t))) - UNIT
        # a token whose literal takes the narrow load: the matcher probes up to 16
        # bytes before the end, so its copy is at most 18 bytes and reaches the end
        _, (nt, elems, passes, _) = model(("last", name), UNIT)
        assert nt == k + 1 and elems[-2][:2] == (2, 16) and elems[-1][0] == 0, (name, elems[-2:])
        assert elems[-2][3] + 20 > len(data(("last", name))) - UNIT
        assert passes[-1][2] == (name == "planted_dense")
        print("tail", name, "cut after token", k, "last pass", passes[-1], "last token", elems[-2])

    for which in BOUNDARY:
        _, (nt, elems, passes, _) = model(("boundary", which), UNIT)
        live, total, staged = passes[-1]
        print("boundary", which, "tokens", nt, "tail", elems[-1][0], "last pass", passes[-1])
        assert total == int(which[-4:]) and staged == (total <= STAGE)
        assert (nt, live) == ((PASS, 1) if which.startswith("alone") else (PASS - 1, PASS))
    assert data(("boundary", "alone_4096")).size - 4093 == data(("boundary", "alone_4097")).size - 4094


def run(codec, a: np.ndarray, chunk: int, layout: int, out_want: bytes, offs_want, s_in: int = 0, s_outs=(0,)):
    """Compress a placed s_in bytes past a dword boundary into a sentinel-filled
    buffer s_out bytes past one, decode the GPU's bytes on the GPU."""
    import torch
    n = a.size
    units = codec.num_units(n, chunk, layout)
    cap = codec.max_output(n, chunk, layout)
    pad = 64
    xin = torch.zeros(pad + n + pad, dtype=torch.uint8, device="cuda")
    xin[pad + s_in:pad + s_in + n] = torch.from_numpy(np.array(a)).cuda()
    for s_out in s_outs:
        buf = torch.full((pad + cap + pad,), SENTINEL, dtype=torch.uint8, device="cuda")
        offs = torch.empty(units + 1, dtype=torch.int64, device="cuda")
        back = torch.full((n + 8,), SENTINEL, dtype=torch.uint8, device="cuda")
        o = pad + s_out
        codec._bind_stream()  # torch's stream: the fills and copies above are ordered before the kernels
        length = codec.compress_ptr(xin.data_ptr() + pad + s_in, n, chunk, layout, buf.data_ptr() + o, offs.data_ptr())
        torch.cuda.synchronize()
        got = buf.cpu().numpy()
        assert length <= cap
        if offs_want is not None:
            assert np.array_equal(offs.cpu().numpy().astype(np.uint64), offs_want), (s_in, s_out)
        assert got[o:o + length].tobytes() == out_want, (s_in, s_out)
        assert (got[:o] == SENTINEL).all(), (s_in, s_out)
        assert (got[o + length:] == SENTINEL).all(), (s_in, s_out, np.flatnonzero(got[o + length:] != SENTINEL)[:8])
        # only the oracle's bytes reach the decoder
        codec.decompress_ptr(buf.data_ptr() + o, offs.data_ptr(), n, chunk, layout, back.data_ptr())
        torch.cuda.synchronize()
        assert np.array_equal(back.cpu().numpy()[:n], a), (s_in, s_out)
        assert (back.cpu().numpy()[n:] == SENTINEL).all(), (s_in, s_out)


@pytest.mark.gpu
@pytest.mark.parametrize("chunk", CHUNKS)
@pytest.mark.parametrize("name", INPUTS)
def test_planted_streams(codec, name, chunk):
    run(codec, make(name), chunk, snappy_amd.STREAMS, *want(name, chunk))


@pytest.mark.gpu
@pytest.mark.parametrize("name", INPUTS)
def test_planted_single(codec, name):
    run(codec, make(name), 65536, snappy_amd.SINGLE, want_single(name), None)


@pytest.mark.gpu
@pytest.mark.parametrize("k", COUNTS)
def test_exact_token_counts(codec, k):
    run(codec, data(("count", k)), UNIT, snappy_amd.STREAMS, *want(("count", k), UNIT))


@pytest.mark.gpu
@pytest.mark.parametrize("t", TAILS)
@pytest.mark.parametrize("name", INPUTS)
def test_tail_sweep(codec, name, t):
    run(codec, data(("tail", name, t)), UNIT, snappy_amd.STREAMS, *want(("tail", name, t), UNIT))


@pytest.mark.gpu
@pytest.mark.parametrize("s_in", range(4))
@pytest.mark.parametrize("name", INPUTS)
def test_last_token_narrow_load(codec, name, s_in):
    """The input ends with a token of a 2-byte literal and a 16-byte copy: a real
    token's literal less than 20 bytes before the input's end."""
    key = ("last", name)
    run(codec, data(key), UNIT, snappy_amd.STREAMS, *want(key, UNIT), s_in=s_in, s_outs=range(4))


@pytest.mark.gpu
@pytest.mark.parametrize("which", BOUNDARY)
def test_staging_boundary(codec, which):
    run(codec, data(("boundary", which)), UNIT, snappy_amd.STREAMS, *want(("boundary", which), UNIT))


@pytest.mark.gpu
@pytest.mark.parametrize("s_in", range(4))
@pytest.mark.parametrize("layout", ["streams", "single"])
def test_planted_any_alignment(codec, layout, s_in):
    """Input s_in bytes past a dword boundary, output at every s_out: the direct
    path's byte head, realigned dwords and byte tail at all sixteen pairs."""
    if layout == "streams":
        run(codec, make("planted"), UNIT, snappy_amd.STREAMS, *want("planted", UNIT), s_in=s_in, s_outs=range(4))
    else:
        run(codec, make("planted"), 65536, snappy_amd.SINGLE, want_single("planted"), None, s_in=s_in, s_outs=range(4))


@pytest.mark.gpu
@pytest.mark.parametrize("s_in", range(4))
@pytest.mark.parametrize("t", ALIGN_TAILS)
@pytest.mark.parametrize("name", INPUTS)
def test_tail_any_alignment(codec, name, t, s_in):
    """The stream's last bytes (the narrow loads, the guarded read at the input's
    end, the last unit's byte tail) at every input and output alignment."""
    key = ("tail", name, t)
    run(codec, data(key), UNIT, snappy_amd.STREAMS, *want(key, UNIT), s_in=s_in, s_outs=range(4))

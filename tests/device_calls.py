"""A catalogue of small device calls, one or more per device entry point of the
C ABI (include/snappy_amd.h), shared by test_stream_order.py and
test_call_sequences.py.  A plain module: nothing here touches the GPU at import,
and every expected result is computed on the CPU from what the tests already
have (the oracle, the frame / container / range models, the element encoders of
golden_inputs.py, the hostile inputs of the existing GPU tests).

A case has two worlds of equal shapes and dtypes: its inputs and a decoy.  The
decoy is itself a valid input of the same call with another result, so a call
that reads its input too early or too late gives wrong bytes or a wrong status,
never a hostile stream.  case.inputs() / case.decoy() are dicts of numpy arrays,
case.expect() / case.expect_decoy() dicts of what the call must leave: every
output buffer whole (the sentinel where nothing may be written; NAME#care = a
mask of the bytes that are compared, for a failing unit's own output range), and
the return codes and lengths under their names.  case.run(codec, dev) makes the
call on tensors that exist already (dev: name -> tensor, inputs and outputs) and
returns the host-side results; it allocates nothing on the device.  Cases with
async_form use the form the header documents as "returns once queued"; what
such a case reads afterwards (the decode status) is case.after(codec), called
once the stream has been synchronised.

kind: "ok", "fail" (a status is expected) or "large" (about 16 MiB: grow()
reallocates the scratch the small case of the family left)."""
import ctypes
import functools

import numpy as np

import datagen
import oracle
import snappy_amd
import container_cases as cc
import container_model as cm
import frame_model as fm
import frame_ranges_cases as frc
from golden_inputs import build_stream

SENT = 0xA5
B = 65536
E = snappy_amd
u8, i32, i64 = np.uint8, np.int32, np.int64


# ---- small helpers ----------------------------------------------------------------
def sent(n, dtype=u8):
    """n elements whose every byte is the sentinel"""
    return np.full(n * np.dtype(dtype).itemsize, SENT, dtype=u8).view(dtype).copy()


def image(n, data, dtype=u8):
    """data at the front of a sentinel buffer of n elements"""
    buf = sent(n, dtype)
    d = np.asarray(data, dtype=dtype) if not isinstance(data, (bytes, bytearray)) else np.frombuffer(data, dtype=u8)
    buf[:d.size] = d
    return buf


def arr(b):
    return np.frombuffer(bytes(b), dtype=u8).copy()


def T(n, seed):
    return datagen.make("T", n, seed)


def pairs(p):
    return np.array([v for x in p for v in x], dtype=i64)


def packed(lens):
    o, out = 0, []
    for n in lens:
        out.append((o, n))
        o += n
    return out


def P(t):
    return ctypes.c_void_p(t.data_ptr() if t is not None else 0)


def lib():
    return snappy_amd.lib()


def k5():
    import test_k5_index
    return test_k5_index


def k4():
    import test_k4_decode
    return test_k4_decode


def single_index(stream):
    """the block index of a valid SINGLE stream, by the serial walk's model"""
    st, n, units, ent = k5().k5_serial(stream)
    assert st == 0
    return n, ent


def streams_as_single(a):
    """(stream, block index) of oracle.compress(a) from its blocks' own streams: block
    i of the one stream is unit i of the 65,536-byte STREAMS layout without that
    unit's preamble, behind one preamble of the whole length"""
    payload, offs = oracle.compress_streams(a, B)
    payload, head = payload.tobytes(), fm.varint(a.size)
    out, ent = bytearray(head), [0]
    for u in range(len(offs) - 1):
        pre = len(fm.varint(min(B, a.size - u * B)))
        out += payload[int(offs[u]) + pre:int(offs[u + 1])]
        ent.append(len(out))
    return bytes(out), ent


_CRC = None


def crc32c_rows(rows):
    """masked CRC-32C of every row of a 2-D uint8 array (frame_model's table, one step
    per column over all rows at once)"""
    global _CRC
    if _CRC is None:
        fm.crc32c(b"")
        _CRC = np.array(fm._TABLE, dtype=np.uint32)
    c = np.full(rows.shape[0], 0xFFFFFFFF, dtype=np.uint32)
    for k in range(rows.shape[1]):
        c = _CRC[(c ^ rows[:, k]) & 0xFF] ^ (c >> 8)
    c ^= 0xFFFFFFFF
    return (((c >> 15) | (c << 17)) + np.uint32(0xA282EAD8)).astype(np.uint32)


def frame_of(a):
    """the framed stream compress_frame_device writes for a, with its chunk CRCs taken
    row-wise (a whole number of 65,536-byte chunks, then the last one)"""
    payload, offs = oracle.compress_streams(a, B)
    payload = payload.tobytes()
    full = a.size // B
    crcs = list(crc32c_rows(a[:full * B].reshape(full, B))) if full else []
    if a.size % B:
        crcs.append(fm.mask(fm.crc32c(a[full * B:].tobytes())))
    out = bytearray(fm.IDENTIFIER)
    for u in range(len(offs) - 1):
        out += fm.compressed(b"", payload[int(offs[u]):int(offs[u + 1])], crc=int(crcs[u]))
    return bytes(out)


def same_length(f0, f1, pad):
    """both streams closed with pad(k) so that they are equally long (pad(k) is k + 4 bytes)"""
    n = max(len(f0), len(f1)) + 4
    return f0 + pad(n - len(f0) - 4), f1 + pad(n - len(f1) - 4)


def ranges_image(raw, ranges, out_bytes, accepted=None):
    return arr(frc.expected(raw, ranges, out_bytes, accepted))


class Case:
    def __init__(self, name, family, kind, make, outputs, run, async_form=False, after=None, shares=()):
        self.name, self.family, self.kind, self.async_form = name, family, kind, async_form
        self._make, self._outputs, self._run, self._after = make, outputs, run, after
        self.shares = tuple(shares) if kind == "fail" else ()  # a failing case: the families that share a buffer or a status path with it

    def __repr__(self):
        return self.name

    @functools.lru_cache(maxsize=None)
    def _worlds(self):
        w = [self._make(0), self._make(1)]
        ins = [dict(w[0][0]), dict(w[1][0])]
        for k in ins[0]:
            a, b = np.ascontiguousarray(ins[0][k]), np.ascontiguousarray(ins[1][k])
            assert a.dtype == b.dtype and a.ndim == 1 and b.ndim == 1, (self.name, k)
            n = max(a.size, b.size) + (16 if a.dtype == u8 else 0)  # (room behind a byte stream, as the tests give it)
            ins[0][k], ins[1][k] = [np.concatenate([x, np.zeros(n - x.size, dtype=x.dtype)]) for x in (a, b)]
        return (ins[0], w[0][1]), (ins[1], w[1][1])

    def inputs(self):
        return self._worlds()[0][0]

    def decoy(self):
        return self._worlds()[1][0]

    def expect(self):
        return self._worlds()[0][1]

    def expect_decoy(self):
        return self._worlds()[1][1]

    def outputs(self):
        """name -> (elements, dtype) of every output buffer"""
        return self._outputs

    def run(self, codec, dev, bind=True):
        if bind:
            codec._bind_stream()
        return self._run(codec, dev)

    def after(self, codec):
        return self._after(codec) if self._after else {}


def differs(x, y):
    """two expectations tell their worlds apart"""
    for k in x:
        if k.endswith("#care"):
            continue
        a, b = np.asarray(x[k]), np.asarray(y[k])
        if a.shape != b.shape or not np.array_equal(a, b):
            return True
    return False


def compare(case, exp, outs, res):
    """outs: name -> numpy array read back from the output buffers; res: run()'s and
    after()'s results.  Asserts all of exp."""
    for k, want in exp.items():
        if k.endswith("#care"):
            continue
        if k in outs:
            got, care = outs[k], exp.get(k + "#care")
            assert got.dtype == want.dtype and got.shape == want.shape, (case.name, k, got.shape, want.shape)
            bad = np.nonzero((got != want) & care if care is not None else got != want)[0]
            assert bad.size == 0, f"{case.name}: {k}[{bad[0]}] = {got[bad[0]]}, want {want[bad[0]]} ({bad.size} differ)"
        else:
            assert k in res, (case.name, k)
            assert res[k] == want, f"{case.name}: {k} = {res[k]}, want {want}"


# ---- 1, 2: unit compress ----------------------------------------------------------
def compress_case(name, family, kind, n, chunk, layout):
    units = E.Codec.num_units(n, chunk, layout)
    cap = E.Codec.max_output(n, chunk, layout)

    def make(v):
        a = T(n, 100 + v)
        if layout == E.STREAMS:
            payload, offs = oracle.compress_streams(a, chunk)
        else:
            payload, offs = streams_as_single(a)
            payload = arr(payload)
        return {"x": a}, {"out": image(cap, payload), "offs": np.asarray(offs).astype(i64), "rc": 0}

    def run(codec, d):
        return {"rc": lib().snappy_amd_compress_device(codec._h, P(d["x"]), n, chunk, layout, P(d["out"]), P(d["offs"]),
                                                       None)}

    return Case(name, family, kind, make, {"out": (cap, u8), "offs": (units + 1, i64)}, run, async_form=True)


# ---- 3, 4: unit decode ------------------------------------------------------------
def _decode_run(n, chunk, layout, sync):
    def run(codec, d):
        fn = lib().snappy_amd_decompress_device if sync else lib().snappy_amd_decompress_device_async
        return {"rc": fn(codec._h, P(d["comp"]), P(d["offs"]), n, chunk, layout, P(d["out"]))}
    return run


def _status_after(codec):
    return {"status": codec.decompress_status()}


def decode_streams_case():
    n, chunk = 3 * 32768 + 1000, 32768

    def make(v):
        a = T(n, 110 + v)
        payload, offs = oracle.compress_streams(a, chunk)
        return {"comp": payload, "offs": offs.astype(i64)}, {"out": a.copy(), "rc": 0, "status": 0}

    return Case("decode_streams", "decode_streams", "ok", make, {"out": (n, u8)}, _decode_run(n, chunk, E.STREAMS, 0),
                async_form=True, after=_status_after)


HOSTILE = "copy-2 offset 0"


@functools.lru_cache(maxsize=None)
def hostile_units():
    """four good 8,192-byte units, the hostile unit test_k4_decode.test_hostile_streams
    puts between them, a fifth good unit, and every unit's decoded bytes (None: refused)"""
    m = k4()
    tape, rng = m.Tape(992, 1 << 20), np.random.default_rng(993)
    good = [m.varint(m.HCHUNK) + m.encode(m.filler(rng, m.HCHUNK), tape)[0] for _ in range(5)]
    body, code, _, _ = m.hostile_bodies()[HOSTILE]
    bad = m.varint(m.HCHUNK) + body
    assert code == E.ERR_OFFSET and m.oracle_accepts(bad, m.HCHUNK) is None
    return good, bad, [m.oracle_accepts(u, m.HCHUNK) for u in good]


def decode_streams_fail_case(sync=True):
    """the decoy is the same launch with a good unit in the hostile one's place"""
    H = 8192
    n = 5 * H

    def make(v):
        good, bad, raw = hostile_units()
        units = good[:2] + [bad if v == 0 else good[4]] + good[2:4]
        want = raw[:2] + [None if v == 0 else raw[4]] + raw[2:4]
        offs = np.cumsum([0] + [len(u) for u in units]).astype(i64)
        out, care = sent(n), np.ones(n, dtype=bool)
        for i, w in enumerate(want):
            if w is None:
                care[i * H:(i + 1) * H] = False  # (a failing unit may leave a prefix of its own range written)
            else:
                out[i * H:(i + 1) * H] = arr(w)
        st = E.ERR_OFFSET if v == 0 else 0
        exp = {"out": out, "out#care": care, "rc": st if sync else 0}
        if not sync:
            exp["status"] = st
        return {"comp": arr(b"".join(units)), "offs": offs}, exp

    if sync:
        return Case("decode_streams/fail", "decode_streams", "fail", make, {"out": (n, u8)},
                    _decode_run(n, H, E.STREAMS, 1), shares=("decode_streams", "decode_single"))
    return Case("decode_streams/fail_async", "decode_streams", "fail", make, {"out": (n, u8)},
                _decode_run(n, H, E.STREAMS, 0), async_form=True, after=_status_after,
                shares=("decode_streams", "decode_single"))


XBLOCK_OPS = [[["lit", B - 10, 21], ["copy", 40, 1000, 2], ["lit", 50, 22], ["lit", B, 23], ["copy", 64, 70000, 4],
               ["lit", 20, 24]],
              # the same elements in another order: the same length, other bytes and another index
              [["lit", 50, 32], ["copy", 40, 30, 2], ["lit", B - 10, 31], ["lit", B, 33], ["copy", 64, 70000, 4],
               ["lit", 20, 34]]]


def decode_single_case():
    """a copy that straddles the first block edge (v = 0: a literal does) and a copy-4
    from 70,000 bytes back in block 2: pass 2 decodes blocks 1 and 2"""
    n = 2 * B + 164

    def make(v):
        s = build_stream(XBLOCK_OPS[v])
        got_n, ent = single_index(s)
        assert got_n == n
        return {"comp": arr(s), "offs": np.array(ent, dtype=i64)}, {"out": arr(oracle.decompress(s)), "rc": 0,
                                                                    "status": 0}

    return Case("decode_single", "decode_single", "ok", make, {"out": (n, u8)}, _decode_run(n, B, E.SINGLE, 0),
                async_form=True, after=_status_after)


def decode_single_fail_case(sync=True):
    """test_k4_decode.test_hostile_single's stream: three blocks, the hostile element in
    block 1; the decoy is a valid stream of three blocks"""
    n = 3 * B

    def make(v):
        m = k4()
        tape, rng = m.Tape(994, 1 << 20), np.random.default_rng(995)
        body = m.hostile_bodies()[HOSTILE if v == 0 else "control"][0]
        s, index, got_n, _ = m.single_hostile(body, tape, rng, False)
        assert got_n == n
        raw = m.oracle_accepts(s, n)
        assert (raw is None) == (v == 0)
        out, care = sent(n), np.ones(n, dtype=bool)
        if raw is None:
            care[:] = False  # (which blocks of a refused stream are written is not promised)
        else:
            out[:] = arr(raw)
        st = E.ERR_OFFSET if v == 0 else 0
        exp = {"out": out, "out#care": care, "rc": st if sync else 0}
        if not sync:
            exp["status"] = st
        return {"comp": arr(s), "offs": np.array(index, dtype=i64)}, exp

    if sync:
        return Case("decode_single/fail", "decode_single", "fail", make, {"out": (n, u8)},
                    _decode_run(n, B, E.SINGLE, 1), shares=("decode_streams", "decode_single"))
    return Case("decode_single/fail_async", "decode_single", "fail", make, {"out": (n, u8)},
                _decode_run(n, B, E.SINGLE, 0), async_form=True, after=_status_after,
                shares=("decode_streams", "decode_single"))


# ---- 5: index ---------------------------------------------------------------------
def index_case(fail):
    """XBLOCK_OPS' streams are over 65,536 bytes long: the chunk-parallel walk.  fail:
    the stream without its last 7 bytes; the decoy is a whole stream of that length"""
    room = 8
    ops = [list(map(list, XBLOCK_OPS[0])), list(map(list, XBLOCK_OPS[1]))]
    if fail:
        ops[1][-1] = ["lit", 13, 34]
    clen = len(build_stream(ops[1]))

    def make(v):
        s = build_stream(ops[v])[:clen]
        st, n, units, ent = k5().k5_serial(s)
        assert (st != 0) == (fail and v == 0) and len(s) == clen
        exp = {"rc": st}
        if st == 0:
            exp.update({"n": n, "offs": image(room, ent, i64)})
        return {"comp": arr(s)}, exp

    def run(codec, d):
        n = ctypes.c_size_t(0)
        rc = lib().snappy_amd_index_device(codec._h, P(d["comp"]), clen, P(d["offs"]), room, ctypes.byref(n))
        return {"rc": rc, "n": n.value}

    return Case("index/fail" if fail else "index", "index", "fail" if fail else "ok", make, {"offs": (room, i64)}, run,
                shares=("index", "frame_index", "container_decode"))


# ---- 6: ranges --------------------------------------------------------------------
def ranges_case(name, kind, n, layout, ranges, out_bytes, want_status=None, seed=120):
    """want_status: the synchronous form with d_status; None: the queued form"""
    count = len(ranges)
    r = np.ascontiguousarray(np.array(ranges, dtype=np.uint64).reshape(-1, 3))
    units = (n + B - 1) // B

    def make(v):
        a = T(n, seed + v)
        if layout == E.STREAMS:
            payload, offs = oracle.compress_streams(a, B)
        else:
            payload, offs = streams_as_single(a)
            payload = arr(payload)
        ok = None if want_status is None else {i for i, s in enumerate(want_status) if s == 0}
        exp = {"out": ranges_image(a.tobytes(), ranges, out_bytes, ok)}
        if want_status is None:
            exp["rc"] = 0
        else:
            exp["rc"] = next((s for s in want_status if s), 0)
            exp["status"] = np.array(want_status, dtype=i32)
        return {"comp": payload, "offs": np.asarray(offs).astype(i64)}, exp

    def run(codec, d):
        # (comp_bytes: the whole buffer, padding included -- both worlds' streams lie inside it)
        return {"rc": lib().snappy_amd_decompress_ranges_device(
            codec._h, P(d["comp"]), 0, d["comp"].numel(), P(d["offs"]), n, B, layout, r.ctypes.data_as(ctypes.c_void_p),
            count, P(d["out"]), out_bytes, P(d.get("status")), 0 if want_status is None else 1)}

    outs = {"out": (out_bytes, u8)}
    if want_status is not None:
        outs["status"] = (count, i32)
    assert units >= 2
    return Case(name, "ranges", kind, make, outs, run, async_form=want_status is None,
                shares=("ranges", "frame_ranges", "container_ranges", "frame_decode", "records_decode"))


RN = 4 * B + 1234
RANGES_SMALL = [(B, 2 * B, 16), (100, 1000, 2 * B + 40), (3 * B - 5, 10, 2 * B + 1100), (RN - 1, 1, 2 * B + 1200),
                (4 * B, 1234, 2 * B + 1300)]
RANGES_SMALL_BYTES = 2 * B + 1300 + 1234 + 9


def ranges_fail():
    """test_ranges.test_batch_with_refused_ranges' two refusals among good ranges"""
    ranges = list(RANGES_SMALL)
    ranges.insert(1, (RN - 5, 6, 0))                          # leaves n
    ranges.insert(3, (100, 50, RANGES_SMALL_BYTES - 49))      # its output leaves out_bytes
    want = [0, E.ERR_ARG, 0, E.ERR_CAPACITY, 0, 0, 0]
    return ranges_case("ranges/fail", "fail", RN, E.SINGLE, ranges, RANGES_SMALL_BYTES, want)


def ranges_large():
    n = 16 << 20
    ranges = [(u * B + 5 + u % 7, 100 + u, 512 * u + u % 16) for u in range(256)]   # 256 edge units
    ranges.append((B, 3 * B, 512 * 256 + 16))
    return ranges_case("ranges/large", "large", n, E.STREAMS, ranges, 512 * 256 + 16 + 3 * B + 7, seed=122)


# ---- 7 .. 9: record batches -------------------------------------------------------
def records_compress_case(name, kind, lens, refused=None):
    """refused: {record: status} -- a record over 65,536 bytes among good ones, as
    test_records.test_refusals has it"""
    refused = refused or {}
    count, total = len(lens), sum(lens)
    descs = packed(lens)
    good = sum(n for i, n in enumerate(lens) if i not in refused)
    cap = E.max_records_output(good, count)

    def make(v):
        a = T(total, 130 + v)
        if not refused and all(n == B for n in lens):
            payload, offs = oracle.compress_streams(a, B)
            payload, offs = payload.tobytes(), [int(x) for x in offs]
        else:
            ss = [b"" if i in refused else oracle.compress(a[o:o + n].tobytes()) for i, (o, n) in enumerate(descs)]
            payload, offs = b"".join(ss), [int(x) for x in np.cumsum([0] + [len(s) for s in ss])]
        st = np.array([refused.get(i, 0) for i in range(count)], dtype=i32)
        return {"base": a, "ol": pairs(descs)}, {"out": image(cap, payload), "offs": np.array(offs, dtype=i64),
                                                 "status": st, "rc": next((int(s) for s in st if s), 0),
                                                 "len": len(payload)}

    def run(codec, d):
        got = ctypes.c_size_t(0)
        rc = lib().snappy_amd_compress_records_device(codec._h, P(d["base"]), total, P(d["ol"]), count, P(d["out"]),
                                                      cap, P(d["offs"]), P(d["status"]), ctypes.byref(got))
        return {"rc": rc, "len": got.value}

    return Case(name, "records_compress", kind, make, {"out": (cap, u8), "offs": (count + 1, i64), "status": (count, i32)},
                run, shares=("records_compress", "long_compress", "compress_streams", "records_decode", "ranges"))


REC_LENS = [[100, 40000, 65536, 3000], [3000, 65536, 100, 40000]]


def _record_streams(v, seed):
    lens = REC_LENS[v]
    a = T(sum(lens), seed + v).tobytes()
    raws = [a[o:o + n] for o, n in packed(lens)]
    return raws, [oracle.compress(r) for r in raws]


def records_length_case():
    def make(v):
        raws, ss = _record_streams(v, 140)
        return {"comp": arr(b"".join(ss)), "ol": pairs(packed(len(s) for s in ss))}, {
            "lens": np.array(REC_LENS[v], dtype=i64), "status": np.zeros(4, dtype=i32), "rc": 0}

    def run(codec, d):
        return {"rc": lib().snappy_amd_records_length_device(codec._h, P(d["comp"]), d["comp"].numel(), P(d["ol"]), 4,
                                                             P(d["lens"]), P(d["status"]))}

    return Case("records_length", "records_length", "ok", make, {"lens": (4, i64), "status": (4, i32)}, run,
                async_form=True)


def records_decode_case(fail):
    """ok: four records into scattered ranges, the queued form with d_status.  fail: the
    hostile 8,192-byte unit between two good ones (test_k4_record_forms), synchronous"""
    if fail:
        lens = [8192] * 3
    gap = 37

    def make(v):
        if fail:
            good, bad, raw = hostile_units()
            ss = [good[0], bad if v == 0 else good[4], good[1]]
            raws = [raw[0], None if v == 0 else raw[4], raw[1]]
            ln = lens
        else:
            raws, ss = _record_streams(v, 150)
            ln = REC_LENS[v]
        o_descs, o = [], 5
        for n in ln:
            o_descs.append((o, n))
            o += n + gap
        out, care = sent(out_bytes), np.ones(out_bytes, dtype=bool)
        for (o, n), r in zip(o_descs, raws):
            if r is None:
                care[o:o + n] = False
            else:
                out[o:o + n] = arr(r)
        st = np.array([0 if r is not None else E.ERR_OFFSET for r in raws], dtype=i32)
        return {"comp": arr(b"".join(ss)), "c_ol": pairs(packed(len(s) for s in ss)), "o_ol": pairs(o_descs)}, {
            "out": out, "out#care": care, "status": st, "rc": next((int(s) for s in st if s), 0) if fail else 0}

    count = 3 if fail else 4
    out_bytes = (3 * 8192 if fail else sum(REC_LENS[0])) + count * gap + 5

    def run(codec, d):
        return {"rc": lib().snappy_amd_decompress_records_device(
            codec._h, P(d["comp"]), d["comp"].numel(), P(d["c_ol"]), count, P(d["out"]), out_bytes, P(d["o_ol"]),
            P(d["status"]), 1 if fail else 0)}

    return Case("records_decode/fail" if fail else "records_decode", "records_decode", "fail" if fail else "ok", make,
                {"out": (out_bytes, u8), "status": (count, i32)}, run, async_form=not fail,
                shares=("records_decode", "records_compress", "ranges", "long_decode"))


# ---- 10 .. 12: long records -------------------------------------------------------
LONG_LENS = [[70000, 150000, 300], [150000, 300, 70000]]


def _long_streams(v, seed):
    import test_long_records as tl
    lens = LONG_LENS[v]
    a = T(sum(lens), seed + v).tobytes()
    raws = [a[o:o + n] for o, n in packed(lens)]
    ss = [oracle.compress(r) for r in raws]
    tables = [e for s, r in zip(ss, raws) for e in tl.walk_table(s, len(r))]
    return raws, ss, tables


def long_compress_case():
    count, total = 3, sum(LONG_LENS[0])
    cap = E.max_long_records_output(total, count)
    icap = E.max_records_index(total, count) + 3

    def make(v):
        raws, ss, tables = _long_streams(v, 160)
        payload = b"".join(ss)
        return {"base": arr(b"".join(raws)), "ol": pairs(packed(LONG_LENS[v]))}, {
            "out": image(cap, payload), "offs": np.cumsum([0] + [len(s) for s in ss]).astype(i64),
            "index": image(icap, tables, i64), "status": np.zeros(count, dtype=i32), "rc": 0, "len": len(payload)}

    def run(codec, d):
        got = ctypes.c_size_t(0)
        rc = lib().snappy_amd_compress_long_records_device(
            codec._h, P(d["base"]), total, P(d["ol"]), count, P(d["out"]), cap, P(d["offs"]), P(d["index"]), icap,
            P(d["status"]), ctypes.byref(got))
        return {"rc": rc, "len": got.value}

    return Case("long_compress", "long_compress", "ok", make,
                {"out": (cap, u8), "offs": (count + 1, i64), "index": (icap, i64), "status": (count, i32)}, run)


def records_index_case():
    count = 3
    icap = E.max_records_index(sum(LONG_LENS[0]), count) + 3

    def make(v):
        raws, ss, tables = _long_streams(v, 170)
        return {"comp": arr(b"".join(ss)), "c_ol": pairs(packed(len(s) for s in ss)),
                "o_ol": pairs(packed(LONG_LENS[v]))}, {
            "index": image(icap, tables, i64), "status": np.zeros(count, dtype=i32), "rc": 0}

    def run(codec, d):
        return {"rc": lib().snappy_amd_records_index_device(codec._h, P(d["comp"]), d["comp"].numel(), P(d["c_ol"]),
                                                            count, P(d["o_ol"]), P(d["index"]), icap, P(d["status"]))}

    return Case("records_index", "records_index", "ok", make, {"index": (icap, i64), "status": (count, i32)}, run)


def long_decode_case(fail):
    """no table passed: the call builds the block tables in scratch.  fail: the hostile
    8,192-byte unit between two long records"""
    count = 3
    lens_of = (lambda v: [70000, 8192, 150000]) if fail else (lambda v: LONG_LENS[v])
    out_bytes = sum(lens_of(0)) + 3 * 21 + 7

    def make(v):
        if fail:
            good, bad, raw = hostile_units()
            a = T(220000, 180 + v).tobytes()
            raws = [a[:70000], None if v == 0 else raw[4], a[70000:]]
            ss = [oracle.compress(raws[0]), bad if v == 0 else good[4], oracle.compress(raws[2])]
        else:
            raws, ss, _ = _long_streams(v, 180)
        o_descs, o = [], 7
        for n in lens_of(v):
            o_descs.append((o, n))
            o += n + 21
        out, care = sent(out_bytes), np.ones(out_bytes, dtype=bool)
        for (o, n), r in zip(o_descs, raws):
            if r is None:
                care[o:o + n] = False
            else:
                out[o:o + n] = arr(r)
        st = np.array([0 if r is not None else E.ERR_OFFSET for r in raws], dtype=i32)
        return {"comp": arr(b"".join(ss)), "c_ol": pairs(packed(len(s) for s in ss)), "o_ol": pairs(o_descs)}, {
            "out": out, "out#care": care, "status": st, "rc": next((int(s) for s in st if s), 0)}

    def run(codec, d):
        return {"rc": lib().snappy_amd_decompress_long_records_device(
            codec._h, P(d["comp"]), d["comp"].numel(), P(d["c_ol"]), count, P(d["out"]), out_bytes, P(d["o_ol"]), None,
            P(d["status"]), 1)}

    return Case("long_decode/fail" if fail else "long_decode", "long_decode", "fail" if fail else "ok", make,
                {"out": (out_bytes, u8), "status": (count, i32)}, run,
                shares=("long_decode", "records_decode", "records_index", "decode_single"))


# ---- 13 .. 17: framing format -----------------------------------------------------
def crc_case():
    descs = [(0, 1), (3, 4096), (5000, 65536), (70001, 777)]

    def make(v):
        a = T(72000, 190 + v)
        want = [fm.mask(fm.crc32c(a[o:o + n].tobytes())) for o, n in descs]
        return {"base": a, "ol": pairs(descs)}, {"crc": np.array(want, dtype=np.uint32).view(i32), "rc": 0}

    def run(codec, d):
        return {"rc": lib().snappy_amd_crc32c_device(codec._h, P(d["base"]), P(d["ol"]), len(descs), 1, P(d["crc"]))}

    return Case("crc32c", "crc32c", "ok", make, {"crc": (len(descs), i32)}, run, async_form=True)


FN = 2 * B + 3000


def frame_compress_case():
    cap, units = E.max_frame_output(FN), 3

    def make(v):
        f = frame_of(T(FN, 200 + v))
        st, table, total = fm.chunk_table(f)
        assert st == fm.OK and total == FN
        return {"x": T(FN, 200 + v)}, {"out": image(cap, f), "chunks": np.array(table, dtype=i64), "rc": 0, "len": len(f)}

    def run(codec, d):
        got = ctypes.c_size_t(0)
        rc = lib().snappy_amd_compress_frame_device(codec._h, P(d["x"]), FN, 0, P(d["out"]), P(d["chunks"]),
                                                    ctypes.byref(got))
        return {"rc": rc, "len": got.value}

    return Case("frame_compress", "frame_compress", "ok", make, {"out": (cap, u8), "chunks": (units + 1, i64)}, run)


@functools.lru_cache(maxsize=None)
def _frames(n0, n1, seed):
    """two framed streams of n0 and n1 bytes made equally long by a closing padding
    chunk; the second has a skippable chunk in it"""
    f0 = frame_of(T(n0, seed))
    f1 = frame_of(T(n1, seed + 1))
    if n1 != n0:
        f1 = f1[:10] + fm.skippable(0x80, b"index: none") + f1[10:]
    return same_length(f0, f1, fm.padding)


def frame_index_case():
    room = 7

    def make(v):
        f = _frames(FN, B + 40000, 210)[v]
        st, table, total = fm.chunk_table(f)
        assert st == fm.OK
        return {"frame": arr(f)}, {"chunks": image(room, table, i64), "rc": 0, "nch": len(table) - 1, "n": total}

    def run(codec, d):
        nch, n = ctypes.c_size_t(0), ctypes.c_size_t(0)
        rc = lib().snappy_amd_frame_index_device(codec._h, P(d["frame"]), len(_frames(FN, B + 40000, 210)[0]),
                                                 P(d["chunks"]), room, ctypes.byref(nch), ctypes.byref(n))
        return {"rc": rc, "nch": nch.value, "n": n.value}

    return Case("frame_index", "frame_index", "ok", make, {"chunks": (room, i64)}, run)


def frame_decode_case(name, kind, n, seed):
    nch = (n + B - 1) // B

    def make(v):
        f = _frames(n, n, seed)[v]
        st, table, total = fm.chunk_table(f)
        assert st == fm.OK and total == n and len(table) == nch + 1
        return {"frame": arr(f), "chunks": np.array(table, dtype=i64)}, {"out": T(n, seed + v), "rc": 0, "len": n}

    def run(codec, d):
        got = ctypes.c_size_t(0)
        rc = lib().snappy_amd_decompress_frame_device(codec._h, P(d["frame"]), len(_frames(n, n, seed)[0]),
                                                      P(d["chunks"]), nch, P(d["out"]), n, ctypes.byref(got))
        return {"rc": rc, "len": got.value}

    return Case(name, "frame_decode", kind, make, {"out": (n, u8)}, run)


def frame_decode_fail_case():
    """test_frame.ERRORS' "bit flipped in a stored CRC"; the decoy is the stream before the flip"""
    def world(v):
        import test_frame as tf
        return (tf.ERRORS["bit flipped in a stored CRC"][0] if v == 0 else tf.GOOD), tf.GOOD_RAW

    def make(v):
        f, raw = world(v)
        st, table, total = fm.chunk_table(f)
        assert st == fm.OK and len(table) == 4
        out, care = image(len(raw) + 16, raw), np.ones(len(raw) + 16, dtype=bool)
        if v == 0:
            care[:len(raw)] = False
        return {"frame": arr(f), "chunks": np.array(table, dtype=i64)}, {
            "out": out, "out#care": care, "rc": E.ERR_CHECKSUM if v == 0 else 0}

    def run(codec, d):
        f, raw = world(0)
        got = ctypes.c_size_t(0)
        return {"rc": lib().snappy_amd_decompress_frame_device(codec._h, P(d["frame"]), len(f), P(d["chunks"]), 3,
                                                               P(d["out"]), len(raw) + 16, ctypes.byref(got))}

    return Case("frame_decode/fail", "frame_decode", "fail", make, {"out": (5500 + 16, u8)}, run,
                shares=("frame_decode", "frame_ranges", "ranges", "frame_compress"))


FRAME_RANGES = [(B, B, 16), (100, 1000, B + 40), (2 * B - 5, 10, B + 1100), (FN - 1, 1, B + 1200), (2 * B, 3000, B + 1300)]
FRAME_RANGES_BYTES = B + 1300 + 3000 + 9


def frame_ranges_case():
    count = len(FRAME_RANGES)
    r = np.ascontiguousarray(np.array(FRAME_RANGES, dtype=np.uint64).reshape(-1, 3))

    def make(v):
        f = _frames(FN, FN, 220)[v]
        chunks, starts = frc.tables(f)
        return {"frame": arr(f), "chunks": np.array(chunks, dtype=i64)}, {
            "starts": np.array(starts, dtype=i64), "out": ranges_image(T(FN, 220 + v).tobytes(), FRAME_RANGES,
                                                                       FRAME_RANGES_BYTES),
            "status": np.zeros(count, dtype=i32), "rc_seek": 0, "n": FN, "rc": 0}

    def run(codec, d):
        flen = len(_frames(FN, FN, 220)[0])
        n = ctypes.c_size_t(0)
        rc_seek = lib().snappy_amd_frame_seek_device(codec._h, P(d["frame"]), flen, P(d["chunks"]), 3, P(d["starts"]),
                                                     ctypes.byref(n))
        rc = lib().snappy_amd_decompress_frame_ranges_device(
            codec._h, P(d["frame"]), 0, flen, P(d["chunks"]), P(d["starts"]), 3, r.ctypes.data_as(ctypes.c_void_p), count,
            P(d["out"]), FRAME_RANGES_BYTES, P(d["status"]))
        return {"rc_seek": rc_seek, "n": n.value, "rc": rc}

    return Case("frame_ranges", "frame_ranges", "ok", make,
                {"starts": (4, i64), "out": (FRAME_RANGES_BYTES, u8), "status": (count, i32)}, run)


# ---- 18 .. 20: containers ---------------------------------------------------------
CN, CBLOCK = 3 * 32768 + 500, 32768


def container_compress_case(fmt, name):
    chunks = 4
    cap = E.max_container_output(CN, CBLOCK, fmt)

    def make(v):
        a = T(CN, 230 + v).tobytes()
        pieces = [a[o:o + CBLOCK] for o in range(0, CN, CBLOCK)]
        cont = cm.wrap(pieces, [oracle.compress(p) for p in pieces], fmt)
        st, comp, outp, total = cm.walk(cont, fmt)
        assert st == cm.OK and total == CN and len(comp) == chunks
        return {"x": arr(a)}, {"out": image(cap, cont), "comp": pairs(comp), "outp": pairs(outp), "rc": 0,
                               "nch": chunks, "len": len(cont)}

    def run(codec, d):
        nch, got = ctypes.c_size_t(0), ctypes.c_size_t(0)
        rc = lib().snappy_amd_compress_container_device(codec._h, P(d["x"]), CN, CBLOCK, fmt, 0, P(d["out"]), cap,
                                                        P(d["comp"]), P(d["outp"]), chunks, ctypes.byref(nch),
                                                        ctypes.byref(got))
        return {"rc": rc, "nch": nch.value, "len": got.value}

    return Case(name, "container_compress", "ok", make, {"out": (cap, u8), "comp": (2 * chunks, i64),
                                                         "outp": (2 * chunks, i64)}, run)


def _stored_container(fmt, sizes, seed):
    raws = [cc.content(n, seed + i) for i, n in enumerate(sizes)]
    return cm.wrap(raws, [cc.stored(r) for r in raws], fmt), b"".join(raws)


def container_decode_case(name, kind, fmt, sizes2):
    """the device walk, then the decode with its tables.  Literal-only payloads: the two
    worlds hold the same chunk sizes in another order, so they are equally long"""
    chunks = len(sizes2[0])
    total = sum(sizes2[0])
    clen = len(_stored_container(fmt, sizes2[0], 1)[0])

    def make(v):
        cont, raw = _stored_container(fmt, sizes2[v], 240 + 10 * v)
        st, comp, outp, n = cm.walk(cont, fmt)
        assert st == cm.OK and n == total and len(cont) == clen
        return {"cont": arr(cont)}, {"comp": image(2 * chunks + 2, pairs(comp), i64),
                                     "outp": image(2 * chunks + 2, pairs(outp), i64), "out": arr(raw), "rc_index": 0,
                                     "nch": chunks, "n": total, "rc": 0, "len": total}

    def run(codec, d):
        nch, n, got = ctypes.c_size_t(0), ctypes.c_size_t(0), ctypes.c_size_t(0)
        rc_index = lib().snappy_amd_container_index_device(codec._h, P(d["cont"]), clen, fmt, P(d["comp"]), P(d["outp"]),
                                                           chunks + 1, ctypes.byref(nch), ctypes.byref(n))
        rc = lib().snappy_amd_decompress_container_device(codec._h, P(d["cont"]), clen, fmt, P(d["comp"]), P(d["outp"]),
                                                          nch.value, P(d["out"]), total, ctypes.byref(got))
        return {"rc_index": rc_index, "nch": nch.value, "n": n.value, "rc": rc, "len": got.value}

    return Case(name, "container_decode", kind, make, {"comp": (2 * chunks + 2, i64), "outp": (2 * chunks + 2, i64),
                                                       "out": (total, u8)}, run)


def container_decode_fail_case():
    """test_container.test_precedence_and_element_errors' cut literal in a Hadoop block,
    decoded without tables; the decoy is a valid block of the same length"""
    cap = 600

    def bad():
        p = [cc.content(200, 21), cc.content(200, 22), cc.content(200, 23)]
        cut_literal = cm.varint(200) + bytes([60 << 2, 199])
        far_copy = cm.varint(200) + bytes([3 << 2]) + b"abcd" + bytes([0x01, 5])
        return cm.hadoop_block(600, [cc.stored(p[0]), cut_literal, far_copy])

    def good():
        want = len(bad())
        for k in range(1, want):
            raw = cc.content(k, 24)
            c = cm.hadoop_block(k, [cc.stored(raw)])
            if len(c) == want:
                return c, raw
        raise AssertionError("no valid block of that length")

    def make(v):
        if v == 0:
            out, care = sent(cap), np.zeros(cap, dtype=bool)
            return {"cont": arr(bad())}, {"out": out, "out#care": care, "rc": E.ERR_TRUNCATED}
        c, raw = good()
        return {"cont": arr(c)}, {"out": image(cap, raw), "rc": 0}

    def run(codec, d):
        got = ctypes.c_size_t(0)
        return {"rc": lib().snappy_amd_decompress_container_device(codec._h, P(d["cont"]), len(bad()), cm.HADOOP, None,
                                                                   None, 0, P(d["out"]), cap, ctypes.byref(got))}

    return Case("container_decode/fail", "container_decode", "fail", make, {"out": (cap, u8)}, run,
                shares=("container_decode", "container_ranges", "frame_decode", "index"))


CR_SIZES = [[70000, 140000, 30000], [140000, 70000, 30000]]
CR_N = 240000
CR_RANGES = [(0, 70000, 16), (100, 1000, 70040), (69990, 20, 71100), (CR_N - 1, 1, 71200), (210000, 30000, 71300)]
CR_BYTES = 71300 + 30000 + 9


def container_ranges_case():
    fmt, count = cm.XERIAL, len(CR_RANGES)
    r = np.ascontiguousarray(np.array(CR_RANGES, dtype=np.uint64).reshape(-1, 3))
    clen = len(_stored_container(fmt, CR_SIZES[0], 1)[0])

    def make(v):
        cont, raw = _stored_container(fmt, CR_SIZES[v], 260 + 10 * v)
        st, comp, outp, n = cm.walk(cont, fmt)
        assert st == cm.OK and n == CR_N and len(cont) == clen
        return {"cont": arr(cont), "comp": pairs(comp), "outp": pairs(outp)}, {
            "out": ranges_image(raw, CR_RANGES, CR_BYTES), "status": np.zeros(count, dtype=i32), "rc": 0}

    def run(codec, d):
        return {"rc": lib().snappy_amd_decompress_container_ranges_device(
            codec._h, P(d["cont"]), 0, clen, P(d["comp"]), P(d["outp"]), 3, r.ctypes.data_as(ctypes.c_void_p), count,
            P(d["out"]), CR_BYTES, P(d["status"]))}

    return Case("container_ranges", "container_ranges", "ok", make, {"out": (CR_BYTES, u8), "status": (count, i32)}, run)


# ---- the catalogue ----------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def catalogue():
    """every case, in the order of the families in the header"""
    big = [[B] * 256, [B] * 256]
    cases = [
        compress_case("compress_streams", "compress_streams", "ok", 3 * 32768 + 1000, 32768, E.STREAMS),
        compress_case("compress_streams/large", "compress_streams", "large", 16 << 20, 32768, E.STREAMS),
        compress_case("compress_single", "compress_single", "ok", B + 40000, B, E.SINGLE),
        decode_streams_case(), decode_streams_fail_case(), decode_streams_fail_case(sync=False),
        decode_single_case(), decode_single_fail_case(), decode_single_fail_case(sync=False),
        index_case(False), index_case(True),
        ranges_case("ranges", "ok", RN, E.SINGLE, RANGES_SMALL, RANGES_SMALL_BYTES), ranges_fail(), ranges_large(),
        records_compress_case("records_compress", "ok", REC_LENS[0]),
        records_compress_case("records_compress/fail", "fail", [300, 65537, 2000], {1: E.ERR_UNSUPPORTED}),
        records_compress_case("records_compress/large", "large", [B] * 256),
        records_length_case(), records_decode_case(False), records_decode_case(True),
        long_compress_case(), records_index_case(), long_decode_case(False), long_decode_case(True),
        crc_case(), frame_compress_case(), frame_index_case(),
        frame_decode_case("frame_decode", "ok", FN, 270), frame_decode_fail_case(),
        frame_decode_case("frame_decode/large", "large", 16 << 20, 272),
        frame_ranges_case(),
        container_compress_case(cm.HADOOP, "container_compress/hadoop"),
        container_compress_case(cm.XERIAL, "container_compress/xerial"),
        container_decode_case("container_decode/hadoop", "ok", cm.HADOOP, [[1000, 3000, 2000], [3000, 1000, 2000]]),
        container_decode_case("container_decode/xerial", "ok", cm.XERIAL, [[40000, 300, 65536], [300, 65536, 40000]]),
        container_decode_fail_case(),
        container_decode_case("container_decode/large", "large", cm.XERIAL, big),
        container_ranges_case(),
    ]
    assert len({c.name for c in cases}) == len(cases)
    return cases


FAMILIES = ["compress_streams", "compress_single", "decode_streams", "decode_single", "index", "ranges",
            "records_compress", "records_length", "records_decode", "long_compress", "records_index", "long_decode",
            "crc32c", "frame_compress", "frame_index", "frame_decode", "frame_ranges", "container_compress",
            "container_decode", "container_ranges"]


# the names of catalogue()'s cases, written out so that a test module can parametrise over
# them without building the catalogue (which needs the built library) while it is collected
NAMES = ["compress_streams", "compress_streams/large", "compress_single", "decode_streams", "decode_streams/fail",
         "decode_streams/fail_async", "decode_single", "decode_single/fail", "decode_single/fail_async", "index",
         "index/fail", "ranges", "ranges/fail", "ranges/large", "records_compress", "records_compress/fail",
         "records_compress/large", "records_length", "records_decode", "records_decode/fail", "long_compress",
         "records_index", "long_decode", "long_decode/fail", "crc32c", "frame_compress", "frame_index", "frame_decode",
         "frame_decode/fail", "frame_decode/large", "frame_ranges", "container_compress/hadoop",
         "container_compress/xerial", "container_decode/hadoop", "container_decode/xerial", "container_decode/fail",
         "container_decode/large", "container_ranges"]
ASYNC_NAMES = ["compress_streams", "compress_streams/large", "compress_single", "decode_streams",
               "decode_streams/fail_async", "decode_single", "decode_single/fail_async", "ranges", "ranges/large",
               "records_length", "records_decode", "crc32c"]


def by_name(name):
    return next(c for c in catalogue() if c.name == name)


def small_of(family):
    """the family's first successful small case"""
    return next(c for c in catalogue() if c.family == family and c.kind == "ok")


# ---- running a case on the device (imports torch only when called) -----------------
class Buffers:
    """the device tensors of one case: both worlds' inputs, the working inputs and the
    outputs, allocated on the current stream; fill() (re)writes the sentinel"""

    def __init__(self, case, device="cuda"):
        import torch
        self.case = case
        self.src = {k: torch.from_numpy(v).to(device) for k, v in case.inputs().items()}
        self.alt = {k: torch.from_numpy(v).to(device) for k, v in case.decoy().items()}
        self.dev = {k: torch.empty_like(v) for k, v in self.src.items()}
        self.out = {}
        for k, (n, dtype) in case.outputs().items():
            self.out[k] = torch.empty(n * np.dtype(dtype).itemsize, dtype=torch.uint8, device=device)
            self.dev[k] = self.out[k].view({u8: torch.uint8, i32: torch.int32, i64: torch.int64}[dtype])
        self.fill()

    def fill(self):
        for t in self.out.values():
            t.fill_(SENT)

    def load(self, world):
        for k, v in world.items():
            self.dev[k].copy_(v, non_blocking=True)

    def read(self):
        return {k: self.dev[k].cpu().numpy() for k in self.out}


def run_plain(codec, case, decoy=False, buffers=None):
    """the case on the current stream, compared with its expectation -> (outs, res)"""
    b = buffers or Buffers(case)
    b.fill()
    b.load(b.alt if decoy else b.src)
    res = case.run(codec, b.dev)
    import torch
    torch.cuda.current_stream().synchronize()
    res.update(case.after(codec))
    outs = b.read()
    compare(case, case.expect_decoy() if decoy else case.expect(), outs, res)
    return outs, res

#!/usr/bin/env python3
"""Record-batch timings on one GPU (the protocol of tools/frame_bench.py): N
bytes of datagen text in HBM, HIP events on the codec's stream, medians of
`reps` repetitions after two warm-up rounds, all calls alternating in the same
process.  Compress and decode each:

  a  uniform 32,768-byte records   vs  the STREAMS call, chunk 32,768
  b  uniform 65,536-byte records   vs  the STREAMS call, chunk 65,536
  c  a seeded log-uniform mix of 64 B .. 64 KiB records, N bytes in all
  d  4 KiB records

and the long-record calls:

  e  1 MiB records                 \
  f  256 KiB records                >  vs  the SINGLE call on the same N bytes
  g  a seeded log-uniform mix of 64 B .. 4 MiB records  /

and the container calls, each format at its default block:

  h  Hadoop SnappyCodec, 131,072-byte pieces       \  vs  the long-record calls on the
  x  snappy-java SnappyOutputStream, 32,768-byte    /  same pieces / the same chunks

The STREAMS calls are the yardstick of a and b (their min..max is the spread a
difference has to exceed); c and d have no fixed-layout counterpart.  The
yardstick of e, f and g is the SINGLE call in the same round: its compress for the
long compress, its decode for the long decode with compress's tables, and
snappy_amd_index_device + its decode for the long decode that builds the tables
(NULL).  The walk a NULL decode adds is also reported per record and per GiB.
The yardsticks of h and x, in the same round: compress_long_records_device on the
same pieces (no block tables asked for, as the container call asks for none) for
the container compress; decompress_long_records_device with NULL block tables on
the container's own chunk tables for the container decode with tables given.
container_index_device alone is reported per chunk.

and range decode, leg r, on the SINGLE stream of the N bytes:

  r_range_whole   one range [1, N - 1)                       \  vs  the SINGLE decode of the
  r_range_1mib    one 1 MiB range at an unaligned start      /  same stream in the same round
  r_range_16k_4k  16,384 ranges of 4,096 bytes at seeded random starts: the time and the
                  bytes decoded per byte delivered (no yardstick)

Every range's out_offset agrees with its start mod 16 (16-byte stores, as the whole
decode writes).

Prints one JSON line and writes it to profiles/<tag>.json when a tag is given:
    python tools/records_bench.py [n_bytes] [reps] [tag] [legs, default abcdefg; hx and r on request]
Run under rocprofv3 --kernel-trace --stats (a run of its own) for per-kernel times."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "lightweight-snappy_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import datagen  # noqa: E402
import snappy_amd  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 1 << 30
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 11
tag = sys.argv[3] if len(sys.argv) > 3 else ""
which = sys.argv[4] if len(sys.argv) > 4 else "abcdefg"
LONG = "efg"
CONTAINER = {"h": snappy_amd.CONTAINER_HADOOP, "x": snappy_amd.CONTAINER_XERIAL}

host = np.empty(n, dtype=np.uint8)
datagen.fill(host, "T", 1234, threads=16)
x = torch.from_numpy(host).cuda()
del host
codec = snappy_amd.Codec(0)
stream = torch.cuda.Stream()
codec.set_stream(stream.cuda_stream)
lib, h, vp, ct = snappy_amd.lib(), codec._h, snappy_amd.ctypes.c_void_p, snappy_amd.ctypes


def uniform(ln):
    offs = np.arange(0, n, ln, dtype=np.int64)
    return np.stack([offs, np.minimum(ln, n - offs)], axis=1)


def log_uniform(seed=1234, hi=65536):
    rng = np.random.default_rng(seed)
    lens = np.exp(rng.uniform(np.log(64), np.log(hi), size=n // 64 + 1)).astype(np.int64)
    ends = np.cumsum(lens)
    k = int(np.searchsorted(ends, n)) + 1
    lens = lens[:k]
    lens[-1] -= ends[k - 1] - n  # the last record ends the buffer
    return np.stack([np.concatenate(([0], ends[:k - 1])), lens], axis=1)


legs = {"a": uniform(32768), "b": uniform(65536), "c": log_uniform(), "d": uniform(4096),
        "e": uniform(1 << 20), "f": uniform(256 << 10), "g": log_uniform(4321, 4 << 20),
        "h": uniform(snappy_amd.CONTAINER_BLOCK[snappy_amd.CONTAINER_HADOOP]),
        "x": uniform(snappy_amd.CONTAINER_BLOCK[snappy_amd.CONTAINER_XERIAL])}
legs = {k: v[v[:, 1] > 0] for k, v in legs.items() if k in which}
max_count = max([len(v) for v in legs.values()] + [1])
out = torch.empty(max(snappy_amd.max_records_output(n, max_count), snappy_amd.max_long_records_output(n, max_count),
                      codec.max_output(n, snappy_amd.BLOCK, snappy_amd.SINGLE)), dtype=torch.uint8, device="cuda")
back = torch.empty(n, dtype=torch.uint8, device="cuda")
dev = {}
for k, v in legs.items():
    dev[k] = {"ol": torch.from_numpy(v.reshape(-1).copy()).cuda(), "count": len(v),
              "offs": torch.empty(len(v) + 1, dtype=torch.int64, device="cuda"),
              "col": torch.empty(2 * len(v), dtype=torch.int64, device="cuda"), "clen": 0}
    if k in LONG:
        dev[k]["index"] = torch.empty(snappy_amd.max_records_index(n, len(v)), dtype=torch.int64, device="cuda")
    if k in CONTAINER:
        dev[k]["comp"] = torch.empty(2 * len(v), dtype=torch.int64, device="cuda")
        dev[k]["outp"] = torch.empty(2 * len(v), dtype=torch.int64, device="cuda")
        dev[k]["cont_len"] = 0
cont = torch.empty(max([snappy_amd.max_container_output(n, 0, f) for k, f in CONTAINER.items() if k in legs] + [1]),
                   dtype=torch.uint8, device="cuda")
units = (n + snappy_amd.BLOCK - 1) // snappy_amd.BLOCK
state = {"single_offs": torch.empty(units + 1, dtype=torch.int64, device="cuda"),
         "single_index": torch.empty(units + 1, dtype=torch.int64, device="cuda")}


def compress_records(k):
    d = dev[k]
    got = ct.c_size_t(0)
    snappy_amd._check(lib.snappy_amd_compress_records_device(h, vp(x.data_ptr()), n, vp(d["ol"].data_ptr()), d["count"],
                                                             vp(out.data_ptr()), out.numel(), vp(d["offs"].data_ptr()),
                                                             None, ct.byref(got)), "compress_records_device")
    d["clen"] = got.value


def decode_records(k):
    d = dev[k]
    snappy_amd._check(lib.snappy_amd_decompress_records_device(h, vp(out.data_ptr()), d["clen"], vp(d["col"].data_ptr()),
                                                               d["count"], vp(back.data_ptr()), n, vp(d["ol"].data_ptr()),
                                                               None, 1), "decompress_records_device")


def compress_long(k):
    d = dev[k]
    got = ct.c_size_t(0)
    snappy_amd._check(lib.snappy_amd_compress_long_records_device(
        h, vp(x.data_ptr()), n, vp(d["ol"].data_ptr()), d["count"], vp(out.data_ptr()), out.numel(),
        vp(d["offs"].data_ptr()), vp(d["index"].data_ptr()), d["index"].numel(), None, ct.byref(got)),
        "compress_long_records_device")
    d["clen"] = got.value


def decode_long(k, with_table):
    d = dev[k]
    snappy_amd._check(lib.snappy_amd_decompress_long_records_device(
        h, vp(out.data_ptr()), d["clen"], vp(d["col"].data_ptr()), d["count"], vp(back.data_ptr()), n,
        vp(d["ol"].data_ptr()), vp(d["index"].data_ptr()) if with_table else None, None, 1),
        "decompress_long_records_device")


def compress_container(k):
    d = dev[k]
    nch, got = ct.c_size_t(0), ct.c_size_t(0)
    snappy_amd._check(lib.snappy_amd_compress_container_device(
        h, vp(x.data_ptr()), n, 0, CONTAINER[k], 0, vp(cont.data_ptr()), cont.numel(), vp(d["comp"].data_ptr()),
        vp(d["outp"].data_ptr()), d["count"], ct.byref(nch), ct.byref(got)), "compress_container_device")
    assert nch.value == d["count"]
    d["cont_len"] = got.value


def compress_long_pieces(k):
    d = dev[k]
    got = ct.c_size_t(0)
    snappy_amd._check(lib.snappy_amd_compress_long_records_device(
        h, vp(x.data_ptr()), n, vp(d["ol"].data_ptr()), d["count"], vp(out.data_ptr()), out.numel(),
        vp(d["offs"].data_ptr()), None, 0, None, ct.byref(got)), "compress_long_records_device")
    d["clen"] = got.value


def decode_container(k):
    d = dev[k]
    got = ct.c_size_t(0)
    snappy_amd._check(lib.snappy_amd_decompress_container_device(
        h, vp(cont.data_ptr()), d["cont_len"], CONTAINER[k], vp(d["comp"].data_ptr()), vp(d["outp"].data_ptr()),
        d["count"], vp(back.data_ptr()), n, ct.byref(got)), "decompress_container_device")
    assert got.value == n


def decode_long_chunks(k):
    d = dev[k]
    snappy_amd._check(lib.snappy_amd_decompress_long_records_device(
        h, vp(cont.data_ptr()), d["cont_len"], vp(d["comp"].data_ptr()), d["count"], vp(back.data_ptr()), n,
        vp(d["outp"].data_ptr()), None, None, 1), "decompress_long_records_device")


def index_container(k):
    d = dev[k]
    nch, got = ct.c_size_t(0), ct.c_size_t(0)
    snappy_amd._check(lib.snappy_amd_container_index_device(
        h, vp(cont.data_ptr()), d["cont_len"], CONTAINER[k], vp(d["icomp"].data_ptr()), vp(d["ioutp"].data_ptr()),
        d["count"], ct.byref(nch), ct.byref(got)), "container_index_device")
    assert (nch.value, got.value) == (d["count"], n)


def container_round(k, r):
    """one round of a container leg and of its yardsticks -> {name: ms}"""
    d = dev[k]
    if "icomp" not in d:
        d["icomp"], d["ioutp"] = torch.empty_like(d["comp"]), torch.empty_like(d["outp"])
    t = {"compress_container": timed(compress_container, k), "compress_long": timed(compress_long_pieces, k)}
    for name, fn in (("decode_container_table", decode_container), ("decode_long_null", decode_long_chunks)):
        if r == 1:
            back.zero_()
        t[name] = timed(fn, k)
        if r == 1:
            assert torch.equal(back, x), f"leg {k}: {name} round trip failed"
    t["index_container"] = timed(index_container, k)
    if r == 1:
        assert torch.equal(d["icomp"], d["comp"]) and torch.equal(d["ioutp"], d["outp"])
        # the container is the long-record payload with a header in front of every record
        hdr = 8 if k == "h" else 4
        assert d["cont_len"] == d["clen"] + hdr * d["count"] + (16 if k == "x" else 0)
    return t


def compress_single():
    state["slen"] = codec.compress_ptr(x.data_ptr(), n, snappy_amd.BLOCK, snappy_amd.SINGLE, out.data_ptr(),
                                       state["single_offs"].data_ptr())


def decode_single():
    codec.decompress_ptr(out.data_ptr(), state["single_offs"].data_ptr(), n, snappy_amd.BLOCK, snappy_amd.SINGLE,
                         back.data_ptr())


def index_single():
    codec.index_ptr(out.data_ptr(), state["slen"], state["single_index"].data_ptr(), units + 1)


def long_round(k, r):
    """one round of a long-record leg and of its yardsticks -> {name: ms}"""
    d = dev[k]
    t = {"compress_long": timed(compress_long, k)}
    o = d["offs"]
    d["col"].copy_(torch.stack([o[:-1], o[1:] - o[:-1]], dim=1).reshape(-1))
    for name, with_table in (("decode_long_table", True), ("decode_long_null", False)):
        if r == 1:
            back.zero_()
        t[name] = timed(decode_long, k, with_table)
        if r == 1:
            assert torch.equal(back, x), f"leg {k}: {name} round trip failed"
    t["compress_single"] = timed(compress_single)
    t["decode_single"] = timed(decode_single)
    t["index_single"] = timed(index_single)
    if r == 1:
        assert torch.equal(state["single_index"], state["single_offs"])
    return t


def range_sets():
    rng = np.random.default_rng(2468)
    starts = rng.integers(0, n - 4096, 16384)
    many = np.stack([starts, np.full(16384, 4096), np.arange(16384) * 4112 + starts % 16], axis=1).astype(np.uint64)
    one = min(300 * (1 << 20) + 12345, n // 3 + 1)
    ln = min(1 << 20, n - one)
    touched = int(((starts + 4095) // snappy_amd.BLOCK - starts // snappy_amd.BLOCK + 1).sum())
    return {"range_whole": np.array([[1, n - 2, 1]], dtype=np.uint64),
            "range_1mib": np.array([[one, ln, one % 16]], dtype=np.uint64), "range_16k_4k": many}, touched


def decode_ranges(ranges):
    codec.decompress_ranges_tensor(out[: state["slen"]], state["single_offs"], n, ranges, out=back)
    assert codec.last_ranges_status == 0


def range_round(r):
    """one round of the range legs and of their yardstick, the SINGLE decode -> {name: ms}"""
    if "ranges" not in state:
        state["ranges"], state["touched"] = range_sets()
        compress_single()
    t = {"decode_single": timed(decode_single)}
    for name, ranges in state["ranges"].items():
        if r == 1:
            back.zero_()
        t[name] = timed(decode_ranges, ranges)
        if r == 1:
            for a, ln, oo in ranges[:: max(1, len(ranges) // 64)].tolist():
                assert torch.equal(back[oo:oo + ln], x[a:a + ln]), f"leg r: {name} differs"
    return t


def compress_streams(chunk):
    state["plen"] = codec.compress_ptr(x.data_ptr(), n, chunk, snappy_amd.STREAMS, out.data_ptr(), state["soffs"].data_ptr())


def decode_streams(chunk):
    codec.decompress_ptr(out.data_ptr(), state["soffs"].data_ptr(), n, chunk, snappy_amd.STREAMS, back.data_ptr())


def timed(fn, *args):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    fn(*args)
    b.record(stream)
    b.synchronize()
    return a.elapsed_time(b)


def median(v):
    return sorted(v)[len(v) // 2]


ms = {}
with torch.cuda.stream(stream):
    for r in range(reps + 2):  # two warm-up rounds (code objects, scratch growth)
        if "r" in which:
            t = range_round(r)
            if r >= 2:
                for name, v in t.items():
                    ms.setdefault(f"r_{name}", []).append(v)
        for k in legs:
            if k in LONG or k in CONTAINER:
                t = long_round(k, r) if k in LONG else container_round(k, r)
                if r >= 2:
                    for name, v in t.items():
                        ms.setdefault(f"{k}_{name}", []).append(v)
                continue
            d = dev[k]
            chunk = {"a": 32768, "b": 65536}.get(k)
            t = {"compress_records": timed(compress_records, k)}
            # the compressed records' (offset, length) pairs, on the device (not timed)
            o = d["offs"]
            d["col"].copy_(torch.stack([o[:-1], o[1:] - o[:-1]], dim=1).reshape(-1))
            if r == 1:
                state[k + "_payload"] = out[: d["clen"]].clone() if chunk else None
            if r == 1:
                back.zero_()
            t["decode_records"] = timed(decode_records, k)
            if r == 1:
                assert torch.equal(back, x), f"leg {k}: record round trip failed"
            if chunk:
                state["soffs"] = torch.empty(d["count"] + 1, dtype=torch.int64, device="cuda")
                t["compress_streams"] = timed(compress_streams, chunk)
                if r == 1:
                    assert state["plen"] == d["clen"] and torch.equal(out[: d["clen"]], state[k + "_payload"]), \
                        f"leg {k}: records != STREAMS"
                    assert torch.equal(state["soffs"], o)
                    state[k + "_payload"] = None
                t["decode_streams"] = timed(decode_streams, chunk)
            if r >= 2:
                for name, v in t.items():
                    ms.setdefault(f"{k}_{name}", []).append(v)
stream.synchronize()
held = codec.device_bytes()
codec.close()
med = {k: median(v) for k, v in ms.items()}
res = {"n": n, "reps": reps, "records": {k: dev[k]["count"] for k in legs},
       "compressed_bytes": {k: dev[k]["clen"] for k in legs},
       "container_bytes": {k: dev[k]["cont_len"] for k in legs if k in CONTAINER}, "device_bytes": held, "median_ms": med,
       "min_max_ms": {k: [min(v), max(v)] for k, v in ms.items()}}
for k in legs:
    if k in "ab":
        res[f"{k}_compress_ratio"] = med[f"{k}_compress_records"] / med[f"{k}_compress_streams"]
        res[f"{k}_decode_ratio"] = med[f"{k}_decode_records"] / med[f"{k}_decode_streams"]
    if k in LONG:
        res[f"{k}_compress_ratio"] = med[f"{k}_compress_long"] / med[f"{k}_compress_single"]
        res[f"{k}_decode_table_ratio"] = med[f"{k}_decode_long_table"] / med[f"{k}_decode_single"]
        res[f"{k}_decode_null_ratio"] = med[f"{k}_decode_long_null"] / (med[f"{k}_index_single"] + med[f"{k}_decode_single"])
        # what building the tables adds to a decode: per record and per GiB
        walk = med[f"{k}_decode_long_null"] - med[f"{k}_decode_long_table"]
        res[f"{k}_null_walk_us_per_record"] = 1e3 * walk / dev[k]["count"]
        res[f"{k}_null_walk_ms_per_gib"] = walk * (1 << 30) / n
    if k in CONTAINER:
        res[f"{k}_compress_ratio"] = med[f"{k}_compress_container"] / med[f"{k}_compress_long"]
        res[f"{k}_compress_extra_ms"] = med[f"{k}_compress_container"] - med[f"{k}_compress_long"]
        res[f"{k}_decode_table_ratio"] = med[f"{k}_decode_container_table"] / med[f"{k}_decode_long_null"]
        res[f"{k}_decode_table_extra_ms"] = med[f"{k}_decode_container_table"] - med[f"{k}_decode_long_null"]
        res[f"{k}_index_us_per_chunk"] = 1e3 * med[f"{k}_index_container"] / dev[k]["count"]
if "r" in which:
    for name in ("range_whole", "range_1mib"):
        res[f"r_{name}_minus_single_ms"] = med[f"r_{name}"] - med["r_decode_single"]
    res["r_range_whole_ratio"] = med["r_range_whole"] / med["r_decode_single"]
    res["r_16k_4k_decoded_per_delivered"] = state["touched"] * snappy_amd.BLOCK / (16384 * 4096)
line = json.dumps(res)
print(line)
if tag:
    with open(os.path.join(ROOT, "profiles", tag + ".json"), "w") as f:
        f.write(line + "\n")

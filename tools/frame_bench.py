#!/usr/bin/env python3
"""Framing-format timings on one GPU: N bytes of datagen text in HBM, HIP
events on the codec's stream, medians of `reps` repetitions after a warm-up,
framed and unframed calls alternating in the same process.

  a  KF1 alone (CRC-32C of every 65,536-byte piece), GB/s
  b  compress_frame_device   vs  compress_device(STREAMS, 65536)
  c  decompress_frame_device (table given)  vs  decompress_device(STREAMS, 65536)
  d  frame_index_device, microseconds per chunk

Prints one JSON line and writes it to profiles/<tag>.json when a tag is given:
    python tools/frame_bench.py [n_bytes] [reps] [tag]
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
CH = 65536
units = (n + CH - 1) // CH

host = np.empty(n, dtype=np.uint8)
datagen.fill(host, "T", 1234, threads=16)
x = torch.from_numpy(host).cuda()
del host
codec = snappy_amd.Codec(0)
stream = torch.cuda.Stream()
codec.set_stream(stream.cuda_stream)

framed = torch.empty(snappy_amd.max_frame_output(n), dtype=torch.uint8, device="cuda")
chunks = torch.empty(units + 1, dtype=torch.int64, device="cuda")
plain = torch.empty(codec.max_output(n, CH, snappy_amd.STREAMS), dtype=torch.uint8, device="cuda")
offs = torch.empty(units + 1, dtype=torch.int64, device="cuda")
back = torch.empty(n, dtype=torch.uint8, device="cuda")
table = torch.empty(units + 2, dtype=torch.int64, device="cuda")
ol = torch.stack([torch.arange(units, dtype=torch.int64) * CH,
                  torch.tensor([min(CH, n - u * CH) for u in range(units)], dtype=torch.int64)], dim=1).cuda().contiguous()
crcs = torch.empty(units, dtype=torch.int32, device="cuda")
lib, h, vp = snappy_amd.lib(), codec._h, snappy_amd.ctypes.c_void_p
state = {}


def kf1():
    snappy_amd._check(lib.snappy_amd_crc32c_device(h, vp(x.data_ptr()), vp(ol.data_ptr()), units, 1, vp(crcs.data_ptr())),
                      "crc32c_device")


def compress_framed():
    state["flen"] = codec.compress_frame_ptr(x.data_ptr(), n, 0, framed.data_ptr(), chunks.data_ptr())


def compress_plain():
    state["plen"] = codec.compress_ptr(x.data_ptr(), n, CH, snappy_amd.STREAMS, plain.data_ptr(), offs.data_ptr())


def decode_framed():
    got = snappy_amd.ctypes.c_size_t(0)
    snappy_amd._check(lib.snappy_amd_decompress_frame_device(h, vp(framed.data_ptr()), state["flen"],
                                                             vp(chunks.data_ptr()), units, vp(back.data_ptr()), n,
                                                             snappy_amd.ctypes.byref(got)), "decompress_frame_device")
    assert got.value == n


def decode_plain():
    codec.decompress_ptr(plain.data_ptr(), offs.data_ptr(), n, CH, snappy_amd.STREAMS, back.data_ptr())


def index_framed():
    nch, tot = snappy_amd.ctypes.c_size_t(0), snappy_amd.ctypes.c_size_t(0)
    snappy_amd._check(lib.snappy_amd_frame_index_device(h, vp(framed.data_ptr()), state["flen"], vp(table.data_ptr()),
                                                        units + 2, snappy_amd.ctypes.byref(nch),
                                                        snappy_amd.ctypes.byref(tot)), "frame_index_device")
    assert (nch.value, tot.value) == (units, n)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    fn()
    b.record(stream)
    b.synchronize()
    return a.elapsed_time(b)


def median(v):
    return sorted(v)[len(v) // 2]


ms = {k: [] for k in ("kf1", "compress_framed", "compress_plain", "decode_framed", "decode_plain", "index_framed")}
with torch.cuda.stream(stream):
    for r in range(reps + 2):  # two warm-up rounds (code objects, scratch growth)
        for name, fn in (("kf1", kf1), ("compress_framed", compress_framed), ("compress_plain", compress_plain),
                         ("decode_framed", decode_framed), ("decode_plain", decode_plain),
                         ("index_framed", index_framed)):
            t = timed(fn)
            if r >= 2:
                ms[name].append(t)
        if r == 1:  # results, once: round trip and the two tables agree
            assert torch.equal(back, x), "round trip failed"
            assert torch.equal(table[: units + 1], chunks), "device walk != compressor's table"
stream.synchronize()
codec.close()
med = {k: median(v) for k, v in ms.items()}
res = {
    "n": n, "reps": reps, "chunks": units, "framed_bytes": state["flen"], "unframed_bytes": state["plen"],
    "a_kf1_ms": med["kf1"], "a_kf1_GBps": n / (med["kf1"] * 1e-3) / 1e9,
    "b_compress_frame_ms": med["compress_framed"], "b_compress_streams_ms": med["compress_plain"],
    "b_ratio": med["compress_framed"] / med["compress_plain"],
    "c_decompress_frame_ms": med["decode_framed"], "c_decompress_streams_ms": med["decode_plain"],
    "c_ratio": med["decode_framed"] / med["decode_plain"],
    "d_index_ms": med["index_framed"], "d_index_us_per_chunk": med["index_framed"] * 1e3 / max(units, 1),
    "min_max_ms": {k: [min(v), max(v)] for k, v in ms.items()},
}
line = json.dumps(res)
print(line)
if tag:
    with open(os.path.join(ROOT, "profiles", tag + ".json"), "w") as f:
        f.write(line + "\n")

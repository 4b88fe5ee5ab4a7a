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
Run under rocprofv3 --kernel-trace --stats (a run of its own) for per-kernel times.

The range-decode leg, a run of its own with the same rules:
    python tools/frame_bench.py ranges [n_bytes] [reps] [tag]
  a  decompress_frame_ranges_device, one range [1, n - 1)
         vs  decompress_frame_device of the whole stream
  b  one 1 MiB range at 300 MiB + 12,345 (n / 3 + 12,345 for a smaller n)
         vs  the same range of the bare SINGLE stream (decompress_ranges_device)
  c  frame_seek_device"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "lightweight-snappy_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import datagen  # noqa: E402
import snappy_amd  # noqa: E402

CH = 65536


def timed(stream, fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    fn()
    b.record(stream)
    b.synchronize()
    return a.elapsed_time(b)


def median(v):
    return sorted(v)[len(v) // 2]


def text_in_hbm(n):
    host = np.empty(n, dtype=np.uint8)
    datagen.fill(host, "T", 1234, threads=16)
    return torch.from_numpy(host).cuda()


def rounds(stream, legs, reps, once):
    """every leg in turn, reps + 2 times: two warm-up rounds (code objects, scratch growth),
    the results checked once after the second; -> the timed rounds' ms per leg"""
    ms = {name: [] for name, _ in legs}
    with torch.cuda.stream(stream):
        for r in range(reps + 2):
            for name, fn in legs:
                t = timed(stream, fn)
                if r >= 2:
                    ms[name].append(t)
            if r == 1:
                once()
    stream.synchronize()
    return ms


def report(res, tag):
    line = json.dumps(res)
    print(line)
    if tag:
        with open(os.path.join(ROOT, "profiles", tag + ".json"), "w") as f:
            f.write(line + "\n")


def frames_leg(n, reps, tag):
    units = (n + CH - 1) // CH
    x = text_in_hbm(n)
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
                      torch.tensor([min(CH, n - u * CH) for u in range(units)], dtype=torch.int64)],
                     dim=1).cuda().contiguous()
    crcs = torch.empty(units, dtype=torch.int32, device="cuda")
    lib, h, vp = snappy_amd.lib(), codec._h, snappy_amd.ctypes.c_void_p
    state = {}

    def kf1():
        snappy_amd._check(lib.snappy_amd_crc32c_device(h, vp(x.data_ptr()), vp(ol.data_ptr()), units, 1,
                                                       vp(crcs.data_ptr())), "crc32c_device")

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
        snappy_amd._check(lib.snappy_amd_frame_index_device(h, vp(framed.data_ptr()), state["flen"],
                                                            vp(table.data_ptr()), units + 2, snappy_amd.ctypes.byref(nch),
                                                            snappy_amd.ctypes.byref(tot)), "frame_index_device")
        assert (nch.value, tot.value) == (units, n)

    def once():  # round trip, and the two tables agree
        assert torch.equal(back, x), "round trip failed"
        assert torch.equal(table[: units + 1], chunks), "device walk != compressor's table"

    ms = rounds(stream, (("kf1", kf1), ("compress_framed", compress_framed), ("compress_plain", compress_plain),
                         ("decode_framed", decode_framed), ("decode_plain", decode_plain),
                         ("index_framed", index_framed)), reps, once)
    codec.close()
    med = {k: median(v) for k, v in ms.items()}
    report({
        "n": n, "reps": reps, "chunks": units, "framed_bytes": state["flen"], "unframed_bytes": state["plen"],
        "a_kf1_ms": med["kf1"], "a_kf1_GBps": n / (med["kf1"] * 1e-3) / 1e9,
        "b_compress_frame_ms": med["compress_framed"], "b_compress_streams_ms": med["compress_plain"],
        "b_ratio": med["compress_framed"] / med["compress_plain"],
        "c_decompress_frame_ms": med["decode_framed"], "c_decompress_streams_ms": med["decode_plain"],
        "c_ratio": med["decode_framed"] / med["decode_plain"],
        "d_index_ms": med["index_framed"], "d_index_us_per_chunk": med["index_framed"] * 1e3 / max(units, 1),
        "min_max_ms": {k: [min(v), max(v)] for k, v in ms.items()},
    }, tag)


def ranges_leg(n, reps, tag):
    x = text_in_hbm(n)
    codec = snappy_amd.Codec(0)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):  # (the tensor forms bind the codec to torch's current stream: this one)
        framed, chunks = codec.compress_frame_tensor(x)
        bare, offs = codec.compress_tensor(x, chunk=CH, layout=snappy_amd.SINGLE)
        total, starts = codec.frame_seek_tensor(framed, chunks)
    assert total == n
    back = torch.empty(n + 16, dtype=torch.uint8, device="cuda")
    at = (300 << 20) + 12345 if n >= 400 << 20 else n // 3 + 12345
    mib = min(1 << 20, n - at)
    # every range's out_offset agrees with its start mod 16
    r_all, r_1m = [(1, n - 2, 1)], [(at, mib, at % 16)]

    def check(st):
        assert codec.last_ranges_status == 0 and int(st[0]) == 0

    def decode_framed():
        codec.decompress_frame_tensor(framed, chunks, n, out=back)

    def a_range_all():
        check(codec.decompress_frame_ranges_tensor(framed, 0, chunks, starts, r_all, out=back)[1])

    def b_range_1m():
        check(codec.decompress_frame_ranges_tensor(framed, 0, chunks, starts, r_1m, out=back)[1])

    def b_bare_range_1m():
        check(codec.decompress_ranges_tensor(bare, offs, n, r_1m, out=back)[1])

    def c_seek():
        assert codec.frame_seek_tensor(framed, chunks)[0] == n

    def once():
        a_range_all()
        assert torch.equal(back[1:n - 1], x[1:n - 1]), "range [1, n - 1) differs"
        b_range_1m()
        assert torch.equal(back[at % 16:at % 16 + mib], x[at:at + mib]), "the 1 MiB range differs"

    ms = rounds(stream, (("decode_framed", decode_framed), ("a_range_all", a_range_all), ("b_range_1m", b_range_1m),
                         ("b_bare_range_1m", b_bare_range_1m), ("c_seek", c_seek)), reps, once)
    codec.close()
    med = {k: median(v) for k, v in ms.items()}
    report({"n": n, "reps": reps, "chunks": chunks.numel() - 1, "framed_bytes": framed.numel(), "range_b": [at, mib],
            "decompress_frame_ms": med["decode_framed"], "a_range_all_ms": med["a_range_all"],
            "a_ratio": med["a_range_all"] / med["decode_framed"], "b_range_1m_ms": med["b_range_1m"],
            "b_bare_range_1m_ms": med["b_bare_range_1m"], "c_seek_ms": med["c_seek"],
            "min_max_ms": {k: [min(v), max(v)] for k, v in ms.items()}}, tag)


if __name__ == "__main__":
    args = sys.argv[1:]
    leg = frames_leg
    if args and args[0] == "ranges":
        leg, args = ranges_leg, args[1:]
    leg(int(args[0]) if args else 1 << 30, int(args[1]) if len(args) > 1 else 11, args[2] if len(args) > 2 else "")

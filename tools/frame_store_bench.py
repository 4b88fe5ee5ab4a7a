#!/usr/bin/env python3
"""Framed compress with and without SNAPPY_AMD_FRAME_STORE, and the decode of both
outputs, on one GPU: N bytes of datagen random bytes, then of datagen text, in HBM,
chunks of 65,536; HIP events on the codec's stream, medians of `reps` repetitions
after two warm-up rounds, all legs alternating in the same process (the method of
tools/frame_bench.py).

  compress        compress_frame_device_ex(chunk 65536, flags 0)
  compress_store  the same with SNAPPY_AMD_FRAME_STORE
  decode          decompress_frame_device of the first output, table given
  decode_store    of the second
  copy            a device-to-device hipMemcpyAsync of the N input bytes: what a
                  launch of stored chunks alone (kf2_store) has to move

Prints one JSON line per input and writes both to `out` when given:
    python tools/frame_store_bench.py [n_bytes] [reps] [out.json]
Run under rocprofv3 --kernel-trace --stats (a run of its own) for per-kernel times."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from frame_bench import median, rounds  # noqa: E402  (puts the package on sys.path)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import datagen  # noqa: E402
import snappy_amd  # noqa: E402

CH = 65536


def one_input(kind, n, reps):
    units = (n + CH - 1) // CH
    host = np.empty(n, dtype=np.uint8)
    datagen.fill(host, kind, 1234, threads=16)
    x = torch.from_numpy(host).cuda()
    codec = snappy_amd.Codec(0)
    stream = torch.cuda.Stream()
    codec.set_stream(stream.cuda_stream)
    cap = snappy_amd.max_frame_output(n, CH)
    outs = {f: torch.empty(cap, dtype=torch.uint8, device="cuda") for f in (0, snappy_amd.FRAME_STORE)}
    tabs = {f: torch.empty(units + 1, dtype=torch.int64, device="cuda") for f in outs}
    back = torch.empty(n, dtype=torch.uint8, device="cuda")
    lens = {}
    lib, h, vp, ct = snappy_amd.lib(), codec._h, snappy_amd.ctypes.c_void_p, snappy_amd.ctypes

    def compress(flags):
        def fn():
            lens[flags] = codec.compress_frame_ptr(x.data_ptr(), n, flags, outs[flags].data_ptr(),
                                                   tabs[flags].data_ptr(), CH)
        return fn

    def decode(flags):
        def fn():
            got = ct.c_size_t(0)
            snappy_amd._check(lib.snappy_amd_decompress_frame_device(h, vp(outs[flags].data_ptr()), lens[flags],
                                                                     vp(tabs[flags].data_ptr()), units,
                                                                     vp(back.data_ptr()), n, ct.byref(got)),
                              "decompress_frame_device")
            assert got.value == n
        return fn

    def copy():
        back.copy_(x, non_blocking=True)

    checked = []

    def once():  # both outputs decode to the input (the last decode leg ran on the stored one)
        for f in outs:
            back.zero_()
            decode(f)()
            assert torch.equal(back, x), "round trip failed"
        checked.append(True)

    S = snappy_amd.FRAME_STORE
    ms = rounds(stream, (("compress", compress(0)), ("compress_store", compress(S)), ("decode", decode(0)),
                         ("decode_store", decode(S)), ("copy", copy)), reps, once)
    assert checked
    types = outs[S][tabs[S][:-1]].to(torch.int64)
    stored = int(types.sum())
    codec.close()
    med = {k: median(v) for k, v in ms.items()}
    res = {"input": {"R": "random", "T": "text"}[kind], "n": n, "chunk": CH, "reps": reps, "chunks": units,
           "stored_chunks": stored, "bytes": lens[0], "bytes_store": lens[S]}
    for k, v in med.items():
        res[k + "_ms"] = v
        res[k + "_GBps"] = n / (v * 1e-3) / 1e9
    res["min_max_ms"] = {k: [min(v), max(v)] for k, v in ms.items()}
    return res


def main(argv):
    n = int(argv[0]) if argv else 1 << 30
    reps = int(argv[1]) if len(argv) > 1 else 11
    lines = []
    for kind in "RT":
        lines.append(json.dumps(one_input(kind, n, reps)))
        print(lines[-1], flush=True)
        torch.cuda.empty_cache()
    if len(argv) > 2:
        with open(argv[2], "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main(sys.argv[1:])

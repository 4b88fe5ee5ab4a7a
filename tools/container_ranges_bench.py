#!/usr/bin/env python3
"""Range decode of containers on one GPU, under the conditions of
7.5's measurements: N bytes of datagen text in HBM, compressed into a Hadoop and
a snappy-java container at the formats' default blocks; HIP events around the
whole synchronous call, two warm-up rounds, medians of `reps` with min..max, the
calls alternating in one process.  Per format:

  a  decompress_container_ranges_device, one range [1, n - 1)
         vs  decompress_container_device with the tables given
  b  one 1 MiB range at 300 MiB + 12,345 (n / 3 + 12,345 for a smaller n)
         vs  the same range of the bare SINGLE stream (decompress_ranges_device)

Prints one JSON line and writes it to profiles/<tag>.json when a tag is given:
    python tools/container_ranges_bench.py [n_bytes] [reps] [tag]
Run under rocprofv3 --kernel-trace --stats (a run of its own) for per-kernel times."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "lightweight-snappy_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch  # noqa: E402

import snappy_amd  # noqa: E402
from frame_bench import CH, median, report, rounds, text_in_hbm  # noqa: E402

FORMATS = (("hadoop", snappy_amd.CONTAINER_HADOOP), ("xerial", snappy_amd.CONTAINER_XERIAL))


def main(n, reps, tag):
    x = text_in_hbm(n)
    codec = snappy_amd.Codec(0)
    stream = torch.cuda.Stream()
    cont = {}
    with torch.cuda.stream(stream):  # (the tensor forms bind the codec to torch's current stream: this one)
        for name, fmt in FORMATS:
            cont[name] = codec.compress_container_tensor(x, fmt)
        bare, offs = codec.compress_tensor(x, chunk=CH, layout=snappy_amd.SINGLE)
    back = torch.empty(n + 16, dtype=torch.uint8, device="cuda")
    at = (300 << 20) + 12345 if n >= 400 << 20 else n // 3 + 12345
    mib = min(1 << 20, n - at)
    # every range's out_offset agrees with its start mod 16
    r_all, r_1m = [(1, n - 2, 1)], [(at, mib, at % 16)]

    def check(st):
        assert codec.last_ranges_status == 0 and int(st[0]) == 0

    def whole(name, fmt):
        c, comp, outp = cont[name]
        return lambda: codec.decompress_container_tensor(c, fmt, comp, outp, cap=n, out=back)

    def ranges(name, r):
        c, comp, outp = cont[name]
        return lambda: check(codec.decompress_container_ranges_tensor(c, 0, comp, outp, r, out=back)[1])

    def b_bare_range_1m():
        check(codec.decompress_ranges_tensor(bare, offs, n, r_1m, out=back)[1])

    legs = [("b_bare_range_1m", b_bare_range_1m)]
    for name, fmt in FORMATS:
        legs += [(name + "_decompress_container", whole(name, fmt)), (name + "_a_range_all", ranges(name, r_all)),
                 (name + "_b_range_1m", ranges(name, r_1m))]

    def once():
        for name, fmt in FORMATS:
            back.zero_()
            ranges(name, r_all)()
            assert torch.equal(back[1:n - 1], x[1:n - 1]), name + ": range [1, n - 1) differs"
            back.zero_()
            ranges(name, r_1m)()
            assert torch.equal(back[at % 16:at % 16 + mib], x[at:at + mib]), name + ": the 1 MiB range differs"

    ms = rounds(stream, legs, reps, once)
    codec.close()
    med = {k: median(v) for k, v in ms.items()}
    res = {"n": n, "reps": reps, "range_b": [at, mib], "b_bare_range_1m_ms": med["b_bare_range_1m"]}
    for name, fmt in FORMATS:
        c, comp, outp = cont[name]
        res[name] = {"chunks": comp.numel() // 2, "container_bytes": c.numel(),
                     "decompress_container_ms": med[name + "_decompress_container"],
                     "a_range_all_ms": med[name + "_a_range_all"],
                     "a_ratio": med[name + "_a_range_all"] / med[name + "_decompress_container"],
                     "b_range_1m_ms": med[name + "_b_range_1m"],
                     "b_minus_bare_ms": med[name + "_b_range_1m"] - med["b_bare_range_1m"]}
    res["min_max_ms"] = {k: [min(v), max(v)] for k, v in ms.items()}
    report(res, tag)


if __name__ == "__main__":
    args = sys.argv[1:]
    main(int(args[0]) if args else 1 << 30, int(args[1]) if len(args) > 1 else 11, args[2] if len(args) > 2 else "")

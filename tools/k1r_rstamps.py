#!/usr/bin/env python3
"""Window-refresh share of K1r / K1r64 with the asm round loop in place
(SNAPPY_K1R_RSTAMPS build): loop cycles per unit, token-flush and window-move
cycles per refresh, exits from the asm statement by code, and the glue around
one group of exits (from the statement's end to the first useful instruction
outside, from the last one back to the statement).  The build picks the group
with -DSNAPPY_K1R_RSTAMPS_GROUP=: 1 code-2 refreshes without a token flush,
2 code-2 refreshes with one, 4 / 5 the code-4 / code-5 exits that come back.
K1r refreshes, flushes and finishes tag collisions inside its statement (it
leaves with code 2 only for a flush that holds a long-form token, never with
code 5): the refresh-by-exit groups are measured on K1r64 (CHUNK 65536), whose
statement keeps those exits.
Usage: tools/k1r_rstamps.py BYTES CHUNK [VARIANT [GROUP]]
(VARIANT: tools/build_pads.sh 'rst:-DSNAPPY_K1R_RSTAMPS'; GROUP: the group the
variant was built with, for the label)"""
import ctypes, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "lightweight-snappy_amd"))
os.environ["SNAPPY_AMD_LIB"] = os.path.join(ROOT, "lightweight-snappy_amd", "variants",
                                            "libsnappy_amd_" + (sys.argv[3] if len(sys.argv) > 3 else "rst") + ".so")
import numpy as np, torch
import datagen, snappy_amd
n = int(sys.argv[1]) if len(sys.argv) > 1 else 256 << 20
chunk = int(sys.argv[2]) if len(sys.argv) > 2 else 32768
group = int(sys.argv[4]) if len(sys.argv) > 4 else 1
layout = snappy_amd.SINGLE if chunk == 65536 else snappy_amd.STREAMS
a = datagen.make("T", n, 1234)
x = torch.from_numpy(a).cuda()
c = snappy_amd.Codec(0)
comp, offs = c.compress_tensor(x, chunk=chunk, layout=layout)
torch.cuda.synchronize()
class Ctx(ctypes.Structure):
    _fields_ = [("device", ctypes.c_int), ("own", ctypes.c_void_p), ("stream", ctypes.c_void_p),
                ("sizes", ctypes.c_void_p), ("sizes_cap", ctypes.c_size_t),
                ("tokens", ctypes.c_void_p), ("tokens_cap", ctypes.c_size_t)]
ctx = ctypes.cast(c._h, ctypes.POINTER(Ctx)).contents
units = n // chunk
tok_cap = chunk // 4 + 2
hip = ctypes.CDLL("libamdhip64.so")
buf = np.empty(units * 4, dtype=np.uint64)
hip.hipMemcpy(buf.ctypes.data_as(ctypes.c_void_p), ctypes.c_void_p(ctx.tokens + units * tok_cap * 8),
              ctypes.c_size_t(buf.nbytes), 2)
raw = buf.reshape(units, 4)
f = lambda v: v.astype(np.float64).mean()
loop = f(raw[:, 0] & ((1 << 30) - 1))
gout, ng = f((raw[:, 0] >> 30) & ((1 << 22) - 1)), f(raw[:, 0] >> 52)
fl, asm = f(raw[:, 1] & ((1 << 24) - 1)), f(raw[:, 1] >> 24)
win, gin, nasm = f(raw[:, 2] & ((1 << 24) - 1)), f((raw[:, 2] >> 24) & ((1 << 22) - 1)), f(raw[:, 2] >> 46)
nref, nfl = f(raw[:, 3] & 0xFFF), f((raw[:, 3] >> 12) & 0xFFF)
c3, c4, c5 = f((raw[:, 3] >> 24) & 0xFFF), f((raw[:, 3] >> 36) & 0x3FFF), f(raw[:, 3] >> 50)
what = {1: "code-2 refreshes without a flush", 2: "code-2 refreshes with a token flush",
        4: "code-4 exits that come back", 5: "code-5 exits that come back"}[group]
print(f"chunk {chunk}: loop {loop:.0f} cycles/unit; refreshes in C++ {nref:.1f}/unit ({nfl:.1f} with a token flush)")
print(f"  asm round loop {asm/loop*100:5.1f}%  {nasm:.1f} entries/unit, {asm/max(nasm,1):.0f} cycles/entry; exits by code: "
      f"1 and 2 {nasm-c3-c4-c5:.1f}, 3 {c3:.1f}, 4 {c4:.2f}, 5 {c5:.2f}")
print(f"  window move    {win/loop*100:5.1f}%  {win/max(nref,1):6.0f} cycles/refresh (s_memtime clock)")
print(f"  token flush    {fl/loop*100:5.1f}%  {fl/max(nfl,1e-9):6.0f} cycles/flush")
print(f"  {what}: {ng:.2f}/unit; glue from the asm statement's end to the first useful instruction "
      f"{gout/max(ng,1e-9):.0f} cycles/exit, from the last one to the statement {gin/max(ng,1e-9):.0f} "
      f"(each holds one stamp; {(gout+gin)/loop*100:.2f}% of the loop)")
print(f"  rest (C++ rounds, W-probe rounds, stamps) {(loop-asm-win-fl)/loop*100:5.1f}%")

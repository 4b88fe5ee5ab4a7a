// v_alignbyte_b32 D, S0, S1, S2 = ({S0, S1} >> 8 * shift)[31:0]: which bits of
// S2 make the shift?  With S2[1:0] alone a byte position x is its own funnel
// operand (the four bytes at x of little-endian dwords are alignbyte(next,
// cur, x)); if higher bits count, x has to be masked or shifted first.  Each
// lane funnels with S2 = lane's low two bits plus a pattern of high bits, as a
// VGPR and as an SGPR operand, next to v_alignbit_b32 with 8 * S2.
#include <hip/hip_runtime.h>
#include <cstdio>

constexpr uint32_t kHi = 0x0B0A0908u, kLo = 0x03020100u;

__global__ __launch_bounds__(64) void k(const uint32_t *sh, uint32_t *out)
{
    const uint32_t lane = threadIdx.x;
    const uint32_t s = sh[lane];
    uint32_t byv, biv, bys;
    asm volatile("v_alignbyte_b32 %0, %1, %2, %3" : "=v"(byv) : "v"(kHi), "v"(kLo), "v"(s));
    asm volatile("v_alignbit_b32 %0, %1, %2, %3" : "=v"(biv) : "v"(kHi), "v"(kLo), "v"(s << 3));
    // the scalar operand: lane 0's shift for every lane
    asm volatile("v_alignbyte_b32 %0, %1, %2, %3"
                 : "=v"(bys)
                 : "v"(kHi), "v"(kLo), "s"(__builtin_amdgcn_readfirstlane(sh[blockIdx.x])));
    out[blockIdx.x * 192 + lane] = byv;
    out[blockIdx.x * 192 + 64 + lane] = biv;
    out[blockIdx.x * 192 + 128 + lane] = bys;
}

int main()
{
    // lane l: low bits l & 3, high bits from a pattern chosen by l >> 2
    const uint32_t pat[16] = {0,          0x4,        0x8,        0x10,       0x1C,       0x20,
                              0x100,      0xFFFC,     0x10000,    0x7FFC,     0x80000000, 0xFFFFFFFC,
                              0x12345678 & ~3u, 0x3FC, 0x1000000,  0x18};
    uint32_t hs[64], h[64 * 192];
    for (int l = 0; l < 64; l++) hs[l] = pat[l >> 2] | (l & 3);
    uint32_t *ds, *d;
    (void)hipMalloc(&ds, sizeof(hs));
    (void)hipMalloc(&d, sizeof(h));
    (void)hipMemcpy(ds, hs, sizeof(hs), hipMemcpyHostToDevice);
    hipLaunchKernelGGL(k, dim3(64), dim3(64), 0, 0, ds, d);
    hipError_t e = hipMemcpy(h, d, sizeof(h), hipMemcpyDeviceToHost);
    const uint64_t w = ((uint64_t)kHi << 32) | kLo;
    int bad_byte_v = 0, bad_byte_s = 0, bad_bit = 0;
    for (int l = 0; l < 64; l++) {
        const uint32_t want = (uint32_t)(w >> (8 * (hs[l] & 3)));  // S2[1:0] alone
        const uint32_t want_bit = (uint32_t)(w >> ((hs[l] << 3) & 31));
        if (h[l] != want) {
            if (bad_byte_v++ < 8) printf("alignbyte vgpr S2 %08x: got %08x want %08x\n", hs[l], h[l], want);
        }
        if (h[64 + l] != want_bit) bad_bit++;
        // block b's scalar operand is hs[b]
        if (h[l * 192 + 128] != want) {
            if (bad_byte_s++ < 8) printf("alignbyte sgpr S2 %08x: got %08x want %08x\n", hs[l], h[l * 192 + 128], want);
        }
    }
    printf("hip %d; v_alignbyte_b32 shifts by S2[1:0] alone: vgpr %s (%d of 64 differ), sgpr %s (%d of 64 differ); "
           "v_alignbit_b32 by S2[4:0]: %s\n",
           (int)e, bad_byte_v ? "NO" : "yes", bad_byte_v, bad_byte_s ? "NO" : "yes", bad_byte_s, bad_bit ? "NO" : "yes");
    return 0;
}

// snappy_frame.hip -- the Snappy framing format (framing_format.txt of
// google/snappy) on the device: a stream identifier, then chunks of at most
// 65,536 uncompressed bytes, each its own raw Snappy stream (or stored bytes)
// under the masked CRC-32C of its uncompressed bytes.
//
//   KF1  kf1_crc32c      batched CRC-32C, one wave per (offset, length) entry
//   KF2  kf2_headers     identifier + chunk headers around the payloads K2 wrote
//        kf2_choose      SNAPPY_AMD_FRAME_STORE: which chunks are stored (type 01), their slots
//        kf2_store       the stored chunks' bytes, 16-byte stores at any alignment pair
//   KF3  kf3_walk        chunk walk of a foreign stream (one wave, one hop per chunk)
//   KF4  kf4_scan        per data chunk: header checks, decoded length, scratch bytes
//        kf4_gather      payloads -> contiguous scratch, as SNAPPY_AMD_STREAMS units
//        kf4_verify      stored CRC against KF1's over the decoded bytes
//   KF5  kf5_seek_lens   kf4_scan's lengths for the seek table (their K3 scan is the table)
//
// The match finder, the scan, the emitter (K1r64, K3, K2) and the decoder (K4)
// are the unframed path's kernels, unchanged (the compress ones through the
// unframed path's own compress_launch, snappy_device.hip): a framed chunk's
// payload is exactly a STREAMS unit of the chunk size (1..65,536 bytes; with
// FRAME_STORE K2 runs from its entry point k2_emit_units_sel).  Declared in
// include/snappy_amd.h.  DESIGN.md 7.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include <vector>

#include "snappy_amd.h"
#include "snappy_ctx.h"
#include "snappy_frame.h"
#include "snappy_kernels.h"

using namespace snappy_amd;

namespace {

// ---------------------------------------------------------------------------
// CRC-32C (iSCSI): polynomial 0x82F63B78 reflected, init and xor-out all ones.
// A register value is a polynomial over GF(2) with bit 31 = x^0 ... bit 0 =
// x^31; one zero bit shifted in multiplies it by x modulo P.
// ---------------------------------------------------------------------------
constexpr uint32_t kCrcPoly = 0x82F63B78u;

constexpr uint32_t gf_xtime(uint32_t a) { return (a >> 1) ^ ((a & 1u) ? kCrcPoly : 0u); }

__host__ __device__ constexpr uint32_t gf_mul(uint32_t a, uint32_t b)
{
    uint32_t r = 0;
    for (int i = 0; i < 32; i++) {
        if (b & (0x80000000u >> i)) r ^= a;
        a = (a >> 1) ^ ((a & 1u) ? kCrcPoly : 0u);
    }
    return r;
}

constexpr uint32_t gf_xpow(uint32_t e)  // x^e mod P
{
    uint32_t r = 0x80000000u, b = 0x40000000u;
    for (; e; e >>= 1) {
        if (e & 1u) r = gf_mul(r, b);
        b = gf_mul(b, b);
    }
    return r;
}

// KF1 gives lane l the dwords l, l + 64, ... of an entry, so the wave's loads
// stay coalesced; a lane's step is acc = acc * x^2048 ^ dword (the 256 bytes
// the other lanes cover in between), the multiply by that one constant being
// four byte-indexed table lookups (z); at the end lane l's partial is still
// 64 - l dwords short of the entry's end (lane[l] = x^(32 (64 - l))).
struct CrcTables {
    uint32_t z[4][256];  // z[k][b] = (b << 8 k) * x^2048
    uint32_t t0[256];    // the bytewise table: b * x^8 for b in the low byte
    uint32_t lane[64];
};

constexpr CrcTables make_crc_tables()
{
    CrcTables t{};
    const uint32_t x2048 = gf_xpow(2048);
    for (uint32_t k = 0; k < 4; k++)
        for (uint32_t b = 0; b < 256; b++) t.z[k][b] = gf_mul(b << (8 * k), x2048);
    for (uint32_t b = 0; b < 256; b++) {
        uint32_t c = b;
        for (int k = 0; k < 8; k++) c = gf_xtime(c);
        t.t0[b] = c;
    }
    for (uint32_t l = 0; l < 64; l++) t.lane[l] = gf_xpow(32 * (64 - l));
    return t;
}

__device__ const CrcTables g_crc = make_crc_tables();

constexpr uint32_t kCrcMaskDelta = 0xA282EAD8u;
constexpr uint32_t kF1Waves = 4;  // entries per workgroup (they share the LDS tables)

// Entry e = base[off, off + len): off_len[2 e], off_len[2 e + 1], or (off_len
// null) the e-th `stride`-byte piece of base[0, n).  Any alignment, any length.
__global__ __launch_bounds__(64 * kF1Waves) void kf1_crc32c(const uint8_t *__restrict__ base,
                                                            const uint64_t *__restrict__ off_len, uint64_t count,
                                                            uint64_t stride, uint64_t n, uint32_t masked,
                                                            uint32_t *__restrict__ crc)
{
    __shared__ uint32_t zt[4 * 256];
    __shared__ uint32_t t0[256];
    for (uint32_t i = threadIdx.x; i < 4 * 256; i += 64 * kF1Waves) zt[i] = (&g_crc.z[0][0])[i];
    for (uint32_t i = threadIdx.x; i < 256; i += 64 * kF1Waves) t0[i] = g_crc.t0[i];
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t e = (uint64_t)blockIdx.x * kF1Waves + (threadIdx.x >> 6);
    if (e >= count) return;
    uint64_t off, len;
    if (off_len) {
        off = off_len[2 * e];
        len = off_len[2 * e + 1];
    } else {
        off = e * stride;
        len = n - off < stride ? n - off : stride;
    }
    const uint8_t *p = base + off;
    uint32_t s = 0xFFFFFFFFu;
    if (len < 4) {
        for (uint32_t k = 0; k < (uint32_t)len; k++) s = t0[(s ^ p[k]) & 0xFFu] ^ (s >> 8);
    } else {
        // The aligned dwords q[0 .. nd) cover the entry up to its last < 4 bytes;
        // the bytes of q[0] before the entry count as zeros in front of it (they
        // change nothing), and CRC's init comes in by xoring ones into the
        // entry's first four bytes (then the register starts at 0).
        const uint32_t head = (uint32_t)(reinterpret_cast<uintptr_t>(p) & 3u);
        const uint32_t *q = reinterpret_cast<const uint32_t *>(p - head);
        const uint64_t nd = (head + len) >> 2;  // >= 1
        const uint32_t m0 = 0xFFFFFFFFu << (8 * head);
        const uint32_t m1 = head ? 0xFFFFFFFFu >> (8 * (4 - head)) : 0u;
        // zero dwords in front so the count is a multiple of 64
        const uint32_t pad = (64u - (uint32_t)(nd & 63u)) & 63u;
        const uint64_t nb = (nd + pad) >> 6;
#define KF1_Z(a) (zt[(a) & 0xFFu] ^ zt[256 + (((a) >> 8) & 0xFFu)] ^ zt[512 + (((a) >> 16) & 0xFFu)] ^ zt[768 + ((a) >> 24)])
        uint32_t acc = 0;
        if (lane >= pad) {  // the first 64: q[0], q[1] and the padding are in it
            const uint32_t i = lane - pad;
            acc = q[i];
            if (i == 0) acc = ~acc & m0;
            else if (i == 1) acc ^= m1;
        }
        const uint32_t *r = q + 64 - pad + lane;  // this lane's dword of the second 64
        uint64_t k = 1;
        if (pad == 63 && nb > 1) {  // q[0] stood alone in the first 64: q[1] opens the second
            uint32_t w = r[0];
            if (lane == 0) w ^= m1;
            acc = KF1_Z(acc) ^ w;
            k = 2;
            r += 64;
        }
        for (; k + 4 <= nb; k += 4, r += 256) {
            const uint32_t w0 = r[0], w1 = r[64], w2 = r[128], w3 = r[192];
            acc = KF1_Z(acc) ^ w0;
            acc = KF1_Z(acc) ^ w1;
            acc = KF1_Z(acc) ^ w2;
            acc = KF1_Z(acc) ^ w3;
        }
        for (; k < nb; k++, r += 64) acc = KF1_Z(acc) ^ r[0];
#undef KF1_Z
        acc = gf_mul(acc, g_crc.lane[lane]);
        for (uint32_t d = 32; d; d >>= 1) acc ^= __shfl_xor(acc, d);
        s = acc;
        const uint8_t *qb = reinterpret_cast<const uint8_t *>(q);
        for (uint64_t t = 4 * nd; t < head + len; t++) {
            uint32_t b = qb[t];
            if (t - head < 4) b ^= 0xFFu;
            s = t0[(s ^ b) & 0xFFu] ^ (s >> 8);
        }
    }
    uint32_t c = ~s;
    if (masked) c = ((c >> 15) | (c << 17)) + kCrcMaskDelta;
    if (lane == 0) crc[e] = c;
}

// ---------------------------------------------------------------------------
// KF2: compress side.  K1r64 left each unit's stream size in sizes[]; adding 8
// before the scan makes room for a chunk header in front of every payload, so
// K2 (given out + ident + 8) puts payload u right behind where its header goes.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void kf2_bump(uint32_t *__restrict__ sizes, uint64_t units)
{
    const uint64_t u = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (u < units) sizes[u] += 8u;
}

// SNAPPY_AMD_FRAME_STORE: kf2_choose in kf2_bump's place.  One thread per chunk:
// the store rule (snappy_frame_store_chunk) on the chunk's R input bytes and its
// stream's P bytes; a stored chunk's slot is its header and its R bytes, so the
// scan lays the stored chunks out too, and K2 (k2_emit_units_sel) skips them.
__global__ __launch_bounds__(256) void kf2_choose(uint32_t *__restrict__ sizes, uint64_t units, uint64_t n,
                                                  uint32_t chunk, uint32_t *__restrict__ stored)
{
    const uint64_t u = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (u >= units) return;
    const uint64_t at = u * chunk;
    const uint32_t R = (uint32_t)(n - at < chunk ? n - at : chunk), P = sizes[u];
    const uint32_t st = snappy_frame_store_chunk(R, P) ? 1u : 0u;
    stored[u] = st;
    sizes[u] = (st ? R : P) + 8u;
}

constexpr uint32_t kF2StoreThreads = 256;  // 4 waves: 4 KiB of a chunk per round of 16-byte stores
constexpr uint32_t kF2StoreSpan = 16 * kF2StoreThreads;
constexpr uint32_t kF2StoreParts = 4;      // workgroups per chunk above 3 rounds: 16 waves on 65,536 bytes
typedef uint32_t kf2_u32x4 __attribute__((ext_vector_type(4)));

// Stored chunk u (blockIdx.x; blockIdx.y = its part): in[u * chunk, + R) to out +
// ident + offsets[u] + 8.  16-byte stores at the destination's alignment; the source
// bytes of each come from the four or five aligned dwords that hold them (every
// dword read holds a byte of the chunk), shifted into place.  Part 0 also writes the
// < 16 bytes in front of the first aligned store and behind the last.  No byte
// outside the chunk's R payload bytes is written, none outside in[0, n) read
// beyond the aligned dwords of its first and last byte.
__global__ __launch_bounds__(kF2StoreThreads) void kf2_store(const uint8_t *__restrict__ in, uint64_t n, uint32_t chunk,
                                                             const uint32_t *__restrict__ stored,
                                                             const uint64_t *__restrict__ offsets, uint32_t ident,
                                                             uint8_t *__restrict__ out)
{
    const uint32_t u = blockIdx.x;
    if (!stored[u]) return;
    const uint64_t at = (uint64_t)u * chunk;
    const uint32_t R = (uint32_t)(n - at < chunk ? n - at : chunk), t = threadIdx.x;
    const uint8_t *const src = in + at;
    uint8_t *const dst = out + ident + offsets[u] + 8;
    const uint32_t h0 = (uint32_t)(-reinterpret_cast<uintptr_t>(dst) & 15);
    const uint32_t h = h0 < R ? h0 : R;
    const uint32_t body = (R - h) & ~15u;
    const uint8_t *const s = src + h;
    uint8_t *const d = dst + h;
    const uint32_t sa = (uint32_t)(reinterpret_cast<uintptr_t>(s) & 3);
    const uint32_t *const s4 = reinterpret_cast<const uint32_t *>(s - sa);
    const uint32_t first = (blockIdx.y * kF2StoreThreads + t) * 16u, step = gridDim.y * kF2StoreSpan;
    if (sa == 0) {
        for (uint32_t x = first; x < body; x += step) {
            const uint32_t *const q = s4 + x / 4;
            const kf2_u32x4 v = {q[0], q[1], q[2], q[3]};
            *reinterpret_cast<kf2_u32x4 *>(d + x) = v;
        }
    } else {
        const uint32_t sh = 8 * sa;
        for (uint32_t x = first; x < body; x += step) {
            const uint32_t *const q = s4 + x / 4;
            const uint32_t w0 = q[0], w1 = q[1], w2 = q[2], w3 = q[3], w4 = q[4];
            const kf2_u32x4 v = {__builtin_amdgcn_alignbit(w1, w0, sh), __builtin_amdgcn_alignbit(w2, w1, sh),
                                 __builtin_amdgcn_alignbit(w3, w2, sh), __builtin_amdgcn_alignbit(w4, w3, sh)};
            *reinterpret_cast<kf2_u32x4 *>(d + x) = v;
        }
    }
    if (blockIdx.y == 0) {  // h < 16 and R - h - body < 16
        if (t < h) dst[t] = src[t];
        const uint32_t done = h + body;
        if (done + t < R) dst[done + t] = src[done + t];
    }
}

// offsets/sizes: the scan of the bumped sizes.  Chunk u: its type (00, or 01 where
// stored[u] is set; stored null: all 00), 24-bit (4 + payload bytes), masked CRC, at
// out + ident + offsets[u]; chunks[u] = that position.
__global__ __launch_bounds__(256) void kf2_headers(uint8_t *__restrict__ out, uint32_t ident,
                                                   const uint64_t *__restrict__ offsets,
                                                   const uint32_t *__restrict__ sizes,
                                                   const uint32_t *__restrict__ crc,
                                                   const uint32_t *__restrict__ stored, uint64_t units,
                                                   uint64_t *__restrict__ chunks)
{
    const uint64_t u = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (u == 0) {
        const uint8_t id[SNAPPY_FRAME_IDENT_LEN] = {0xFF, 0x06, 0x00, 0x00, 0x73, 0x4E, 0x61, 0x50, 0x70, 0x59};
        for (uint32_t k = 0; k < ident; k++) out[k] = id[k];
        chunks[units] = ident + (units ? offsets[units] : 0ull);
    }
    if (u >= units) return;
    const uint64_t at = ident + offsets[u];
    const uint32_t len = sizes[u] - 8u + 4u, c = crc[u];
    uint8_t *h = out + at;
    h[0] = stored && stored[u] ? 0x01 : 0x00;
    h[1] = (uint8_t)len;
    h[2] = (uint8_t)(len >> 8);
    h[3] = (uint8_t)(len >> 16);
    h[4] = (uint8_t)c;
    h[5] = (uint8_t)(c >> 8);
    h[6] = (uint8_t)(c >> 16);
    h[7] = (uint8_t)(c >> 24);
    chunks[u] = at;
}

// ---------------------------------------------------------------------------
// KF3: the chunk walk.  A dependent chain, one hop (one round of loads) per
// chunk: latency-bound like the one-wave index walk of K5.  Every lane walks
// the same chain; no byte at or past clen is read.
// result[0] = status, [1] = decoded bytes, [2] = data chunks.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(64) void kf3_walk(const uint8_t *__restrict__ f, uint64_t clen,
                                               uint64_t *__restrict__ chunks, uint64_t max_chunks,
                                               uint32_t need_ident, int64_t *__restrict__ result)
{
    uint64_t pos = 0, total = 0, count = 0;
    int32_t st = SNAPPY_AMD_OK;
    int first = need_ident != 0;
    if (max_chunks == 0) st = SNAPPY_AMD_ERR_CAPACITY;
    while (st == SNAPPY_AMD_OK && pos < clen) {
        uint8_t w[SNAPPY_FRAME_WINDOW];
        const uint64_t avail = clen - pos;
#pragma unroll
        for (uint32_t k = 0; k < SNAPPY_FRAME_WINDOW; k++) w[k] = k < avail ? f[pos + k] : (uint8_t)0;
        uint32_t dlen;
        uint64_t adv;
        const int r = snappy_frame_chunk(w, avail, first, &dlen, &adv);
        if (r < 0) {
            st = r;
            break;
        }
        first = 0;
        if (r == 1) {
            if (count + 1 >= max_chunks) {  // (the closing entry needs a place too)
                st = SNAPPY_AMD_ERR_CAPACITY;
                break;
            }
            if (threadIdx.x == 0) chunks[count] = pos;
            count++;
            total += dlen;
        }
        pos += adv;
    }
    if (threadIdx.x == 0) {
        if (st == SNAPPY_AMD_OK) chunks[count] = clen;
        result[0] = st;
        result[1] = (int64_t)total;
        result[2] = (int64_t)count;
    }
}

// ---------------------------------------------------------------------------
// KF4: decode side.
// ---------------------------------------------------------------------------
struct FrameInfo {
    int32_t st;      // SNAPPY_AMD_OK or the chunk's error
    uint32_t dlen;   // decoded bytes
    uint32_t ssize;  // bytes of its raw stream in the scratch
    uint32_t type;
};

// One thread per entry of the caller's chunk table: nothing is taken on trust
// but that the entries are the stream's data chunks -- every read is checked
// against clen.
__global__ __launch_bounds__(256) void kf4_scan(const uint8_t *__restrict__ f, uint64_t clen,
                                                const uint64_t *__restrict__ chunks, uint64_t nchunks,
                                                FrameInfo *__restrict__ info)
{
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= nchunks) return;
    const uint64_t pos = chunks[i];
    FrameInfo o = {SNAPPY_AMD_OK, 0u, 0u, 0u};
    if (pos >= clen) {
        o.st = SNAPPY_AMD_ERR_TRUNCATED;
    } else {
        uint8_t w[SNAPPY_FRAME_WINDOW];
        const uint64_t avail = clen - pos;
#pragma unroll
        for (uint32_t k = 0; k < SNAPPY_FRAME_WINDOW; k++) w[k] = k < avail ? f[pos + k] : (uint8_t)0;
        uint32_t dlen = 0;
        uint64_t adv = 0;
        const int r = snappy_frame_chunk(w, avail, 0, &dlen, &adv);
        if (r < 0) o.st = r;
        else if (r == 0) o.st = SNAPPY_AMD_ERR_INDEX;  // not a data chunk: not this stream's table
        else {
            const uint32_t plen = (uint32_t)(adv - 8);
            o.type = w[0];
            o.dlen = dlen;
            if (o.type == 0x01u) {
                o.ssize = snappy_frame_varint_len(dlen) + snappy_frame_literal_tag_len(dlen) + dlen;
            } else {
                o.ssize = plen;
                // an empty chunk goes to no decoder: elements behind its preamble overrun it
                uint32_t v;
                if (dlen == 0 && plen != snappy_frame_preamble(w + 8, plen < 5u ? plen : 5u, &v))
                    o.st = SNAPPY_AMD_ERR_OVERRUN;
            }
        }
    }
    info[i] = o;
}

constexpr uint32_t kF4Waves = 4;

// One wave per unit (a data chunk that decodes to >= 1 byte, checked by
// kf4_scan): its payload to scr + idx[j]; a stored chunk becomes the raw stream
// varint(len) ++ one literal element, whose <= 6 header bytes idx[] has room for.
__global__ __launch_bounds__(64 * kF4Waves) void kf4_gather(const uint8_t *__restrict__ f,
                                                            const uint64_t *__restrict__ cpos,
                                                            const uint64_t *__restrict__ idx, uint64_t units,
                                                            uint8_t *__restrict__ scr)
{
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t j = (uint64_t)blockIdx.x * kF4Waves + (threadIdx.x >> 6);
    if (j >= units) return;
    const uint8_t *h = f + cpos[j];
    const uint32_t type = h[0];
    const uint32_t plen = ((uint32_t)h[1] | ((uint32_t)h[2] << 8) | ((uint32_t)h[3] << 16)) - 4u;
    uint8_t *dst = scr + idx[j];
    if (type == 0x01u) {
        uint8_t hb[6];
        uint32_t k = 0;
        for (uint32_t v = plen;; v >>= 7) {
            hb[k++] = (uint8_t)((v & 0x7Fu) | (v >= 128u ? 0x80u : 0u));
            if (v < 128u) break;
        }
        const uint32_t L = plen - 1u;
        if (L < 60u) {
            hb[k++] = (uint8_t)(L << 2);
        } else if (L < 256u) {
            hb[k++] = (uint8_t)(60u << 2);
            hb[k++] = (uint8_t)L;
        } else {
            hb[k++] = (uint8_t)(61u << 2);
            hb[k++] = (uint8_t)L;
            hb[k++] = (uint8_t)(L >> 8);
        }
        if (lane == 0)
            for (uint32_t b = 0; b < k; b++) dst[b] = hb[b];
        dst += k;
    }
    snappy_frame_wave_copy(dst, h + 8, plen, lane);
}

__global__ __launch_bounds__(256) void kf4_verify(const uint8_t *__restrict__ f, const uint64_t *__restrict__ chunks,
                                                  uint64_t nchunks, const uint32_t *__restrict__ crc,
                                                  int32_t *__restrict__ cst)
{
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= nchunks) return;
    const uint8_t *h = f + chunks[i] + 4;
    const uint32_t stored = (uint32_t)h[0] | ((uint32_t)h[1] << 8) | ((uint32_t)h[2] << 16) | ((uint32_t)h[3] << 24);
    cst[i] = stored == crc[i] ? SNAPPY_AMD_OK : SNAPPY_AMD_ERR_CHECKSUM;
}

// KF5: the seek table's input.  One thread per entry kf4_scan looked at: its decoded
// length for the scan (0 where it failed), and the first failing entry as
// entry << 8 | -status (atomicMin; ~0 before).
__global__ __launch_bounds__(256) void kf5_seek_lens(const FrameInfo *__restrict__ info, uint64_t nchunks,
                                                     uint32_t *__restrict__ lens, unsigned long long *__restrict__ first)
{
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= nchunks) return;
    const FrameInfo o = info[i];
    lens[i] = o.st == SNAPPY_AMD_OK ? o.dlen : 0u;
    if (o.st != SNAPPY_AMD_OK) atomicMin(first, ((unsigned long long)i << 8) | (uint32_t)-o.st);
}

uint32_t blocks_of(uint64_t items, uint32_t per) { return (uint32_t)((items + per - 1) / per); }

int frame_call_begin(snappy_amd_ctx *c)
{
    HIP_OK(hipSetDevice(c->device));
    if (ctx_stream(c)) return SNAPPY_AMD_ERR_DEVICE;
    (void)hipGetLastError();  // (a pending error that is not this call's, as in compress_launch)
    return SNAPPY_AMD_OK;
}

void launch_kf1(snappy_amd_ctx *c, const void *d_base, const uint64_t *d_off_len, uint64_t count, uint64_t stride,
                uint64_t n, int masked, uint32_t *d_crc)
{
    hipLaunchKernelGGL(kf1_crc32c, dim3(blocks_of(count, kF1Waves)), dim3(64 * kF1Waves), 0, c->stream,
                       static_cast<const uint8_t *>(d_base), d_off_len, count, stride, n, masked ? 1u : 0u, d_crc);
}

}  // namespace

// KF1 for the range decode of framed streams (snappy_frame_ranges.hip; declared in snappy_kernels.h)
void snappy_amd::frame_launch_crc32c(hipStream_t stream, const void *d_base, const uint64_t *d_off_len, uint64_t count,
                                     int masked, uint32_t *d_crc)
{
    hipLaunchKernelGGL(kf1_crc32c, dim3(blocks_of(count, kF1Waves)), dim3(64 * kF1Waves), 0, stream,
                       static_cast<const uint8_t *>(d_base), d_off_len, count, 0ull, 0ull, masked ? 1u : 0u, d_crc);
}

extern "C" {

int snappy_amd_crc32c_device(snappy_amd_ctx *c, const void *d_base, const uint64_t *d_off_len, size_t count, int masked,
                             uint32_t *d_crc)
{
    if (!c || !d_off_len || !d_crc || count > 0xFFFFFFFFull) return SNAPPY_AMD_ERR_ARG;
    if (count == 0) return SNAPPY_AMD_OK;
    int rc = frame_call_begin(c);
    if (rc) return rc;
    launch_kf1(c, d_base, d_off_len, count, 0, 0, masked, d_crc);
    HIP_OK(hipGetLastError());
    return SNAPPY_AMD_OK;
}

size_t snappy_amd_max_frame_output_ex(size_t n, uint32_t chunk)
{
    if (chunk == 0 || chunk > SNAPPY_FRAME_CHUNK_MAX) return 0;
    const size_t units = (n + chunk - 1) / chunk;
    return SNAPPY_FRAME_IDENT_LEN + 8 * units + snappy_amd_max_output(n, chunk, SNAPPY_AMD_STREAMS);
}

size_t snappy_amd_max_frame_output(size_t n) { return snappy_amd_max_frame_output_ex(n, SNAPPY_AMD_BLOCK); }

namespace {
struct ChooseArgs {
    size_t n;
    uint32_t chunk;
    uint32_t *stored;
};

// `flags` checked by the caller; chunk in 1..65,536
int frame_compress_device(snappy_amd_ctx *c, const void *d_in, size_t n, uint32_t unit, uint32_t flags, void *d_out,
                          uint64_t *d_chunks, size_t *out_len)
{
    if (!c || (!d_in && n) || !d_out || !d_chunks) return SNAPPY_AMD_ERR_ARG;
    const size_t units = (n + unit - 1) / unit;
    if (units > 0x7FFFFFFFull) return SNAPPY_AMD_ERR_ARG;
    int rc = frame_call_begin(c);
    if (rc) return rc;
    const uint32_t ident = (flags & SNAPPY_AMD_FRAME_NO_IDENTIFIER) ? 0u : SNAPPY_FRAME_IDENT_LEN;
    const bool store = (flags & SNAPPY_AMD_FRAME_STORE) != 0;
    uint8_t *out = static_cast<uint8_t *>(d_out);
    uint64_t *f_off = nullptr;
    uint32_t *f_crc = nullptr, *f_stored = nullptr;
    if (units) {
        // scan offsets | CRCs | (FRAME_STORE) the chunks' stored words
        if ((rc = grow(reinterpret_cast<void **>(&c->f_meta), &c->f_meta_cap,
                       (units + 1) * sizeof(uint64_t) + units * sizeof(uint32_t) * (store ? 2 : 1))))
            return rc;
        f_off = reinterpret_cast<uint64_t *>(c->f_meta);
        f_crc = reinterpret_cast<uint32_t *>(f_off + units + 1);
        if (!store) {
            // STREAMS units of `unit` bytes, with kf2_bump between the match finder and the scan (KF2 above)
            auto bump = [](snappy_amd_ctx *cc, size_t nu, void *) {
                hipLaunchKernelGGL(kf2_bump, dim3(blocks_of(nu, 256)), dim3(256), 0, cc->stream, cc->sizes, (uint64_t)nu);
            };
            if ((rc = compress_launch(c, d_in, n, unit, SNAPPY_HDR_EVERY_UNIT, (uint64_t)n, f_off, out + ident + 8, bump)))
                return rc;
        } else {
            // kf2_choose there instead; K2 leaves the stored chunks' slots to kf2_store
            f_stored = f_crc + units;
            ChooseArgs a = {n, unit, f_stored};
            auto choose = [](snappy_amd_ctx *cc, size_t nu, void *arg) {
                const ChooseArgs *ca = static_cast<const ChooseArgs *>(arg);
                hipLaunchKernelGGL(kf2_choose, dim3(blocks_of(nu, 256)), dim3(256), 0, cc->stream, cc->sizes,
                                   (uint64_t)nu, (uint64_t)ca->n, ca->chunk, ca->stored);
            };
            if ((rc = compress_launch(c, d_in, n, unit, SNAPPY_HDR_EVERY_UNIT, (uint64_t)n, f_off, out + ident + 8, choose,
                                      &a, f_stored)))
                return rc;
        }
        launch_kf1(c, d_in, nullptr, units, unit, n, 1, f_crc);
        if (store) {
            const uint32_t rounds = (unit + kF2StoreSpan - 1) / kF2StoreSpan;
            hipLaunchKernelGGL(kf2_store, dim3((uint32_t)units, rounds > 3 ? kF2StoreParts : 1u), dim3(kF2StoreThreads), 0,
                               c->stream, static_cast<const uint8_t *>(d_in), (uint64_t)n, unit, f_stored, f_off, ident,
                               out);
        }
    }
    hipLaunchKernelGGL(kf2_headers, dim3(units ? blocks_of(units, 256) : 1u), dim3(256), 0, c->stream, out, ident,
                       f_off, c->sizes, f_crc, f_stored, (uint64_t)units, d_chunks);
    HIP_OK(hipGetLastError());
    if (out_len) {
        *c->h_total = 0;
        if (units) HIP_OK(hipMemcpyAsync(c->h_total, c->total, sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
        HIP_OK(hipStreamSynchronize(c->stream));
        *out_len = ident + (size_t)*c->h_total;
    }
    return SNAPPY_AMD_OK;
}
}  // namespace

int snappy_amd_compress_frame_device(snappy_amd_ctx *c, const void *d_in, size_t n, uint32_t flags, void *d_out,
                                     uint64_t *d_chunks, size_t *out_len)
{
    if (flags & ~SNAPPY_AMD_FRAME_NO_IDENTIFIER) return SNAPPY_AMD_ERR_ARG;
    return frame_compress_device(c, d_in, n, SNAPPY_AMD_BLOCK, flags, d_out, d_chunks, out_len);
}

int snappy_amd_compress_frame_device_ex(snappy_amd_ctx *c, const void *d_in, size_t n, uint32_t chunk, uint32_t flags,
                                        void *d_out, uint64_t *d_chunks, size_t *out_len)
{
    if (chunk == 0 || chunk > SNAPPY_FRAME_CHUNK_MAX) return SNAPPY_AMD_ERR_ARG;
    if (flags & ~(SNAPPY_AMD_FRAME_NO_IDENTIFIER | SNAPPY_AMD_FRAME_STORE)) return SNAPPY_AMD_ERR_ARG;
    return frame_compress_device(c, d_in, n, chunk, flags, d_out, d_chunks, out_len);
}

int snappy_amd_frame_index_device(snappy_amd_ctx *c, const void *d_frame, size_t clen, uint64_t *d_chunks,
                                  size_t max_chunks, size_t *nchunks_out, size_t *n_out)
{
    if (!c || (!d_frame && clen) || !d_chunks) return SNAPPY_AMD_ERR_ARG;
    int rc = frame_call_begin(c);
    if (rc) return rc;
    hipLaunchKernelGGL(kf3_walk, dim3(1), dim3(64), 0, c->stream, static_cast<const uint8_t *>(d_frame), (uint64_t)clen,
                       d_chunks, (uint64_t)max_chunks, 1u, c->k5res);
    HIP_OK(hipGetLastError());
    int64_t res[3];
    HIP_OK(hipMemcpyAsync(res, c->k5res, sizeof(res), hipMemcpyDeviceToHost, c->stream));
    HIP_OK(hipStreamSynchronize(c->stream));
    if (n_out) *n_out = (size_t)res[1];
    if (nchunks_out) *nchunks_out = (size_t)res[2];
    return (int)res[0];
}

int snappy_amd_frame_seek_device(snappy_amd_ctx *c, const void *d_frame, size_t clen, const uint64_t *d_chunks,
                                 size_t nchunks, uint64_t *d_starts, size_t *n_out)
{
    if (!c || (!d_frame && clen) || (!d_chunks && nchunks) || !d_starts || nchunks > 0x7FFFFFFFull)
        return SNAPPY_AMD_ERR_ARG;
    if (n_out) *n_out = 0;
    int rc = frame_call_begin(c);
    if (rc) return rc;
    // head (the first failure, the total) | info | lens
    const size_t nc = nchunks;
    if ((rc = grow(reinterpret_cast<void **>(&c->f_meta), &c->f_meta_cap, 64 + nc * (sizeof(FrameInfo) + 4)))) return rc;
    unsigned long long *d_head = reinterpret_cast<unsigned long long *>(c->f_meta);
    FrameInfo *d_info = reinterpret_cast<FrameInfo *>(c->f_meta + 64);
    uint32_t *d_lens = reinterpret_cast<uint32_t *>(d_info + nc);
    HIP_OK(hipMemsetAsync(d_head, 0xFF, sizeof(uint64_t), c->stream));
    if (nc) {
        hipLaunchKernelGGL(kf4_scan, dim3(blocks_of(nc, 256)), dim3(256), 0, c->stream,
                           static_cast<const uint8_t *>(d_frame), (uint64_t)clen, d_chunks, (uint64_t)nc, d_info);
        hipLaunchKernelGGL(kf5_seek_lens, dim3(blocks_of(nc, 256)), dim3(256), 0, c->stream, d_info, (uint64_t)nc,
                           d_lens, d_head);
    }
    // the exclusive scan of the lengths is the table; its total the decoded length
    if (nc <= SNAPPY_K3_WAVE_MAX)
        hipLaunchKernelGGL(k3_scan_wave, dim3(1), dim3(64), 0, c->stream, d_lens, (uint64_t)nc, d_starts,
                           reinterpret_cast<uint64_t *>(d_head + 1));
    else
        hipLaunchKernelGGL(k3_scan, dim3(1), dim3(1024), 0, c->stream, d_lens, (uint64_t)nc, d_starts,
                           reinterpret_cast<uint64_t *>(d_head + 1));
    HIP_OK(hipGetLastError());
    HIP_OK(hipMemcpyAsync(c->h_total, d_head, 2 * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
    HIP_OK(hipStreamSynchronize(c->stream));
    if (c->h_total[0] != ~0ull) return -(int)(c->h_total[0] & 0xFF);
    if (n_out) *n_out = (size_t)c->h_total[1];
    return SNAPPY_AMD_OK;
}

int snappy_amd_decompress_frame_device(snappy_amd_ctx *c, const void *d_frame, size_t clen, const uint64_t *d_chunks,
                                       size_t nchunks, void *d_out, size_t cap, size_t *n_out)
{
    if (!c || (!d_frame && clen) || !d_chunks || (!d_out && cap) || nchunks > 0x7FFFFFFFull) return SNAPPY_AMD_ERR_ARG;
    if (n_out) *n_out = 0;
    if (nchunks == 0) return SNAPPY_AMD_OK;
    int rc = frame_call_begin(c);
    if (rc) return rc;
    const uint8_t *f = static_cast<const uint8_t *>(d_frame);
    const size_t nc = nchunks;
    // one allocation (grow keeps no contents), laid out for at most nc units:
    // info | idx (units + 1) | cpos (units) | off_len (2 nc) | crc (nc) | status (units) | crc status (nc)
    if ((rc = grow(reinterpret_cast<void **>(&c->f_meta), &c->f_meta_cap, nc * 64 + 64))) return rc;
    FrameInfo *d_info = reinterpret_cast<FrameInfo *>(c->f_meta);
    hipLaunchKernelGGL(kf4_scan, dim3(blocks_of(nc, 256)), dim3(256), 0, c->stream, f, (uint64_t)clen, d_chunks,
                       (uint64_t)nc, d_info);
    HIP_OK(hipGetLastError());
    std::vector<FrameInfo> info(nc);
    HIP_OK(hipMemcpyAsync(info.data(), d_info, nc * sizeof(FrameInfo), hipMemcpyDeviceToHost, c->stream));
    HIP_OK(hipStreamSynchronize(c->stream));
    uint64_t total = 0, scratch = 0;
    size_t units = 0;
    for (size_t i = 0; i < nc; i++) {
        if (info[i].st != SNAPPY_AMD_OK) return info[i].st;  // the first failing chunk
        total += info[i].dlen;
        if (info[i].dlen) {
            units++;
            scratch += info[i].ssize;
        }
    }
    if (total > cap) return SNAPPY_AMD_ERR_CAPACITY;  // before any decode
    // tables of the units (chunks that decode to >= 1 byte) and of the CRC pass (every chunk)
    std::vector<uint64_t> tab(2 * units + 1 + 2 * nc);
    std::vector<uint32_t> unit_chunk(units);
    uint64_t *h_idx = tab.data(), *h_cpos = h_idx + units + 1, *h_ol = h_cpos + units;
    std::vector<uint64_t> chunks(nc);
    HIP_OK(hipMemcpyAsync(chunks.data(), d_chunks, nc * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
    HIP_OK(hipStreamSynchronize(c->stream));
    {
        uint64_t so = 0, oo = 0;
        size_t j = 0;
        for (size_t i = 0; i < nc; i++) {
            h_ol[2 * i] = oo;
            h_ol[2 * i + 1] = info[i].dlen;
            if (info[i].dlen) {
                h_idx[j] = so;
                h_cpos[j] = chunks[i];
                unit_chunk[j] = (uint32_t)i;
                so += info[i].ssize;
                j++;
            }
            oo += info[i].dlen;
        }
        h_idx[units] = so;
    }
    uint64_t *d_tab = reinterpret_cast<uint64_t *>(d_info + nc);
    uint64_t *d_idx = d_tab, *d_cpos = d_idx + units + 1, *d_ol = d_cpos + units;
    uint32_t *d_crc = reinterpret_cast<uint32_t *>(d_ol + 2 * nc);
    int32_t *d_st = reinterpret_cast<int32_t *>(d_crc + nc);  // units words, then nc words of CRC status
    int32_t *d_cst = d_st + units;
    if ((rc = grow(reinterpret_cast<void **>(&c->f_scr), &c->f_scr_cap, scratch + 16))) return rc;
    HIP_OK(hipMemcpyAsync(d_tab, tab.data(), tab.size() * sizeof(uint64_t), hipMemcpyHostToDevice, c->stream));
    HIP_OK(hipStreamSynchronize(c->stream));  // (tab is pageable: its bytes are taken before the call goes on)
    uint8_t *out = static_cast<uint8_t *>(d_out);
    if (units) {
        hipLaunchKernelGGL(kf4_gather, dim3(blocks_of(units, kF4Waves)), dim3(64 * kF4Waves), 0, c->stream, f, d_cpos,
                           d_idx, (uint64_t)units, c->f_scr);
        HIP_OK(hipGetLastError());
        // K4 puts unit u at u * unit and lets only the last be short: one launch per
        // maximal run of equal-length chunks plus at most one shorter closing chunk
        for (size_t j = 0; j < units;) {
            const uint32_t L = info[unit_chunk[j]].dlen;
            uint64_t bytes = 0;
            size_t k = j;
            for (; k < units && info[unit_chunk[k]].dlen == L; k++) bytes += L;
            if (k < units && info[unit_chunk[k]].dlen < L) bytes += info[unit_chunk[k++]].dlen;
            hipLaunchKernelGGL(k4_decompress_units, dim3((uint32_t)(k - j)), dim3(64), 0, c->stream,
                               static_cast<const uint8_t *>(c->f_scr), d_idx + j, bytes, L, (uint32_t)SNAPPY_HDR_EVERY_UNIT,
                               bytes, 0u, 0u, out + h_ol[2 * (size_t)unit_chunk[j]], d_st + j);
            HIP_OK(hipGetLastError());
            j = k;
        }
    }
    launch_kf1(c, out, d_ol, nc, 0, 0, 1, d_crc);
    hipLaunchKernelGGL(kf4_verify, dim3(blocks_of(nc, 256)), dim3(256), 0, c->stream, f, d_chunks, (uint64_t)nc, d_crc,
                       d_cst);
    HIP_OK(hipGetLastError());
    std::vector<int32_t> st(units + nc);
    HIP_OK(hipMemcpyAsync(st.data(), d_st, st.size() * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    HIP_OK(hipStreamSynchronize(c->stream));
    // the first failing chunk wins; its CRC counts only where its decode succeeded
    std::vector<int32_t> dec(nc, SNAPPY_AMD_OK);
    for (size_t j = 0; j < units; j++)
        // (a STREAMS unit left in K4's DEFER state copied from before its own start)
        dec[unit_chunk[j]] = st[j] > 0 ? SNAPPY_AMD_ERR_OFFSET : st[j];
    for (size_t i = 0; i < nc; i++) {
        if (dec[i] != SNAPPY_AMD_OK) return dec[i];
        if (st[units + i] != SNAPPY_AMD_OK) return st[units + i];
    }
    if (n_out) *n_out = (size_t)total;
    return SNAPPY_AMD_OK;
}

}  // extern "C"

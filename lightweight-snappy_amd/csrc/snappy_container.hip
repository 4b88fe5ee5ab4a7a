// snappy_container.hip -- Hadoop SnappyCodec and snappy-java SnappyOutputStream
// container streams on the device: big-endian 32-bit lengths in front of raw
// Snappy streams (include/snappy_amd.h).
//
//   KC1  kc1_walk    the header walk of a container (one wave, one hop per chunk)
//   KC2  kc2_plan    (n, block) -> the long-record descriptors of the pieces
//   KC3  kc3_place   headers + payloads from the scratch into the container,
//                    a wave per chunk; the chunk tables
//   KC4  kc4_check   a caller's chunk tables against the container's length
//
// The payloads are written by snappy_amd_compress_long_records_device and the
// chunks decoded by snappy_amd_decompress_long_records_device, both unchanged:
// a chunk is exactly one long record.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "snappy_amd.h"
#include "snappy_container.h"
#include "snappy_ctx.h"

namespace {

// ---------------------------------------------------------------------------
// KC1: the walk.  A dependent chain, one hop per step of snappy_container_step:
// the 16 bytes at the position come as the (up to five) aligned dwords that
// hold them, loaded in one round -- in Hadoop block header, chunk header and
// preamble together.  Every lane walks the same chain at a wave-uniform
// position.  A dword is loaded only if it holds a byte of [pos, clen): no byte
// outside [0, clen) is read but those sharing an aligned dword with the first
// or the last byte.  Past max_chunks the walk goes on counting without storing.
// result[0] = status, [1] = decoded bytes, [2] = chunks.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(64) void kc1_walk(const uint8_t *__restrict__ f, uint64_t clen, int format,
                                               uint64_t *__restrict__ comp, uint64_t *__restrict__ outp,
                                               uint64_t max_chunks, int64_t *__restrict__ result)
{
    uint64_t pos = 0, total = 0, count = 0, R = 0;
    int32_t st = SNAPPY_AMD_OK;
    int first = format == SNAPPY_AMD_CONTAINER_XERIAL;
    // the stream as aligned dwords: byte i of it is byte bias + i of fd
    const uint32_t bias = (uint32_t)(reinterpret_cast<uintptr_t>(f) & 3u);
    const uint32_t *__restrict__ fd = reinterpret_cast<const uint32_t *>(f - bias);
    while (pos < clen) {
        const uint64_t avail = clen - pos;
        // the dwords of [pos, lim): five unconditional loads in one round, a dword past
        // the last one replaced by the last one (a load behind a condition would be
        // waited for on its own: five round trips per hop)
        const uint64_t lim = avail < SNAPPY_CONTAINER_WINDOW ? clen : pos + SNAPPY_CONTAINER_WINDOW;
        const uint64_t q = (bias + pos) >> 2, last = (bias + lim - 1) >> 2;
        uint32_t d[5];
#pragma unroll
        for (uint32_t j = 0; j < 5; j++) d[j] = fd[q + j < last ? q + j : last];
        const uint32_t sh = 8u * ((bias + (uint32_t)pos) & 3u);
        uint32_t x[4];
#pragma unroll
        for (uint32_t j = 0; j < 4; j++) {
            x[j] = (uint32_t)((((uint64_t)d[j + 1] << 32) | d[j]) >> sh);
            // zero from `avail` on, as snappy_container_window leaves it
            const uint64_t left = avail > 4u * j ? avail - 4u * j : 0u;
            if (left < 4u) x[j] &= (1u << (8u * (uint32_t)left)) - 1u;
        }
        uint32_t coff, cl, dlen;
        uint64_t adv;
        const int r = snappy_container_step(x, avail, format, first, &R, &coff, &cl, &dlen, &adv);
        if (r < 0) {
            st = r;
            break;
        }
        first = 0;
        if (r == 1) {
            if (count < max_chunks && threadIdx.x == 0) {
                if (comp) {
                    comp[2 * count] = pos + coff;
                    comp[2 * count + 1] = cl;
                }
                if (outp) {
                    outp[2 * count] = total;
                    outp[2 * count + 1] = dlen;
                }
            }
            count++;
            total += dlen;
        }
        // (every lane holds the same position: say so, and the loads stay uniform)
        pos += adv;
        pos = ((uint64_t)__builtin_amdgcn_readfirstlane((uint32_t)(pos >> 32)) << 32) |
              (uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)pos);
    }
    if (st == SNAPPY_AMD_OK) st = snappy_container_end(format, first, R);
    if (st == SNAPPY_AMD_OK && count > max_chunks) st = SNAPPY_AMD_ERR_CAPACITY;
    if (threadIdx.x == 0) {
        result[0] = st;
        result[1] = (int64_t)total;
        result[2] = (int64_t)count;
    }
}

// ---------------------------------------------------------------------------
// KC2: piece i of the input = the long record (i block, min(block, n - i block))
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void kc2_plan(uint64_t n, uint64_t block, uint64_t chunks, uint64_t *__restrict__ desc)
{
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= chunks) return;
    const uint64_t off = i * block;
    desc[2 * i] = off;
    desc[2 * i + 1] = n - off < block ? n - off : block;
}

// dst[0, n) = src[0, n), one wave; 16-byte stores on the aligned middle
__device__ __forceinline__ void wave_copy(uint8_t *dst, const uint8_t *src, uint64_t n, uint32_t lane)
{
    uint64_t head = (16u - (uint32_t)(reinterpret_cast<uintptr_t>(dst) & 15u)) & 15u;
    if (head > n) head = n;
    if (lane < head) dst[lane] = src[lane];
    dst += head;
    src += head;
    n -= head;
    const uint64_t nv = n >> 4;
    for (uint64_t i = lane; i < nv; i += 64) {
        uint4 v;
        __builtin_memcpy(&v, src + 16 * i, 16);
        *reinterpret_cast<uint4 *>(dst + 16 * i) = v;
    }
    for (uint64_t i = 16 * nv + lane; i < n; i += 64) dst[i] = src[i];
}

__device__ __forceinline__ void put_be32(uint8_t *p, uint32_t v)
{
    p[0] = (uint8_t)(v >> 24);
    p[1] = (uint8_t)(v >> 16);
    p[2] = (uint8_t)(v >> 8);
    p[3] = (uint8_t)v;
}

constexpr uint32_t kC3Waves = 4;

// ---------------------------------------------------------------------------
// KC3: one wave per chunk.  The long-record call left payload i at scr +
// offsets[i]; headers have a fixed size (hdr: 8 Hadoop, 4 snappy-java), so chunk
// i stands at ident + hdr i + offsets[i] and no scan is needed.  Lane 0 writes
// the header with byte stores (any alignment) and the table pairs; the wave
// copies the payload.  Chunk 0's wave also writes the stream header.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(64 * kC3Waves) void kc3_place(const uint8_t *__restrict__ scr,
                                                           const uint64_t *__restrict__ offsets,
                                                           const uint64_t *__restrict__ desc, uint64_t chunks,
                                                           int format, uint32_t ident, uint8_t *__restrict__ out,
                                                           uint64_t *__restrict__ comp, uint64_t *__restrict__ outp)
{
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t i = (uint64_t)blockIdx.x * kC3Waves + (threadIdx.x >> 6);
    if (i == 0 && lane == 0 && ident) {
        for (uint32_t k = 0; k < 8; k++) out[k] = (uint8_t)(SNAPPY_CONTAINER_MAGIC >> (8 * k));
        put_be32(out + 8, 1u);
        put_be32(out + 12, 1u);
    }
    if (i >= chunks) return;
    const uint32_t hdr = snappy_container_chunk_header(format);
    const uint64_t so = offsets[i], c = offsets[i + 1] - so, L = desc[2 * i + 1];
    uint8_t *h = out + ident + hdr * i + so;
    if (lane == 0) {
        if (format == SNAPPY_AMD_CONTAINER_HADOOP) {
            put_be32(h, (uint32_t)L);
            put_be32(h + 4, (uint32_t)c);
        } else {
            put_be32(h, (uint32_t)c);
        }
        if (comp) {
            comp[2 * i] = ident + hdr * (i + 1) + so;
            comp[2 * i + 1] = c;
        }
        if (outp) {
            outp[2 * i] = desc[2 * i];
            outp[2 * i + 1] = L;
        }
    }
    wave_copy(h + hdr, scr + so, c, lane);
}

// ---------------------------------------------------------------------------
// KC4: one thread per pair of a caller's tables.  res[0] = min over failing
// chunks of chunk << 8 | -status (~0: none), res[1] = the end of the last
// output range.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void kc4_check(const uint64_t *__restrict__ comp, const uint64_t *__restrict__ outp,
                                                 uint64_t nchunks, uint64_t clen, unsigned long long *__restrict__ res)
{
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= nchunks) return;
    const uint64_t co = comp[2 * i], cl = comp[2 * i + 1], oo = outp[2 * i], ol = outp[2 * i + 1];
    int32_t st = SNAPPY_AMD_OK;
    if (co > clen || cl > clen - co) st = SNAPPY_AMD_ERR_TRUNCATED;
    else if (cl == 0) st = SNAPPY_AMD_ERR_HEADER;
    else if (ol > SNAPPY_CONTAINER_CHUNK_MAX) st = SNAPPY_AMD_ERR_UNSUPPORTED;
    if (st != SNAPPY_AMD_OK) {
        atomicMin(&res[0], (unsigned long long)((i << 8) | (uint32_t)-st));
    } else {
        const uint64_t end = oo + ol < oo ? ~0ull : oo + ol;
        atomicMax(&res[1], (unsigned long long)end);
    }
}

uint32_t blocks_of(uint64_t items, uint32_t per) { return (uint32_t)((items + per - 1) / per); }

int call_begin(snappy_amd_ctx *c)
{
    HIP_OK(hipSetDevice(c->device));
    if (ctx_stream(c)) return SNAPPY_AMD_ERR_DEVICE;
    (void)hipGetLastError();  // (a pending error that is not this call's, as in compress_launch)
    return SNAPPY_AMD_OK;
}

bool known(int format) { return format == SNAPPY_AMD_CONTAINER_HADOOP || format == SNAPPY_AMD_CONTAINER_XERIAL; }

uint32_t block_of(uint32_t block, int format)
{
    if (block) return block;
    return format == SNAPPY_AMD_CONTAINER_HADOOP ? SNAPPY_CONTAINER_HADOOP_BLOCK : SNAPPY_CONTAINER_XERIAL_BLOCK;
}

// the walk into the given tables; res = status, decoded bytes, chunks
int walk(snappy_amd_ctx *c, const void *d_cont, size_t clen, int format, uint64_t *d_comp, uint64_t *d_outp,
         size_t max_chunks, int64_t res[3])
{
    hipLaunchKernelGGL(kc1_walk, dim3(1), dim3(64), 0, c->stream, static_cast<const uint8_t *>(d_cont), (uint64_t)clen,
                       format, d_comp, d_outp, (uint64_t)max_chunks, c->k5res);
    HIP_OK(hipGetLastError());
    HIP_OK(hipMemcpyAsync(res, c->k5res, 3 * sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
    HIP_OK(hipStreamSynchronize(c->stream));
    return SNAPPY_AMD_OK;
}

}  // namespace

extern "C" {

size_t snappy_amd_max_container_output(size_t n, uint32_t block, int format)
{
    if (!known(format) || block > SNAPPY_CONTAINER_CHUNK_MAX) return 0;
    const size_t b = block_of(block, format), chunks = (n + b - 1) / b;
    return snappy_container_stream_header(format, 0) + snappy_container_chunk_header(format) * chunks +
           snappy_amd_max_long_records_output(n, chunks);
}

int snappy_amd_compress_container_device(snappy_amd_ctx *c, const void *d_in, size_t n, uint32_t block, int format,
                                         uint32_t flags, void *d_out, size_t out_cap, uint64_t *d_comp_off_len,
                                         uint64_t *d_out_off_len, size_t chunks_cap, size_t *nchunks, size_t *out_len)
{
    if (!c || (!d_in && n) || !d_out || !known(format) || block > SNAPPY_CONTAINER_CHUNK_MAX ||
        (flags & ~SNAPPY_AMD_CONTAINER_NO_HEADER))
        return SNAPPY_AMD_ERR_ARG;
    const size_t b = block_of(block, format), chunks = (n + b - 1) / b;
    if (chunks > 0x7FFFFFFFull) return SNAPPY_AMD_ERR_ARG;
    if (out_cap < snappy_amd_max_container_output(n, block, format)) return SNAPPY_AMD_ERR_CAPACITY;
    if ((d_comp_off_len || d_out_off_len) && chunks_cap < chunks) return SNAPPY_AMD_ERR_CAPACITY;
    int rc = call_begin(c);
    if (rc) return rc;
    const uint32_t ident = snappy_container_stream_header(format, flags);
    const uint32_t hdr = snappy_container_chunk_header(format);
    uint64_t *desc = nullptr, *offsets = nullptr;
    if (chunks) {
        // f_meta: the pieces' descriptors (2 chunks) | the payloads' offsets in the scratch (chunks + 1)
        const size_t scr_cap = snappy_amd_max_long_records_output(n, chunks);
        if ((rc = grow(reinterpret_cast<void **>(&c->f_meta), &c->f_meta_cap, (3 * chunks + 1) * sizeof(uint64_t))))
            return rc;
        if ((rc = grow(reinterpret_cast<void **>(&c->f_scr), &c->f_scr_cap, scr_cap))) return rc;
        desc = reinterpret_cast<uint64_t *>(c->f_meta);
        offsets = desc + 2 * chunks;
        hipLaunchKernelGGL(kc2_plan, dim3(blocks_of(chunks, 256)), dim3(256), 0, c->stream, (uint64_t)n, (uint64_t)b,
                           (uint64_t)chunks, desc);
        HIP_OK(hipGetLastError());
        if ((rc = snappy_amd_compress_long_records_device(c, d_in, n, desc, chunks, c->f_scr, scr_cap, offsets, nullptr, 0,
                                                          nullptr, nullptr)))
            return rc;
    }
    if (chunks || ident) {
        hipLaunchKernelGGL(kc3_place, dim3(chunks ? blocks_of(chunks, kC3Waves) : 1u), dim3(64 * kC3Waves), 0, c->stream,
                           c->f_scr, offsets, desc, (uint64_t)chunks, format, ident, static_cast<uint8_t *>(d_out),
                           d_comp_off_len, d_out_off_len);
        HIP_OK(hipGetLastError());
    }
    if (nchunks) *nchunks = chunks;
    if (out_len) {
        *c->h_total = 0;
        if (chunks) HIP_OK(hipMemcpyAsync(c->h_total, offsets + chunks, sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
        HIP_OK(hipStreamSynchronize(c->stream));
        *out_len = ident + (size_t)hdr * chunks + (size_t)*c->h_total;
    }
    return SNAPPY_AMD_OK;
}

int snappy_amd_container_index_device(snappy_amd_ctx *c, const void *d_cont, size_t clen, int format,
                                      uint64_t *d_comp_off_len, uint64_t *d_out_off_len, size_t max_chunks,
                                      size_t *nchunks, size_t *n_out)
{
    if (!c || (!d_cont && clen) || !known(format)) return SNAPPY_AMD_ERR_ARG;
    int rc = call_begin(c);
    if (rc) return rc;
    int64_t res[3];
    if ((rc = walk(c, d_cont, clen, format, d_comp_off_len, d_out_off_len, max_chunks, res))) return rc;
    if (n_out) *n_out = (size_t)res[1];
    if (nchunks) *nchunks = (size_t)res[2];
    return (int)res[0];
}

int snappy_amd_decompress_container_device(snappy_amd_ctx *c, const void *d_cont, size_t clen, int format,
                                           const uint64_t *d_comp_off_len, const uint64_t *d_out_off_len,
                                           size_t nchunks, void *d_out, size_t cap, size_t *n_out)
{
    if (!c || (!d_cont && clen) || (!d_out && cap) || !known(format) || (!d_comp_off_len) != (!d_out_off_len) ||
        nchunks > 0x7FFFFFFFull)
        return SNAPPY_AMD_ERR_ARG;
    if (n_out) *n_out = 0;
    int rc = call_begin(c);
    if (rc) return rc;
    const uint64_t *comp = d_comp_off_len, *outp = d_out_off_len;
    uint64_t total = 0;
    if (!comp) {
        // stage 1, no tables: the walk into f_meta.  The room is a guess (a chunk per
        // KiB); a stream of smaller chunks says how many it has and is walked again.
        size_t room = clen / 1024 + 1024;
        for (int pass = 0;; pass++) {
            if ((rc = grow(reinterpret_cast<void **>(&c->f_meta), &c->f_meta_cap, 4 * room * sizeof(uint64_t)))) return rc;
            uint64_t *t = reinterpret_cast<uint64_t *>(c->f_meta);
            int64_t res[3];
            if ((rc = walk(c, d_cont, clen, format, t, t + 2 * room, room, res))) return rc;
            if (res[0] == SNAPPY_AMD_ERR_CAPACITY && pass == 0) {
                room = (size_t)res[2];
                continue;
            }
            if (res[0]) return (int)res[0];
            total = (uint64_t)res[1];
            nchunks = (size_t)res[2];
            comp = t;
            outp = t + 2 * room;
            break;
        }
        if (nchunks > 0x7FFFFFFFull) return SNAPPY_AMD_ERR_UNSUPPORTED;
    } else if (nchunks) {
        // stage 1, the caller's tables: every pair against clen
        unsigned long long *res = reinterpret_cast<unsigned long long *>(c->k5res);
        HIP_OK(hipMemsetAsync(res, 0xFF, sizeof(uint64_t), c->stream));
        HIP_OK(hipMemsetAsync(res + 1, 0, sizeof(uint64_t), c->stream));
        hipLaunchKernelGGL(kc4_check, dim3(blocks_of(nchunks, 256)), dim3(256), 0, c->stream, comp, outp,
                           (uint64_t)nchunks, (uint64_t)clen, res);
        HIP_OK(hipGetLastError());
        uint64_t h[2];
        HIP_OK(hipMemcpyAsync(h, res, sizeof(h), hipMemcpyDeviceToHost, c->stream));
        HIP_OK(hipStreamSynchronize(c->stream));
        if (h[0] != ~0ull) return -(int)(h[0] & 0xFF);
        total = h[1];
    }
    if (total > cap) return SNAPPY_AMD_ERR_CAPACITY;  // before any decode
    if (nchunks) {
        // stage 2: the chunks as one long-record batch, block tables built by the decoder
        if ((rc = snappy_amd_decompress_long_records_device(c, d_cont, clen, comp, nchunks, d_out, (size_t)total, outp,
                                                            nullptr, nullptr, 1)))
            return rc;
    }
    if (n_out) *n_out = (size_t)total;
    return SNAPPY_AMD_OK;
}

}  // extern "C"

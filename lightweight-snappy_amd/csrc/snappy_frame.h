// snappy_frame.h -- the chunk rules of the Snappy framing format
// (framing_format.txt of google/snappy), shared by the device walk (KF3,
// snappy_frame.hip) and the host walk (snappy_frame_host.cpp) so both accept
// and refuse exactly the same streams.  Private: not part of the C ABI.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "snappy_amd.h"

#if defined(__HIPCC__)
#define SNAPPY_FRAME_FN __host__ __device__ static inline
#else
#define SNAPPY_FRAME_FN static inline
#endif

#define SNAPPY_FRAME_IDENT_LEN 10u
#define SNAPPY_FRAME_CHUNK_MAX 65536u  // uncompressed bytes of one data chunk
#define SNAPPY_FRAME_WINDOW 16u        // bytes of a chunk one step looks at

#if defined(__HIPCC__)
// dst[0, n) = src[0, n), one wave; 16-byte stores on the aligned middle (the payload
// copies of the unframe pass and of the range decode's stored chunks)
__device__ __forceinline__ void snappy_frame_wave_copy(uint8_t *dst, const uint8_t *src, uint32_t n, uint32_t lane)
{
    uint32_t head = (16u - (uint32_t)(reinterpret_cast<uintptr_t>(dst) & 15u)) & 15u;
    if (head > n) head = n;
    if (lane < head) dst[lane] = src[lane];
    dst += head;
    src += head;
    n -= head;
    const uint32_t nv = n >> 4;
    for (uint32_t i = lane; i < nv; i += 64) {
        uint4 v;
        __builtin_memcpy(&v, src + 16 * (size_t)i, 16);
        *reinterpret_cast<uint4 *>(dst + 16 * (size_t)i) = v;
    }
    for (uint32_t i = 16 * nv + lane; i < n; i += 64) dst[i] = src[i];
}
#endif

// varint(v) and literal-tag lengths for v <= 65536 (an uncompressed chunk
// rewritten as a raw stream: varint(len) ++ one literal element)
SNAPPY_FRAME_FN uint32_t snappy_frame_varint_len(uint32_t v) { return v < 128u ? 1u : v < 16384u ? 2u : 3u; }
SNAPPY_FRAME_FN uint32_t snappy_frame_literal_tag_len(uint32_t len) { return len <= 60u ? 1u : len <= 256u ? 2u : 3u; }

// varint preamble of a compressed chunk's payload: w[0..have) are its first
// bytes (have <= 5).  Returns the bytes used, 0 if it does not end in them.
SNAPPY_FRAME_FN uint32_t snappy_frame_preamble(const uint8_t *w, uint32_t have, uint32_t *value)
{
    uint64_t v = 0;
    for (uint32_t k = 0; k < have && k < 5u; k++) {
        v |= (uint64_t)(w[k] & 0x7Fu) << (7u * k);
        if (!(w[k] & 0x80u)) {
            *value = v > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)v;
            return k + 1u;
        }
    }
    return 0;
}

// The store rule of the compressor under SNAPPY_AMD_FRAME_STORE (the device's
// kf2_choose; any host code that has to predict a stream): a chunk of R input
// bytes whose raw stream (preamble included) has P bytes is written stored
// (type 01) iff the stream is not one eighth smaller than the bytes.
SNAPPY_FRAME_FN int snappy_frame_store_chunk(uint32_t R, uint32_t P) { return P >= R - R / 8u; }

// One step of the chunk walk.  w = the first 16 bytes of the chunk at the
// walk's position (zero past the stream's end), avail = stream bytes from that
// position on (> 0), first = the stream identifier is still owed.  Returns a
// negative SNAPPY_AMD_ERR_*, 0 for a chunk that holds no data (identifier,
// padding, skippable) or 1 for a data chunk, whose decoded length goes to
// *dlen; *adv = the chunk's bytes, header included.
SNAPPY_FRAME_FN int snappy_frame_chunk(const uint8_t *w, uint64_t avail, int first, uint32_t *dlen, uint64_t *adv)
{
    *dlen = 0;
    *adv = 0;
    if (avail < 4u) return SNAPPY_AMD_ERR_TRUNCATED;
    const uint32_t type = w[0];
    const uint32_t len = (uint32_t)w[1] | ((uint32_t)w[2] << 8) | ((uint32_t)w[3] << 16);
    if (first && type != 0xFFu) return SNAPPY_AMD_ERR_HEADER;
    if (type == 0xFFu) {
        if (len != 6u) return SNAPPY_AMD_ERR_HEADER;
        if (avail < SNAPPY_FRAME_IDENT_LEN) return SNAPPY_AMD_ERR_TRUNCATED;
        if (w[4] != 0x73u || w[5] != 0x4Eu || w[6] != 0x61u || w[7] != 0x50u || w[8] != 0x70u || w[9] != 0x59u)
            return SNAPPY_AMD_ERR_HEADER;
        *adv = SNAPPY_FRAME_IDENT_LEN;
        return 0;
    }
    if (type >= 0x02u && type <= 0x7Fu) return SNAPPY_AMD_ERR_UNSUPPORTED;
    if (type >= 0x80u) {  // skippable (0x80..0xfd) and padding (0xfe)
        if (avail - 4u < len) return SNAPPY_AMD_ERR_TRUNCATED;
        *adv = 4ull + len;
        return 0;
    }
    if (len < 4u) return SNAPPY_AMD_ERR_HEADER;  // no room for the CRC
    if (avail - 4u < len) return SNAPPY_AMD_ERR_TRUNCATED;
    uint32_t d = len - 4u;
    if (type == 0x00u) {
        const uint32_t have = d < 5u ? d : 5u;
        if (snappy_frame_preamble(w + 8, have, &d) == 0) return SNAPPY_AMD_ERR_HEADER;
    }
    if (d > SNAPPY_FRAME_CHUNK_MAX) return SNAPPY_AMD_ERR_OVERRUN;
    *dlen = d;
    *adv = 4ull + len;
    return 1;
}

// snappy_container.h -- the walk rule of the two length-prefixed Snappy
// containers: Hadoop's SnappyCodec blocks and snappy-java's
// SnappyOutputStream chunks.  Shared by the device walk (KC1,
// snappy_container.hip) and the host walk (snappy_container_host.cpp) so both
// accept and refuse exactly the same streams; compiles as C and as HIP device
// code.  Private: not part of the C ABI.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "snappy_amd.h"

#if defined(__HIPCC__)
#define SNAPPY_CONTAINER_FN __host__ __device__ static inline
#else
#define SNAPPY_CONTAINER_FN static inline
#endif

#define SNAPPY_CONTAINER_WINDOW 16u      // bytes of the stream one step looks at
#define SNAPPY_CONTAINER_HEADER_LEN 16u  // snappy-java: magic, version, compatible version
#define SNAPPY_CONTAINER_CHUNK_MAX (1u << 30)  // decoded bytes of one chunk (SNAPPY_AMD_LONG_RECORD_MAX)
// 82 53 4e 41 50 50 59 00 and its first four bytes, as little-endian words
#define SNAPPY_CONTAINER_MAGIC 0x00595050414e5382ull
#define SNAPPY_CONTAINER_MAGIC4 0x414e5382u
#define SNAPPY_CONTAINER_HADOOP_BLOCK 131072u  // the compressor's default pieces
#define SNAPPY_CONTAINER_XERIAL_BLOCK 32768u

// bytes in front of each chunk's payload as this library writes it (Hadoop: one
// block per chunk, raw_len + comp_len) and in front of the first chunk
SNAPPY_CONTAINER_FN uint32_t snappy_container_chunk_header(int format) { return format == SNAPPY_AMD_CONTAINER_HADOOP ? 8u : 4u; }
SNAPPY_CONTAINER_FN uint32_t snappy_container_stream_header(int format, uint32_t flags)
{
    return format == SNAPPY_AMD_CONTAINER_XERIAL && !(flags & SNAPPY_AMD_CONTAINER_NO_HEADER) ? SNAPPY_CONTAINER_HEADER_LEN : 0u;
}

// the big-endian value of four stream bytes held as one little-endian word
SNAPPY_CONTAINER_FN uint32_t snappy_container_be32(uint32_t le)
{
    return (le >> 24) | ((le >> 8) & 0xFF00u) | ((le << 8) & 0xFF0000u) | (le << 24);
}

// x[0..4) = the 16 bytes at p as little-endian words, zero from `avail` on
SNAPPY_CONTAINER_FN void snappy_container_window(const uint8_t *p, uint64_t avail, uint32_t x[4])
{
    for (uint32_t j = 0; j < 4u; j++) {
        uint32_t v = 0;
        for (uint32_t b = 0; b < 4u; b++)
            if (4u * j + b < avail) v |= (uint32_t)p[4u * j + b] << (8u * b);
        x[j] = v;
    }
}

// One step of the walk.  x = the window at the walk's position (above), avail =
// stream bytes from that position on (> 0), first = the snappy-java header is
// still owed, *R = bytes left in the current Hadoop block.  Returns a negative
// SNAPPY_AMD_ERR_*, 0 for a step that holds no chunk (a snappy-java header, a
// Hadoop block of raw_len 0) or 1 for a chunk: its payload is the *clen bytes
// *coff bytes behind the position and decodes to *dlen bytes.  *adv = the bytes
// of the step; *R changes only with a chunk (a step that fails leaves the state
// as it found it, so a reader with more bytes coming repeats the step).
SNAPPY_CONTAINER_FN int snappy_container_step(const uint32_t x[4], uint64_t avail, int format, int first, uint64_t *R,
                                              uint32_t *coff, uint32_t *clen, uint32_t *dlen, uint64_t *adv)
{
    *coff = 0;
    *clen = 0;
    *dlen = 0;
    *adv = 0;
    uint64_t r = *R;
    uint32_t k = 0;
    if (format == SNAPPY_AMD_CONTAINER_XERIAL) {
        if (first || (avail >= 4u && x[0] == SNAPPY_CONTAINER_MAGIC4)) {
            const uint64_t m = (uint64_t)x[0] | ((uint64_t)x[1] << 32);
            const uint64_t mask = avail >= 8u ? ~0ull : (1ull << (8u * (uint32_t)avail)) - 1u;
            if ((m ^ SNAPPY_CONTAINER_MAGIC) & mask) return SNAPPY_AMD_ERR_HEADER;
            if (avail < SNAPPY_CONTAINER_HEADER_LEN) return SNAPPY_AMD_ERR_TRUNCATED;
            if (snappy_container_be32(x[3]) > 1u) return SNAPPY_AMD_ERR_UNSUPPORTED;  // compatible_version
            *adv = SNAPPY_CONTAINER_HEADER_LEN;
            return 0;
        }
    } else if (r == 0) {
        if (avail < 4u) return SNAPPY_AMD_ERR_TRUNCATED;
        r = snappy_container_be32(x[0]);  // raw_len
        if (r == 0) {
            *adv = 4u;
            return 0;
        }
        k = 4u;
    }
    // the chunk rule, at byte k of the window
    if (avail - k < 4u) return SNAPPY_AMD_ERR_TRUNCATED;
    const uint32_t c = snappy_container_be32(k ? x[1] : x[0]);
    if (c == 0) return SNAPPY_AMD_ERR_HEADER;
    if (avail - k - 4u < c) return SNAPPY_AMD_ERR_TRUNCATED;
    // the preamble: LEB128 as snappy_varint_decode reads it, ending inside the
    // chunk's first five bytes (a longer one cannot hold a length <= 2^30)
    const uint64_t pw = k ? ((uint64_t)x[2] | ((uint64_t)x[3] << 32)) : ((uint64_t)x[1] | ((uint64_t)x[2] << 32));
    const uint32_t have = c < 5u ? c : 5u;
    uint64_t L = 0;
    int ended = 0;
    for (uint32_t i = 0; i < 5u; i++) {
        const uint32_t b = (uint32_t)(pw >> (8u * i)) & 0xFFu;
        if (i < have && !ended) {
            L |= (uint64_t)(b & 0x7Fu) << (7u * i);
            if (!(b & 0x80u)) ended = 1;
        }
    }
    if (!ended) return SNAPPY_AMD_ERR_HEADER;
    if (L > SNAPPY_CONTAINER_CHUNK_MAX) return SNAPPY_AMD_ERR_UNSUPPORTED;
    if (format == SNAPPY_AMD_CONTAINER_HADOOP) {
        if (L > r) return SNAPPY_AMD_ERR_OVERRUN;
        *R = r - L;
    }
    *coff = k + 4u;
    *clen = c;
    *dlen = (uint32_t)L;
    *adv = (uint64_t)k + 4u + c;
    return 1;
}

// The end of the input at a step boundary: a snappy-java stream without its
// header (an empty input) and a Hadoop block with bytes still owed are refused.
SNAPPY_CONTAINER_FN int snappy_container_end(int format, int first, uint64_t R)
{
    if (format == SNAPPY_AMD_CONTAINER_XERIAL) return first ? SNAPPY_AMD_ERR_HEADER : SNAPPY_AMD_OK;
    return R ? SNAPPY_AMD_ERR_TRUNCATED : SNAPPY_AMD_OK;
}

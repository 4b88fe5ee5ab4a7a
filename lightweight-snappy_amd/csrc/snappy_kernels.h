// snappy_kernels.h -- private declarations shared by the HIP kernels and
// the extern "C" device shim.  Not part of the public C ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "snappy_ranges.h"

#define SNAPPY_LAYOUT_SINGLE 0
#define SNAPPY_LAYOUT_STREAMS 1
#define SNAPPY_BLOCK 65536u

// which units carry a varint preamble
#define SNAPPY_HDR_NONE 0        // a SINGLE-layout shard continuing a stream
#define SNAPPY_HDR_FIRST_UNIT 1  // unit 0 = start of a SINGLE stream
#define SNAPPY_HDR_EVERY_UNIT 2  // STREAMS layout: every unit is a stream
// (long records pass FIRST_UNIT for block 0 of a record and NONE for its other blocks:
// at the record entry points the mode is the unit's own, whatever its number)

// per-unit status values (same numbers as SNAPPY_AMD_ERR_* in snappy_amd.h)
#define SNAPPY_ST_OK 0
#define SNAPPY_ST_HEADER (-2)
#define SNAPPY_ST_TRUNCATED (-3)
#define SNAPPY_ST_OFFSET (-4)
#define SNAPPY_ST_OVERRUN (-5)
#define SNAPPY_ST_CAPACITY (-6)
#define SNAPPY_ST_UNSUPPORTED (-9)
#define SNAPPY_ST_TIMEOUT (-10)   // K4 pass 2: a unit waited too long for an earlier one
#define SNAPPY_ST_INDEX (-11)     // K4 (SINGLE): the unit's element chain does not end at the next index entry
#define SNAPPY_ST_DEPENDENT (-13) // range decode (SINGLE): the unit needs bytes of an earlier block; no pass 2 there
#define SNAPPY_ST_DEFER 2         // K4 pass 1: the unit copies from earlier units (pass 2 decodes it;
                                  // meanwhile its status is DEFER + output bytes already in HBM)

namespace snappy_amd {

__global__ void k1r_match_units(const uint8_t *__restrict__ in, uint64_t n, uint32_t unit, uint32_t hdr_mode,
                                uint64_t header_value, uint2 *__restrict__ tokens, uint32_t tok_cap,
                                uint32_t *__restrict__ ntok_out, uint32_t *__restrict__ sizes,
                                uint32_t *__restrict__ seg_off, uint32_t segs);
__global__ void k1r_match_units64(const uint8_t *__restrict__ in, uint64_t n, uint32_t unit, uint32_t hdr_mode,
                                uint64_t header_value, uint2 *__restrict__ tokens, uint32_t tok_cap,
                                uint32_t *__restrict__ ntok_out, uint32_t *__restrict__ sizes,
                                uint32_t *__restrict__ seg_off, uint32_t segs);
__global__ void k2_emit_units(const uint8_t *__restrict__ in, uint64_t n, uint32_t unit, uint32_t hdr_mode,
                              uint64_t header_value, const uint2 *__restrict__ tokens, uint32_t tok_cap,
                              const uint32_t *__restrict__ ntok, const uint32_t *__restrict__ seg_off, uint32_t segs,
                              const uint64_t *__restrict__ offsets, uint8_t *__restrict__ out);
// k2_emit_units, but a unit with skip[u] != 0 writes nothing (the framed compressor's stored chunks)
__global__ void k2_emit_units_sel(const uint8_t *__restrict__ in, uint64_t n, uint32_t unit, uint32_t hdr_mode,
                                  uint64_t header_value, const uint2 *__restrict__ tokens, uint32_t tok_cap,
                                  const uint32_t *__restrict__ ntok, const uint32_t *__restrict__ seg_off,
                                  uint32_t segs, const uint64_t *__restrict__ offsets, uint8_t *__restrict__ out,
                                  const uint32_t *__restrict__ skip);
// K2 segments: 256 tokens (4 per lane); waves per unit
#ifndef SNAPPY_K2_SEG
#define SNAPPY_K2_SEG 256u
#endif
#ifndef SNAPPY_K2_WAVES
#define SNAPPY_K2_WAVES 8u
#endif
// register-resident K1r handles units up to this size (128 VGPRs x 64 lanes x 4 B)
#define SNAPPY_K1R_MAX_UNIT 32768u

__global__ void k3_scan(const uint32_t *__restrict__ sizes, uint64_t count, uint64_t *__restrict__ offsets,
                        uint64_t *__restrict__ total);
// one-wave K3 for launches of at most SNAPPY_K3_WAVE_MAX units
__global__ void k3_scan_wave(const uint32_t *__restrict__ sizes, uint64_t count, uint64_t *__restrict__ offsets,
                             uint64_t *__restrict__ total);
#define SNAPPY_K3_WAVE_MAX 8192u
// K4: comp is 4-byte aligned, the stream starts at comp + bias (bias < 4).
// K4 pass 1: every unit; allow_back = 1 for SINGLE-layout streams (straddling
// elements and copies into earlier blocks are legal: such units end with
// status SNAPPY_ST_DEFER, for pass 2, and set status[units + 1])
__global__ void k4_decompress_units(const uint8_t *__restrict__ comp, const uint64_t *__restrict__ offsets,
                                    uint64_t n, uint32_t unit, uint32_t hdr_mode, uint64_t header_value,
                                    uint32_t allow_back, uint32_t bias, uint8_t *__restrict__ out,
                                    int32_t *__restrict__ status);
// K4 pass 2: the DEFER units, in ticket order (status[units] = ticket counter,
// status[units + 1] = pass 1's defer flag; both 0 before pass 1)
__global__ void k4_decompress_back(const uint8_t *__restrict__ comp, const uint64_t *__restrict__ offsets,
                                   uint64_t n, uint32_t unit, uint32_t hdr_mode, uint64_t header_value,
                                   uint32_t bias, uint8_t *__restrict__ out,
                                   int32_t *__restrict__ status);
// ---- record batches (snappy_records.hip): records of 0 .. SNAPPY_BLOCK bytes at
// (offset, length) pairs.  A matched record of L bytes owns records_need_words(L)
// u32 words of scratch at its scanned offset: L / 4 + 2 token words, as many
// escape words, then one (output offset, input position) pair per K2 segment.
__host__ __device__ constexpr uint32_t records_tok_cap(uint32_t L) { return L / 4 + 2; }
__host__ __device__ constexpr uint32_t records_segs(uint32_t L)
{
    return (records_tok_cap(L) + SNAPPY_K2_SEG - 1) / SNAPPY_K2_SEG;
}
__host__ __device__ constexpr uint32_t records_need_words(uint32_t L)
{
    return 2 * records_tok_cap(L) + 2 * records_segs(L);  // (even: the segment pairs stay 8-byte aligned)
}
// K1r / K1r64 over one class of a batch: workgroup b matches record list[b]
__global__ void kr1_match_records(const uint8_t *__restrict__ in, const uint64_t *__restrict__ off_len,
                                  const uint32_t *__restrict__ list, const uint64_t *__restrict__ sbase,
                                  uint32_t *__restrict__ scratch, uint32_t *__restrict__ ntok_out,
                                  uint32_t *__restrict__ sizes);
__global__ void kr1_match_records64(const uint8_t *__restrict__ in, const uint64_t *__restrict__ off_len,
                                    const uint32_t *__restrict__ list, const uint64_t *__restrict__ sbase,
                                    uint32_t *__restrict__ scratch, uint32_t *__restrict__ ntok_out,
                                    uint32_t *__restrict__ sizes);
// K2 over every record (grid x = records, y = waves per record); status = the plan's words
__global__ void kr2_emit_records(const uint8_t *__restrict__ in, const uint64_t *__restrict__ off_len,
                                 const int32_t *__restrict__ status, const uint64_t *__restrict__ sbase,
                                 const uint32_t *__restrict__ scratch, const uint32_t *__restrict__ ntok,
                                 const uint64_t *__restrict__ offsets, uint8_t *__restrict__ out);
// K4 pass 1, one wave per record; *first (~0 before) = min over failing records of record << 8 | -status
__global__ void kr4_decode_records(const uint8_t *__restrict__ comp, uint32_t bias, uint64_t comp_bytes,
                                   const uint64_t *__restrict__ comp_off_len, uint8_t *__restrict__ out,
                                   uint64_t out_bytes, const uint64_t *__restrict__ out_off_len,
                                   int32_t *__restrict__ status, unsigned long long *__restrict__ first);

// ---- long records (snappy_long_records.hip): records of 0 .. 2^30 bytes, each
// ceil(L / SNAPPY_BLOCK) blocks of one stream.  A unit is one block (or an empty
// record); the units of a batch are numbered in record order: record r owns
// units [ubase[r], ubase[r + 1]), urec[u] is unit u's record, and its table
// slice (nblk + 1 entries of the SINGLE index format) starts at tbase[r].
// K1r / K1r64 over one class's unit list: workgroup b matches unit list[b], whose
// scratch is at scratch + sbase[unit]; block 0 accounts for the record's preamble
__global__ void kr1_match_lunits(const uint8_t *__restrict__ in, const uint64_t *__restrict__ off_len,
                                 const uint32_t *__restrict__ list, const uint32_t *__restrict__ urec,
                                 const uint64_t *__restrict__ ubase, const uint64_t *__restrict__ sbase,
                                 uint32_t *__restrict__ scratch, uint32_t *__restrict__ ntok_out,
                                 uint32_t *__restrict__ sizes);
__global__ void kr1_match_lunits64(const uint8_t *__restrict__ in, const uint64_t *__restrict__ off_len,
                                   const uint32_t *__restrict__ list, const uint32_t *__restrict__ urec,
                                   const uint64_t *__restrict__ ubase, const uint64_t *__restrict__ sbase,
                                   uint32_t *__restrict__ scratch, uint32_t *__restrict__ ntok_out,
                                   uint32_t *__restrict__ sizes);
// K2 over every unit (grid x = units, y = waves per unit); offsets = K3 over the unit sizes
__global__ void kr2_emit_lunits(const uint8_t *__restrict__ in, const uint64_t *__restrict__ off_len,
                                const uint32_t *__restrict__ urec, const uint64_t *__restrict__ ubase,
                                const uint64_t *__restrict__ sbase, const uint32_t *__restrict__ scratch,
                                const uint32_t *__restrict__ ntok, const uint64_t *__restrict__ offsets,
                                uint8_t *__restrict__ out);
// The one-wave walk of k5_index_stream over every record of two or more blocks
// (grid x = records): record r's table slice from its own compressed range; the
// preamble must equal its decoded length.  rstatus[r] (the plan's word, 0 where
// the record passed the range checks) gets the walk's failure.  Records of at
// most one block get their entries (0, and the compressed length) without a walk.
__global__ void kr5_index_lrecords(const uint8_t *__restrict__ comp, const uint64_t *__restrict__ comp_off_len,
                                   const uint64_t *__restrict__ out_off_len, const uint64_t *__restrict__ tbase,
                                   uint64_t *__restrict__ index, int32_t *__restrict__ rstatus);
// What the two K4 entry points of long records read: every pointer is the batch's
struct K4LongArgs {
    const uint8_t *comp;            // 4-byte aligned; the records' offsets count from comp + bias
    uint32_t bias;
    const uint64_t *comp_off_len, *out_off_len;
    const uint32_t *urec;           // unit -> record
    const uint64_t *ubase, *tbase;  // record -> first unit, first table entry
    const uint64_t *index;          // the tables, packed
    const int32_t *rstatus;         // the records' status after the plan and the index (< 0: nothing is decoded)
    int32_t *ustatus;               // record r: max(nblk, 1) + 2 words at ubase[r] + 2 r (units, ticket, defer flag)
    uint32_t *defer;                // the batch's flag: some record has work for pass 2
    uint8_t *out;
};
// K4 pass 1 and pass 2 (grid x = units): k4_body with the SINGLE-layout arguments of the unit's record
__global__ void kr4_decode_lunits(const K4LongArgs a);
__global__ void kr4_back_lunits(const K4LongArgs a);

// ---- range decode (snappy_ranges.hip): the planned units of snappy_ranges.h
struct K4RangeArgs {
    uintptr_t comp_at;              // the address of the stream's byte 0: d_comp - comp_origin (any alignment)
    uint64_t win_end;               // comp_origin + comp_bytes: the end of the resident window, stream-relative
    const uint64_t *offsets;        // the stream's full index
    uint64_t n;
    uint32_t unit, hdr_mode, allow_back;
    uint32_t slot_cap;              // staging slots in use (edge k uses slot (k - 1) % slot_cap)
    const snappy_range_unit *plan;  // the planned units
    uint64_t first;                 // this launch's first planned unit
    unsigned long long *keys;       // per range: ~0, < 256 refused before any load (-status), else the
                                    // lowest failing unit: (unit + 1) << 8 | -status
    uint8_t *slots;
    uint8_t *out;
};
// K4 pass 1 over planned units [first, first + grid x), one wave each
__global__ void kr4_decode_range_units(const K4RangeArgs a);

// What the range decode of a framed stream shares with the calls it is built from
// (host functions, hidden: not part of the C ABI).  snappy_ranges.hip: the staging
// slots of a call (SNAPPY_RANGES_SLOT_CAP, or SNAPPY_AMD_RANGE_SLOTS), KG6 kr6_clip
// over planned units [first, first + units) and KG7 kr7_range_status over `count`
// keys.  snappy_frame.hip: KF1 over `count` (offset, length) entries from `base`.
__attribute__((visibility("hidden"))) uint32_t ranges_slot_cap();
__attribute__((visibility("hidden"))) void ranges_launch_clip(hipStream_t stream, const snappy_range_unit *plan,
                                                              uint64_t first, uint32_t units,
                                                              const unsigned long long *keys, const uint8_t *slots,
                                                              uint32_t slot_cap, uint8_t *out);
__attribute__((visibility("hidden"))) void ranges_launch_status(hipStream_t stream, const unsigned long long *keys,
                                                                uint64_t count, int32_t *status,
                                                                unsigned long long *first);
__attribute__((visibility("hidden"))) void frame_launch_crc32c(hipStream_t stream, const void *d_base,
                                                               const uint64_t *d_off_len, uint64_t count, int masked,
                                                               uint32_t *d_crc);
// snappy_long_records.hip, for the container range decode (snappy_container_ranges.hip):
// the launches of decompress_long_records_device on c->stream after its argument
// checks.  check_out = false: no record is refused for its output range (the offsets
// count from d_out, which may be null: then they are addresses).
__attribute__((visibility("hidden"))) int long_records_launch_decode(snappy_amd_ctx *c, const void *d_comp,
                                                                     size_t comp_bytes, const uint64_t *d_comp_off_len,
                                                                     size_t count, void *d_out, size_t out_bytes,
                                                                     const uint64_t *d_out_off_len,
                                                                     const uint64_t *d_index, int32_t *d_status,
                                                                     bool check_out, int sync);

// ---- range decode of a framed stream (snappy_frame_ranges.hip): the planned units
// of snappy_frame_ranges.h, each one data chunk of the stream
struct K4FrameArgs {
    uintptr_t comp_at;              // the address of the stream's byte 0: d_window - comp_origin (any alignment)
    const uint64_t *chunks;         // the chunk table and the seek table (or sub-tables: positions are absolute)
    const uint64_t *starts;
    uint32_t slot_cap;              // staging slots in use (edge k uses slot (k - 1) % slot_cap)
    const snappy_range_unit *plan;  // the planned units
    uint64_t first;                 // this launch's first planned unit
    unsigned long long *keys;       // per range: ~0, < 256 refused before any decode (-status), else the
                                    // lowest failing chunk: (chunk + 1) << 8 | -status
    int32_t *ustatus;               // per planned unit: its decode status (the CRC counts only where it is OK);
                                    // the header stage left 1 there for a unit that is not decoded and 2
                                    // for a stored chunk (the copy kernel's, which then writes 0)
    uint8_t *slots;
    uint8_t *out;
};
// K4 pass 1 over planned units [first, first + grid x), one wave per compressed chunk
__global__ void kr4_decode_frame_units(const K4FrameArgs a);

#ifndef SNAPPY_K5_CHUNK
#define SNAPPY_K5_CHUNK 16384
#endif
constexpr uint32_t K5_CHUNK = SNAPPY_K5_CHUNK;  // K5p chunk of compressed stream (K5_S in the kernels)
__global__ void k5a_chunk_walk(const uint8_t *__restrict__ comp, uint64_t clen, uint64_t *__restrict__ X,
                               uint64_t *__restrict__ O, uint32_t *__restrict__ P);
__global__ void k5b1_compose(const uint32_t *__restrict__ P, uint32_t nchunks, uint64_t *__restrict__ F);
__global__ void k5b_carry(const uint8_t *__restrict__ comp, uint64_t clen, uint32_t nchunks,
                          const uint64_t *__restrict__ X, const uint64_t *__restrict__ O, const uint64_t *__restrict__ F,
                          uint64_t *__restrict__ BE, uint64_t *__restrict__ BB, uint64_t *__restrict__ Ent,
                          uint64_t *__restrict__ Base, int64_t *__restrict__ result);
__global__ void k5b3_fill(const uint8_t *__restrict__ comp, uint64_t clen, const uint32_t *__restrict__ P,
                          uint32_t nchunks, const uint64_t *__restrict__ BE, const uint64_t *__restrict__ BB,
                          uint64_t *__restrict__ Ent, uint64_t *__restrict__ Base);
__global__ void k5c_mark(const uint8_t *__restrict__ comp, uint64_t clen, const uint64_t *__restrict__ Ent,
                         const uint64_t *__restrict__ Base, uint64_t *__restrict__ offsets, uint64_t max_units,
                         int32_t *__restrict__ cst, uint64_t *__restrict__ fin);
__global__ void k5d_result(uint32_t nchunks, const int32_t *__restrict__ cst, int64_t *__restrict__ result,
                           uint64_t *__restrict__ offsets, uint64_t max_units);
__global__ void k5_index_stream(const uint8_t *__restrict__ comp, uint64_t clen, uint64_t *__restrict__ offsets,
                                uint64_t max_units, int64_t *__restrict__ result);

}  // namespace snappy_amd

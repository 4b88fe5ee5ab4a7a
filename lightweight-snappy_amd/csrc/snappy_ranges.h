// snappy_ranges.h -- the plan rule of range decode: which blocks
// of a stream the byte ranges [start, start + length) touch, where each block's
// bytes land in the caller's buffer and which part of it is wanted.  One pure
// function, shared by the device call (snappy_ranges.hip) and the host forms
// (snappy_ranges_host.cpp) so both refuse and cut exactly alike; compiles as
// plain C.  Private: not part of the C ABI (snappy_amd_range is, in snappy_amd.h).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "snappy_amd.h"

// Edge blocks are decoded whole into staging slots of SNAPPY_AMD_BLOCK bytes in
// context scratch; a call holds at most SNAPPY_RANGES_SLOT_CAP of them (64 MiB)
// and runs more edge units in successive launches that reuse the slots.
#define SNAPPY_RANGES_SLOT_CAP 1024u

// One decode unit: one (range, block) pair.  32 bytes.
typedef struct {
    uint64_t unit;   // the stream's unit (block of SINGLE, chunk of STREAMS)
    uint64_t land;   // where the unit's byte 0 lands in the output, mod 2^64 (before the
                     // buffer for a range that starts inside the unit)
    uint32_t range;  // the owning range
    uint32_t lo, hi; // the wanted bytes [lo, hi) of the unit, 0 <= lo < hi <= its size
    uint32_t edge;   // 0: the unit lies wholly inside its range (it decodes straight to the
                     // output); k >= 1: the call's k-th edge unit (staged, then clipped)
} snappy_range_unit;

// The plan of `count` ranges over a stream of n decoded bytes in units of `unit`
// bytes (1 .. 65,536), into an output of out_bytes.  status[i] = 0, or the
// range's refusal, in this order: SNAPPY_AMD_ERR_ARG for a range that leaves
// [0, n), SNAPPY_AMD_ERR_CAPACITY for an output range that leaves [0, out_bytes).
// An accepted range of length > 0 owns the units start / unit .. (start + length
// - 1) / unit, in order; ranges in order.  units (may be NULL: count only) gets
// at most units_cap entries; *nunits and *nedges the numbers needed.  Returns 0,
// SNAPPY_AMD_ERR_ARG for unit == 0 or unit > 65,536, or SNAPPY_AMD_ERR_CAPACITY
// when units_cap was too small (the counts are still right).
static inline int snappy_ranges_plan(uint64_t n, uint32_t unit, const snappy_amd_range *ranges, size_t count,
                                     uint64_t out_bytes, int32_t *status, snappy_range_unit *units, size_t units_cap,
                                     uint64_t *nunits, uint64_t *nedges)
{
    uint64_t nu = 0, ne = 0;
    *nunits = 0;
    *nedges = 0;
    if (unit == 0 || unit > SNAPPY_AMD_BLOCK) return SNAPPY_AMD_ERR_ARG;
    for (size_t i = 0; i < count; i++) {
        const uint64_t start = ranges[i].start, len = ranges[i].length, oo = ranges[i].out_offset;
        int32_t st = SNAPPY_AMD_OK;
        if (start > n || len > n - start) st = SNAPPY_AMD_ERR_ARG;
        else if (oo > out_bytes || len > out_bytes - oo) st = SNAPPY_AMD_ERR_CAPACITY;
        status[i] = st;
        if (st != SNAPPY_AMD_OK || len == 0) continue;
        const uint64_t end = start + len, u0 = start / unit, u1 = (end - 1) / unit;
        for (uint64_t u = u0; u <= u1; u++) {
            const uint64_t b0 = u * unit;
            const uint32_t size = n - b0 < unit ? (uint32_t)(n - b0) : unit;
            const uint32_t lo = start > b0 ? (uint32_t)(start - b0) : 0u;
            const uint32_t hi = end - b0 < size ? (uint32_t)(end - b0) : size;
            const int is_edge = lo != 0 || hi != size;
            if (is_edge) ne++;
            if (units && nu < units_cap) {
                snappy_range_unit *e = &units[nu];
                e->unit = u;
                e->land = oo + b0 - start;
                e->range = (uint32_t)i;
                e->lo = lo;
                e->hi = hi;
                e->edge = is_edge ? (uint32_t)ne : 0u;
            }
            nu++;
        }
    }
    *nunits = nu;
    *nedges = ne;
    return units && nu > units_cap ? SNAPPY_AMD_ERR_CAPACITY : SNAPPY_AMD_OK;
}

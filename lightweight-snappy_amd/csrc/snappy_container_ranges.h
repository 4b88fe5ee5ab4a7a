// snappy_container_ranges.h -- the plan rule of range decode over a Hadoop or
// snappy-java container: which chunks the byte ranges [start,
// start + length) touch, found in the container's chunk tables, where each chunk's
// bytes land in the caller's buffer, which part of it is wanted, and what the
// table stage says about a chunk before it is decoded.  Pure functions, shared by
// the device kernels (snappy_container_ranges.hip) and the tests' stand-alone
// check, so both refuse and cut exactly alike; compiles as plain C.  Private: not
// part of the C ABI.
//
// The tables are those of container_index_device: nchunks (offset, length) u64
// pairs each, `comp` the payloads' places in the container, `outp` their places in
// the decoded bytes.  A sub-table keeps absolute offsets.  The decoded extent the
// tables cover is [outp[0], outp[2 (nchunks - 1)] + outp[2 (nchunks - 1) + 1]).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "snappy_amd.h"
#include "snappy_container.h"
#include "snappy_ranges.h"

// a unit the tables contradict themselves about (offsets that are not sorted or
// not contiguous inside a span, a chunk of more than 2^30 bytes, an empty first
// or last chunk): hi of its plan entry.  No chunk is that long, so the table stage
// refuses it (SNAPPY_AMD_ERR_INDEX, or SNAPPY_AMD_ERR_UNSUPPORTED for the length).
#define SNAPPY_CONTAINER_UNIT_BAD 0xFFFFFFFFu

// The last i in [0, nchunks) with outp[2 i] <= pos, by binary search: pair i is
// looked at only for 0 < i < nchunks.  nchunks >= 1 and outp[0] <= pos are the
// caller's; on a table that is not sorted the result is what the search gives,
// and still outp[2 i] <= pos.
SNAPPY_CONTAINER_FN uint64_t snappy_container_seek(const uint64_t *outp, uint64_t nchunks, uint64_t pos)
{
    uint64_t lo = 0, hi = nchunks - 1;
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo + 1) / 2;
        if (outp[2 * mid] <= pos) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// The span of one range: its refusal, else its first and last chunk.  Returns
// SNAPPY_AMD_ERR_ARG for a range that leaves the tables' extent (any range of
// length > 0 when nchunks == 0; the extent's end is taken mod 2^64), then
// SNAPPY_AMD_ERR_CAPACITY for an output range that leaves [0, out_bytes), then
// SNAPPY_AMD_ERR_INDEX for a span with u1 < u0 (a table that is not sorted).
// *count = the span's units: 0 for a refused or an empty range, else u1 - u0 + 1.
SNAPPY_CONTAINER_FN int32_t snappy_container_span(const uint64_t *outp, uint64_t nchunks, snappy_amd_range r,
                                                  uint64_t out_bytes, uint64_t *u0, uint64_t *u1, uint64_t *count)
{
    *u0 = *u1 = *count = 0;
    if (nchunks == 0) {
        if (r.length) return SNAPPY_AMD_ERR_ARG;
    } else {
        const uint64_t s0 = outp[0], s1 = outp[2 * (nchunks - 1)] + outp[2 * (nchunks - 1) + 1];
        if (r.start < s0 || r.start > s1 || r.length > s1 - r.start) return SNAPPY_AMD_ERR_ARG;
    }
    if (r.out_offset > out_bytes || r.length > out_bytes - r.out_offset) return SNAPPY_AMD_ERR_CAPACITY;
    if (r.length == 0) return SNAPPY_AMD_OK;
    *u0 = snappy_container_seek(outp, nchunks, r.start);
    *u1 = snappy_container_seek(outp, nchunks, r.start + r.length - 1);
    if (*u1 < *u0) return SNAPPY_AMD_ERR_INDEX;
    *count = *u1 - *u0 + 1;
    return SNAPPY_AMD_OK;
}

// Chunk u (u0 <= u <= u1) of an accepted range's span, as a plan unit without its
// edge word: e->unit, land, range, lo, hi.  Returns 1 for an edge unit (part of
// the chunk is wanted: it is staged and clipped), 0 otherwise.  The wanted bytes
// [outp[2 u] + lo, outp[2 u] + hi) lie inside the range whatever the table says:
//   hi == 0                          an empty chunk inside the span, the next one beginning
//                                    where it stands: skipped everywhere
//   hi == SNAPPY_CONTAINER_UNIT_BAD  the table contradicts itself here (see above)
//   else 0 <= lo < hi <= outp[2 u + 1] <= 2^30, and a chunk that is not the span's
//        last ends where the next one begins
SNAPPY_CONTAINER_FN int snappy_container_unit(const uint64_t *outp, snappy_amd_range r, uint32_t range, uint64_t u0,
                                              uint64_t u1, uint64_t u, snappy_range_unit *e)
{
    const uint64_t b0 = outp[2 * u], size = outp[2 * u + 1], end = r.start + r.length;
    const int first = u == u0, last = u == u1;
    e->unit = u;
    e->land = r.out_offset + b0 - r.start;
    e->range = range;
    e->lo = 0;
    e->hi = SNAPPY_CONTAINER_UNIT_BAD;
    e->edge = 0;
    if (size > SNAPPY_CONTAINER_CHUNK_MAX) return 0;
    if (size == 0) {
        if (!first && !last && outp[2 * (u + 1)] == b0) e->hi = 0;
        return 0;
    }
    // (the search gives outp[2 u0] <= start and outp[2 u1] <= end - 1)
    if (!first && b0 < r.start) return 0;
    if (!last && (b0 > end - 1 || end - b0 < size || outp[2 * (u + 1)] != b0 + size)) return 0;
    const uint64_t lo = first ? r.start - b0 : 0, hi = last ? end - b0 : size;
    if (lo >= hi || hi > size) return 0;
    e->lo = (uint32_t)lo;
    e->hi = (uint32_t)hi;
    return lo != 0 || hi != size;
}

// The table stage's verdict on a non-empty unit (hi != 0): the chunk's payload
// [co, co + cl) must lie inside the window [w0, w1) and be non-empty, the table's
// decoded length `size` must be at most 2^30, the unit must not be a contradiction
// (hi), and the payload's preamble -- w = its first min(cl, 5) bytes, read by the
// caller only after the first two checks passed -- must end there and say `size`.
// Returns SNAPPY_AMD_OK or the failure, in this order.
SNAPPY_CONTAINER_FN int32_t snappy_container_unit_check(const uint8_t *w, uint64_t co, uint64_t cl, uint64_t w0,
                                                        uint64_t w1, uint64_t size, uint32_t hi)
{
    if (co < w0 || co > w1 || cl > w1 - co) return SNAPPY_AMD_ERR_TRUNCATED;
    if (cl == 0) return SNAPPY_AMD_ERR_HEADER;
    if (size > SNAPPY_CONTAINER_CHUNK_MAX) return SNAPPY_AMD_ERR_UNSUPPORTED;
    if (hi == SNAPPY_CONTAINER_UNIT_BAD) return SNAPPY_AMD_ERR_INDEX;
    const uint32_t have = cl < 5u ? (uint32_t)cl : 5u;
    uint64_t L = 0;
    int ended = 0;
    for (uint32_t i = 0; i < have && !ended; i++) {
        L |= (uint64_t)(w[i] & 0x7Fu) << (7u * i);
        if (!(w[i] & 0x80u)) ended = 1;
    }
    if (!ended || L != size) return SNAPPY_AMD_ERR_HEADER;
    return SNAPPY_AMD_OK;
}

// Staging: an edge chunk takes its decoded length rounded up to 16 bytes
SNAPPY_CONTAINER_FN uint64_t snappy_container_stage_size(uint64_t size) { return (size + 15u) & ~(uint64_t)15u; }

// One step of the packing of edge chunks into launch groups, in plan order:
// the chunk of `need` staged bytes goes behind the group's `*fill` bytes unless
// that would pass `budget` and the group holds something; then it opens a new
// group (returns 1) at place 0.  *place = where it stands.  A chunk larger than
// the budget is therefore a group of its own.
SNAPPY_CONTAINER_FN int snappy_container_pack(uint64_t budget, uint64_t need, uint64_t *fill, uint64_t *place)
{
    int opened = 0;
    if (*fill && (need > budget || *fill > budget - need)) {
        *fill = 0;
        opened = 1;
    }
    *place = *fill;
    *fill += need;
    return opened;
}

// The plan of `count` ranges, as the device call makes it with a thread per range
// and per unit; this loop is the tests'.  status[i] = the span's result; an
// accepted range owns the units of its span in order, ranges in order; an edge
// unit's edge word is 2 * range + (1 for the span's first chunk, 2 for a last
// chunk that is not the first).  units (may be NULL: count only) gets at most
// units_cap entries; *nunits and *nedges the numbers needed.  Returns 0, or
// SNAPPY_AMD_ERR_CAPACITY when units_cap was too small (the counts are still right).
static inline int snappy_container_ranges_plan(const uint64_t *outp, uint64_t nchunks, const snappy_amd_range *ranges,
                                               size_t count, uint64_t out_bytes, int32_t *status,
                                               snappy_range_unit *units, size_t units_cap, uint64_t *nunits,
                                               uint64_t *nedges)
{
    uint64_t nu = 0, ne = 0;
    for (size_t i = 0; i < count; i++) {
        uint64_t u0, u1, k;
        status[i] = snappy_container_span(outp, nchunks, ranges[i], out_bytes, &u0, &u1, &k);
        for (uint64_t u = u0; k; u++, k--) {
            snappy_range_unit e;
            if (snappy_container_unit(outp, ranges[i], (uint32_t)i, u0, u1, u, &e)) {
                e.edge = 2u * (uint32_t)i + (u == u0 ? 1u : 2u);
                ne++;
            }
            if (units && nu < units_cap) units[nu] = e;
            nu++;
        }
    }
    *nunits = nu;
    *nedges = ne;
    return units && nu > units_cap ? SNAPPY_AMD_ERR_CAPACITY : SNAPPY_AMD_OK;
}

// snappy_frame_ranges.h -- the plan rule of range decode over a framed stream
// (DESIGN.md 7.7): which data chunks the byte ranges [start, start + length)
// touch, found in the stream's seek table, where each chunk's bytes land in the
// caller's buffer and which part of it is wanted.  Pure functions, shared by the
// device kernels (snappy_frame_ranges.hip) and the host forms
// (snappy_frame_host.cpp) so both refuse and cut exactly alike; compiles as plain
// C.  Private: not part of the C ABI.
//
// The seek table `starts` of a chunk table of nchunks data chunks has nchunks + 1
// entries: starts[i] = the decoded position of chunk i's first byte, starts[nchunks]
// = the position after the last chunk.  A sub-table keeps absolute positions.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "snappy_amd.h"
#include "snappy_frame.h"
#include "snappy_ranges.h"

// a unit the tables contradict themselves about (a seek table that is not sorted,
// a chunk of more than 65,536 bytes): hi of its plan entry.  No chunk is that long,
// so the header stage refuses it with SNAPPY_AMD_ERR_INDEX (hi > dlen).
#define SNAPPY_FRAME_UNIT_BAD 0xFFFFFFFFu

// The last i in [0, nchunks) with starts[i] <= pos, by binary search: entry i is
// looked at only for 0 < i < nchunks.  nchunks >= 1 and starts[0] <= pos are the
// caller's; on a table that is not sorted the result is what the search gives.
SNAPPY_FRAME_FN uint64_t snappy_frame_seek(const uint64_t *starts, uint64_t nchunks, uint64_t pos)
{
    uint64_t lo = 0, hi = nchunks - 1;
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo + 1) / 2;
        if (starts[mid] <= pos) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// The span of one range: its refusal, else its first and last chunk.  Returns
// SNAPPY_AMD_ERR_ARG for a range that leaves [starts[0], starts[nchunks]), then
// SNAPPY_AMD_ERR_CAPACITY for an output range that leaves [0, out_bytes), then
// SNAPPY_AMD_ERR_INDEX for a span with u1 < u0 (a table that is not sorted).
// *count = the span's units: 0 for a refused or an empty range, else u1 - u0 + 1.
SNAPPY_FRAME_FN int32_t snappy_frame_span(const uint64_t *starts, uint64_t nchunks, snappy_amd_range r,
                                          uint64_t out_bytes, uint64_t *u0, uint64_t *u1, uint64_t *count)
{
    *u0 = *u1 = *count = 0;
    const uint64_t s0 = starts[0], s1 = starts[nchunks];
    if (r.start < s0 || r.start > s1 || r.length > s1 - r.start) return SNAPPY_AMD_ERR_ARG;
    if (r.out_offset > out_bytes || r.length > out_bytes - r.out_offset) return SNAPPY_AMD_ERR_CAPACITY;
    if (r.length == 0) return SNAPPY_AMD_OK;
    // (length > 0 inside [s0, s1): s0 < s1, so nchunks >= 1)
    *u0 = snappy_frame_seek(starts, nchunks, r.start);
    *u1 = snappy_frame_seek(starts, nchunks, r.start + r.length - 1);
    if (*u1 < *u0) return SNAPPY_AMD_ERR_INDEX;
    *count = *u1 - *u0 + 1;
    return SNAPPY_AMD_OK;
}

// Chunk u (u0 <= u <= u1) of an accepted range's span, as a plan unit without its
// edge ordinal: e->unit, land, range, lo, hi.  Returns 1 for an edge unit (part of
// the chunk is wanted: it is staged and clipped), 0 otherwise.  The wanted bytes
// [starts[u] + lo, starts[u] + hi) lie inside the range whatever the table says:
//   hi == 0                      an empty chunk inside the span: skipped everywhere
//   hi == SNAPPY_FRAME_UNIT_BAD  the table contradicts itself here (see above)
//   else 0 <= lo < hi <= starts[u + 1] - starts[u] <= 65,536
SNAPPY_FRAME_FN int snappy_frame_unit(const uint64_t *starts, snappy_amd_range r, uint32_t range, uint64_t u0,
                                      uint64_t u1, uint64_t u, snappy_range_unit *e)
{
    const uint64_t b0 = starts[u], size = starts[u + 1] - b0, end = r.start + r.length;
    const int first = u == u0, last = u == u1;
    e->unit = u;
    e->land = r.out_offset + b0 - r.start;
    e->range = range;
    e->lo = 0;
    e->hi = SNAPPY_FRAME_UNIT_BAD;
    e->edge = 0;
    if (size > SNAPPY_FRAME_CHUNK_MAX) return 0;
    if (size == 0) {
        if (!first && !last) e->hi = 0;
        return 0;
    }
    // (the search gives starts[u0] <= start and starts[u1] <= end - 1)
    if (!first && b0 < r.start) return 0;
    if (!last && (b0 > end - 1 || end - b0 < size)) return 0;
    const uint64_t lo = first ? r.start - b0 : 0, hi = last ? end - b0 : size;
    if (lo >= hi || hi > size) return 0;
    e->lo = (uint32_t)lo;
    e->hi = (uint32_t)hi;
    return lo != 0 || hi != size;
}

// The plan of `count` ranges, as snappy_ranges_plan gives it for the bare stream:
// status[i] = the span's result; an accepted range owns the units of its span in
// order, ranges in order; edge units are numbered from 1 in plan order.  units
// (may be NULL: count only) gets at most units_cap entries; *nunits and *nedges the
// numbers needed.  Returns 0, or SNAPPY_AMD_ERR_CAPACITY when units_cap was too
// small (the counts are still right).  The device call makes the same plan with a
// thread per range and per unit; this loop is the host's and the tests'.
static inline int snappy_frame_ranges_plan(const uint64_t *starts, uint64_t nchunks, const snappy_amd_range *ranges,
                                           size_t count, uint64_t out_bytes, int32_t *status,
                                           snappy_range_unit *units, size_t units_cap, uint64_t *nunits,
                                           uint64_t *nedges)
{
    uint64_t nu = 0, ne = 0;
    for (size_t i = 0; i < count; i++) {
        uint64_t u0, u1, k;
        status[i] = snappy_frame_span(starts, nchunks, ranges[i], out_bytes, &u0, &u1, &k);
        for (uint64_t u = u0; k; u++, k--) {
            snappy_range_unit e;
            if (snappy_frame_unit(starts, ranges[i], (uint32_t)i, u0, u1, u, &e)) e.edge = (uint32_t)++ne;
            if (units && nu < units_cap) units[nu] = e;
            nu++;
        }
    }
    *nunits = nu;
    *nedges = ne;
    return units && nu > units_cap ? SNAPPY_AMD_ERR_CAPACITY : SNAPPY_AMD_OK;
}

// The header stage's verdict on a non-empty unit: the chunk at chunks[u], seen
// through w = its first 16 bytes (zero past the window's end), must be a data chunk
// that lies inside the window [w0, w1), ends at or before chunks[u + 1], decodes to
// starts[u + 1] - starts[u] bytes and holds the unit's hi.  Returns SNAPPY_AMD_OK
// or the failure, in this order; the caller reads w only for w0 <= pos < w1.
SNAPPY_FRAME_FN int32_t snappy_frame_unit_check(const uint8_t *w, uint64_t pos, uint64_t next, uint64_t w0,
                                                uint64_t w1, uint64_t size, uint32_t hi)
{
    if (pos < w0 || pos >= w1) return SNAPPY_AMD_ERR_TRUNCATED;
    uint32_t dlen;
    uint64_t adv;
    const int r = snappy_frame_chunk(w, w1 - pos, 0, &dlen, &adv);
    if (r < 0) return r;
    if (r == 0) return SNAPPY_AMD_ERR_INDEX;
    if (dlen != size) return SNAPPY_AMD_ERR_INDEX;
    if (next < pos || adv > next - pos) return SNAPPY_AMD_ERR_INDEX;
    if (hi > dlen) return SNAPPY_AMD_ERR_INDEX;
    return SNAPPY_AMD_OK;
}

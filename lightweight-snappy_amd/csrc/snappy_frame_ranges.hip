// snappy_frame_ranges.hip -- range decode of a framed stream: the decoded bytes
// [start, start + length) of many ranges through the stream's chunk table and its
// seek table, from a resident window of the stream, every touched chunk checked
// against its own header and its CRC (include/snappy_amd.h).
//
// Both tables are in HBM, so the plan (snappy_frame_ranges.h) runs there and one
// read-back of 64 bytes sizes the launches, as the long-record plan does:
//
//   KH0 kh0_plan (one thread per range: refusals, span, unit and edge counts) ->
//   K3 x 2 (the counts' scans) -> read-back ->
//   KH1 kh1_expand (one thread per unit: its snappy_range_unit) ->
//   KH2 kh2_headers (one thread per non-empty unit: the chunk inside the window, a
//       data chunk, agreeing with both tables) ->
//   KH3 kh3_entries (a range with a failing unit is refused here, before any decode;
//       every other unit gets its CRC entry and its decode status word) ->
//   per launch group of at most `slot_cap` edge units:
//     kr4_decode_frame_units (snappy_kernels.hip: k4_body's record form, one wave per
//         compressed chunk) + KH4 kh4_copy_stored (one wave per stored chunk);
//         interior units to the output, edge units to their staging slot ->
//     KF1 (snappy_frame.hip) over every unit of the group, whole, where it was decoded ->
//     KH5 kh5_verify (stored CRC against KF1's, where the decode succeeded) ->
//     KG6 kr6_clip (snappy_ranges.hip: slot[lo, hi) to the output) ->
//   KG7 kr7_range_status (keys -> d_status and the first failure)
//
// A range's key is that of snappy_ranges.hip: ~0 while nothing failed; below 256
// the refusal made before any decode (-status: the plan's, or its lowest failing
// unit's in the header stage); else (chunk + 1) << 8 | -status of its lowest
// chunk that failed to decode or to match its CRC (atomicMin).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <vector>

#include "snappy_amd.h"
#include "snappy_ctx.h"
#include "snappy_frame.h"
#include "snappy_frame_ranges.h"
#include "snappy_kernels.h"

using namespace snappy_amd;

namespace {

// what the host reads back once the plan is made (64 bytes, through c->h_total)
struct FramePlan {
    uint64_t units, edges;  // the scans' totals
    uint64_t sum;           // the unit counts added up in 64 bits (a scan's 32-bit partial sums
                            // hold whenever this is below 2^31)
    uint64_t first;         // KG7: min over failing ranges of range << 8 | -status (~0: none)
    uint64_t pad[4];
};
static_assert(sizeof(FramePlan) == 64, "read back through the context's 64 pinned bytes");

// the per-range tables of a call in c->r_meta
struct RangeTables {
    FramePlan *plan;
    unsigned long long *keys, *hkeys;  // hkeys: the header stage's lowest failing unit, (chunk + 1) << 8 | -status
    uint64_t *ubase, *ebase;           // count + 1: each range's first unit, and the edge units before it
    uint64_t *u0;                      // each range's first chunk
    snappy_amd_range *ranges;
    uint32_t *nunits, *nedges;
};
size_t range_bytes(size_t count) { return sizeof(FramePlan) + (count + 1) * 16 + count * (16 + 8 + 24 + 8); }
RangeTables range_tables(uint8_t *m, size_t count)
{
    RangeTables t;
    t.plan = reinterpret_cast<FramePlan *>(m);
    t.keys = reinterpret_cast<unsigned long long *>(m + sizeof(FramePlan));
    t.hkeys = t.keys + count;
    t.ubase = reinterpret_cast<uint64_t *>(t.hkeys + count);
    t.ebase = t.ubase + count + 1;
    t.u0 = t.ebase + count + 1;
    t.ranges = reinterpret_cast<snappy_amd_range *>(t.u0 + count);
    t.nunits = reinterpret_cast<uint32_t *>(t.ranges + count);
    t.nedges = t.nunits + count;
    return t;
}

// the per-unit tables of a call in c->f_meta
struct UnitTables {
    snappy_range_unit *plan;
    // KF1's entries, (offset, decoded bytes), in two tables: an interior unit's in off_len, from the
    // output's first byte; an edge unit's in slot_off_len, from the first staging slot; (0, 0) in the
    // other table and for a unit that is not decoded
    uint64_t *off_len, *slot_off_len;
    uint64_t *gstart;   // groups + 1: each launch group's first unit
    int32_t *ustatus;
    uint32_t *crc, *slot_crc;
};
size_t unit_bytes(size_t units, size_t groups) { return units * (32 + 32 + 4 + 8) + (groups + 1) * 8; }
UnitTables unit_tables(uint8_t *m, size_t units, size_t groups)
{
    UnitTables t;
    t.plan = reinterpret_cast<snappy_range_unit *>(m);
    t.off_len = reinterpret_cast<uint64_t *>(t.plan + units);
    t.slot_off_len = t.off_len + 2 * units;
    t.gstart = t.slot_off_len + 2 * units;
    t.ustatus = reinterpret_cast<int32_t *>(t.gstart + groups + 1);
    t.crc = reinterpret_cast<uint32_t *>(t.ustatus + units);
    t.slot_crc = t.crc + units;
    return t;
}

// KH0: one thread per range
__global__ __launch_bounds__(256) void kh0_plan(RangeTables t, uint64_t count, const uint64_t *__restrict__ starts,
                                                uint64_t nchunks, uint64_t out_bytes)
{
    const uint64_t r = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= count) return;
    const snappy_amd_range g = t.ranges[r];
    uint64_t u0, u1, k;
    const int32_t st = snappy_frame_span(starts, nchunks, g, out_bytes, &u0, &u1, &k);
    uint32_t edges = 0;
    if (k) {
        snappy_range_unit e;
        edges = (uint32_t)snappy_frame_unit(starts, g, (uint32_t)r, u0, u1, u0, &e);
        if (u1 != u0) edges += (uint32_t)snappy_frame_unit(starts, g, (uint32_t)r, u0, u1, u1, &e);
        atomicAdd(reinterpret_cast<unsigned long long *>(&t.plan->sum), (unsigned long long)k);
    }
    t.keys[r] = st == SNAPPY_AMD_OK ? ~0ull : (unsigned long long)-st;
    t.hkeys[r] = ~0ull;
    t.u0[r] = u0;
    t.nunits[r] = (uint32_t)k;  // (k <= nchunks < 2^31)
    t.nedges[r] = edges;
}

// KH1: one thread per unit p: its range is the last r with ubase[r] <= p (a range
// without units shares its entry with the next one)
__global__ __launch_bounds__(256) void kh1_expand(RangeTables t, uint64_t count, uint64_t units,
                                                  const uint64_t *__restrict__ starts, uint32_t slot_cap,
                                                  snappy_range_unit *__restrict__ plan, uint64_t *__restrict__ gstart)
{
    const uint64_t p = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= units) return;
    uint64_t lo = 0, hi = count - 1;
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo + 1) / 2;
        if (t.ubase[mid] <= p) lo = mid;
        else hi = mid - 1;
    }
    const uint32_t r = (uint32_t)lo;
    const snappy_amd_range g = t.ranges[r];
    const uint64_t u0 = t.u0[r], u1 = u0 + t.nunits[r] - 1, u = u0 + (p - t.ubase[r]);
    snappy_range_unit e, e0;
    if (snappy_frame_unit(starts, g, r, u0, u1, u, &e)) {
        // the range's first edge unit, or its second: after its first chunk, where that is one
        const uint64_t k = t.ebase[r] + 1 + (u != u0 && snappy_frame_unit(starts, g, r, u0, u1, u0, &e0) ? 1u : 0u);
        e.edge = (uint32_t)k;
        // a launch group starts at every slot_cap-th edge unit (its slot is free again by then)
        if (k > 1 && (k - 1) % slot_cap == 0) gstart[(k - 1) / slot_cap] = p;
    }
    plan[p] = e;
}

// KH2: one thread per unit.  Reads the tables and at most 16 window bytes, none
// of them outside [w0, w1).
__global__ __launch_bounds__(256) void kh2_headers(RangeTables t, const snappy_range_unit *__restrict__ plan,
                                                   uint64_t units, const uint64_t *__restrict__ chunks,
                                                   const uint64_t *__restrict__ starts, uintptr_t comp_at, uint64_t w0,
                                                   uint64_t w1)
{
    const uint64_t p = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= units) return;
    const snappy_range_unit e = plan[p];
    if (e.hi == 0 || t.keys[e.range] < 256) return;
    const uint64_t pos = chunks[e.unit], next = chunks[e.unit + 1];
    uint8_t w[SNAPPY_FRAME_WINDOW] = {};
    if (pos >= w0 && pos < w1) {
        const uint8_t *f = reinterpret_cast<const uint8_t *>(comp_at + pos);
        const uint64_t avail = w1 - pos;
#pragma unroll
        for (uint32_t k = 0; k < SNAPPY_FRAME_WINDOW; k++) w[k] = k < avail ? f[k] : (uint8_t)0;
    }
    const int32_t st = snappy_frame_unit_check(w, pos, next, w0, w1, starts[e.unit + 1] - starts[e.unit], e.hi);
    if (st != SNAPPY_AMD_OK) atomicMin(t.hkeys + e.range, ((unsigned long long)(e.unit + 1) << 8) | (uint32_t)-st);
}

// KH3: one thread per unit.  A range the header stage failed becomes a refused
// one (every one of its units writes the same key); a unit that will be decoded
// gets KF1's entry over its whole decoded bytes where they will stand and ustatus
// 0 (a compressed chunk: the decode kernel's) or 2 (a stored chunk: the copy
// kernel's), every other one ustatus 1 and empty entries.  The two kernels of a
// launch group then pick their units by this word alone.
__global__ __launch_bounds__(256) void kh3_entries(RangeTables t, const snappy_range_unit *__restrict__ plan,
                                                   uint64_t units, const uint64_t *__restrict__ chunks,
                                                   const uint64_t *__restrict__ starts, uintptr_t comp_at,
                                                   uint32_t slot_cap, uint64_t *__restrict__ off_len,
                                                   uint64_t *__restrict__ slot_off_len, int32_t *__restrict__ ustatus)
{
    const uint64_t p = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= units) return;
    const snappy_range_unit e = plan[p];
    const unsigned long long hk = t.hkeys[e.range];
    bool live = e.hi != 0;
    if (hk != ~0ull) {
        t.keys[e.range] = hk & 0xFF;
        live = false;
    } else if (t.keys[e.range] < 256) {
        live = false;
    }
    const uint64_t len = live ? starts[e.unit + 1] - starts[e.unit] : 0;
    const bool staged = live && e.edge;
    off_len[2 * p] = live && !staged ? e.land : 0;
    off_len[2 * p + 1] = staged ? 0 : len;
    slot_off_len[2 * p] = staged ? (uint64_t)((e.edge - 1) % slot_cap) * SNAPPY_BLOCK : 0;
    slot_off_len[2 * p + 1] = staged ? len : 0;
    // (a live unit's chunk passed the header stage: its type byte is inside the window)
    ustatus[p] = !live ? 1 : *reinterpret_cast<const uint8_t *>(comp_at + chunks[e.unit]) == 0x01u ? 2 : 0;
}

constexpr uint32_t kH4Waves = 4;

// KH4: one wave per unit of the group; a stored chunk's payload is its decoded
// bytes: copied to where the decode kernel would have put them (the place and the
// length are KF1's entry), and the unit's status word becomes 0
__global__ __launch_bounds__(64 * kH4Waves) void kh4_copy_stored(const snappy_range_unit *__restrict__ plan,
                                                                 uint64_t first, uint64_t units,
                                                                 const uint64_t *__restrict__ chunks,
                                                                 uintptr_t comp_at, const uint64_t *__restrict__ off_len,
                                                                 const uint64_t *__restrict__ slot_off_len,
                                                                 uint8_t *__restrict__ out, uint8_t *__restrict__ slots,
                                                                 int32_t *__restrict__ ustatus)
{
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t j = (uint64_t)blockIdx.x * kH4Waves + (threadIdx.x >> 6);
    if (j >= units) return;
    const uint64_t p = first + j;
    if (ustatus[p] != 2) return;
    const uint8_t *h = reinterpret_cast<const uint8_t *>(comp_at + chunks[plan[p].unit]);
    const bool staged = plan[p].edge != 0;
    const uint64_t *ol = (staged ? slot_off_len : off_len) + 2 * p;
    snappy_frame_wave_copy((staged ? slots : out) + ol[0], h + 8, (uint32_t)ol[1], lane);
    if (lane == 0) ustatus[p] = 0;
}

// KH5: one thread per unit of the group: the chunk's stored CRC against KF1's over
// its decoded bytes.  A CRC counts only where the unit's decode succeeded.
__global__ __launch_bounds__(256) void kh5_verify(const snappy_range_unit *__restrict__ plan, uint64_t first,
                                                  uint64_t units, const uint64_t *__restrict__ chunks,
                                                  uintptr_t comp_at, const int32_t *__restrict__ ustatus,
                                                  const uint32_t *__restrict__ crc,
                                                  const uint32_t *__restrict__ slot_crc,
                                                  unsigned long long *__restrict__ keys)
{
    const uint64_t j = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= units) return;
    const uint64_t p = first + j;
    if (ustatus[p] != 0) return;
    const snappy_range_unit e = plan[p];
    const uint8_t *h = reinterpret_cast<const uint8_t *>(comp_at + chunks[e.unit] + 4);
    const uint32_t stored = (uint32_t)h[0] | ((uint32_t)h[1] << 8) | ((uint32_t)h[2] << 16) | ((uint32_t)h[3] << 24);
    if (stored != (e.edge ? slot_crc : crc)[p])
        atomicMin(keys + e.range, ((unsigned long long)(e.unit + 1) << 8) | (uint32_t)-SNAPPY_AMD_ERR_CHECKSUM);
}

uint32_t blocks_of(uint64_t items, uint32_t per) { return (uint32_t)((items + per - 1) / per); }

void scan(snappy_amd_ctx *c, const uint32_t *v, uint64_t count, uint64_t *offsets, uint64_t *total)
{
    if (count <= SNAPPY_K3_WAVE_MAX)
        hipLaunchKernelGGL(k3_scan_wave, dim3(1), dim3(64), 0, c->stream, v, count, offsets, total);
    else
        hipLaunchKernelGGL(k3_scan, dim3(1), dim3(1024), 0, c->stream, v, count, offsets, total);
}

}  // namespace

extern "C" int snappy_amd_decompress_frame_ranges_device(snappy_amd_ctx *c, const void *d_window, uint64_t comp_origin,
                                                         size_t comp_bytes, const uint64_t *d_chunks,
                                                         const uint64_t *d_starts, size_t nchunks,
                                                         const snappy_amd_range *ranges, size_t count, void *d_out,
                                                         size_t out_bytes, int32_t *d_status)
{
    if (!c || (count && !ranges) || (!d_window && comp_bytes) || (!d_out && out_bytes)) return SNAPPY_AMD_ERR_ARG;
    // (the record body numbers chunks in 32 bits, from 1; a range's key holds its index in 56)
    if (count > 0x7FFFFFFFull || nchunks > 0x7FFFFFFEull) return SNAPPY_AMD_ERR_ARG;
    if (comp_origin + (uint64_t)comp_bytes < comp_origin) return SNAPPY_AMD_ERR_ARG;
    if (count == 0) return SNAPPY_AMD_OK;
    if (!d_starts || !d_chunks) return SNAPPY_AMD_ERR_ARG;
    HIP_OK(hipSetDevice(c->device));
    if (ctx_stream(c)) return SNAPPY_AMD_ERR_DEVICE;
    (void)hipGetLastError();  // (a pending error that is not this call's, as in compress_launch)

    // ---- the plan: statuses, spans, unit and edge counts per range, their scans; one read-back
    int rc;
    if ((rc = grow(reinterpret_cast<void **>(&c->r_meta), &c->r_meta_cap, range_bytes(count)))) return rc;
    const RangeTables t = range_tables(c->r_meta, count);
    HIP_OK(hipMemsetAsync(t.plan, 0, sizeof(FramePlan), c->stream));
    HIP_OK(hipMemsetAsync(&t.plan->first, 0xFF, sizeof(uint64_t), c->stream));
    HIP_OK(hipMemcpyAsync(t.ranges, ranges, count * sizeof(snappy_amd_range), hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(kh0_plan, dim3(blocks_of(count, 256)), dim3(256), 0, c->stream, t, (uint64_t)count, d_starts,
                       (uint64_t)nchunks, (uint64_t)out_bytes);
    scan(c, t.nunits, count, t.ubase, &t.plan->units);
    scan(c, t.nedges, count, t.ebase, &t.plan->edges);
    HIP_OK(hipGetLastError());
    FramePlan *const hp = reinterpret_cast<FramePlan *>(c->h_total);
    HIP_OK(hipMemcpyAsync(hp, t.plan, sizeof(FramePlan), hipMemcpyDeviceToHost, c->stream));
    HIP_OK(hipStreamSynchronize(c->stream));
    if (hp->sum > 0x7FFFFFFFull) return SNAPPY_AMD_ERR_ARG;
    const size_t units = (size_t)hp->sum, edges = (size_t)hp->edges;

    if (units) {
        const uint32_t cap = ranges_slot_cap();
        const size_t groups = edges > cap ? (edges + cap - 1) / cap : 1;
        const size_t slots_used = edges < cap ? edges : cap;
        if ((rc = grow(reinterpret_cast<void **>(&c->f_meta), &c->f_meta_cap, unit_bytes(units, groups)))) return rc;
        // (+ 16: the clip's funnel shift reads the aligned dword after a slot's last byte)
        if (slots_used &&
            (rc = grow(reinterpret_cast<void **>(&c->f_scr), &c->f_scr_cap, slots_used * SNAPPY_BLOCK + 16)))
            return rc;
        const UnitTables ut = unit_tables(c->f_meta, units, groups);
        const uintptr_t comp_at = reinterpret_cast<uintptr_t>(d_window) - comp_origin;
        const uint64_t w0 = comp_origin, w1 = comp_origin + (uint64_t)comp_bytes;
        const uint32_t ublocks = blocks_of(units, 256);
        hipLaunchKernelGGL(kh1_expand, dim3(ublocks), dim3(256), 0, c->stream, t, (uint64_t)count, (uint64_t)units,
                           d_starts, cap, ut.plan, ut.gstart);
        hipLaunchKernelGGL(kh2_headers, dim3(ublocks), dim3(256), 0, c->stream, t, ut.plan, (uint64_t)units, d_chunks,
                           d_starts, comp_at, w0, w1);
        hipLaunchKernelGGL(kh3_entries, dim3(ublocks), dim3(256), 0, c->stream, t, ut.plan, (uint64_t)units, d_chunks,
                           d_starts, comp_at, cap, ut.off_len, ut.slot_off_len, ut.ustatus);
        HIP_OK(hipGetLastError());
        // launch groups: consecutive units holding at most `cap` edge units, whose slots
        // (edge ordinal mod cap) are therefore distinct; the next group reuses them after
        // this group's clip, in stream order.  More than one group: their first units are
        // read back (the only call that reads twice is one with more edge units than slots).
        std::vector<uint64_t> gs(groups + 1, 0);
        gs[groups] = units;
        if (groups > 1) {
            HIP_OK(hipMemcpyAsync(gs.data() + 1, ut.gstart + 1, (groups - 1) * sizeof(uint64_t), hipMemcpyDeviceToHost,
                                  c->stream));
            HIP_OK(hipStreamSynchronize(c->stream));
        }
        K4FrameArgs a;
        a.comp_at = comp_at;
        a.chunks = d_chunks;
        a.starts = d_starts;
        a.slot_cap = cap;
        a.plan = ut.plan;
        a.keys = t.keys;
        a.ustatus = ut.ustatus;
        a.slots = c->f_scr;
        a.out = static_cast<uint8_t *>(d_out);
        for (size_t g = 0; g < groups; g++) {
            const uint64_t p0 = gs[g], n = gs[g + 1] - gs[g];
            if (gs[g + 1] < p0 || gs[g + 1] > units) return SNAPPY_AMD_ERR_DEVICE;  // (cannot happen: kh1_expand's)
            if (n == 0) continue;
            a.first = p0;
            hipLaunchKernelGGL(kr4_decode_frame_units, dim3((uint32_t)n), dim3(64), 0, c->stream, a);
            hipLaunchKernelGGL(kh4_copy_stored, dim3(blocks_of(n, kH4Waves)), dim3(64 * kH4Waves), 0, c->stream, ut.plan,
                               p0, n, d_chunks, comp_at, ut.off_len, ut.slot_off_len, a.out, a.slots, ut.ustatus);
            // KF1 over the units that stand in the output, and (a call with edge units) over the staged ones
            frame_launch_crc32c(c->stream, d_out, ut.off_len + 2 * p0, n, 1, ut.crc + p0);
            if (edges) frame_launch_crc32c(c->stream, c->f_scr, ut.slot_off_len + 2 * p0, n, 1, ut.slot_crc + p0);
            hipLaunchKernelGGL(kh5_verify, dim3(blocks_of(n, 256)), dim3(256), 0, c->stream, ut.plan, p0, n, d_chunks,
                               comp_at, ut.ustatus, ut.crc, ut.slot_crc, t.keys);
            if (edges)
                ranges_launch_clip(c->stream, ut.plan, p0, (uint32_t)n, t.keys, c->f_scr, cap,
                                   static_cast<uint8_t *>(d_out));
            HIP_OK(hipGetLastError());
        }
    }
    unsigned long long *first = reinterpret_cast<unsigned long long *>(&t.plan->first);
    ranges_launch_status(c->stream, t.keys, (uint64_t)count, d_status, first);
    HIP_OK(hipGetLastError());
    HIP_OK(hipMemcpyAsync(c->h_total, first, sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
    HIP_OK(hipStreamSynchronize(c->stream));
    return *c->h_total == ~0ull ? SNAPPY_AMD_OK : -(int)(*c->h_total & 0xFF);
}

// snappy_ranges.hip -- range decode: the stream's decoded bytes [start, start +
// length) of many ranges through its block index, from a resident window of the
// compressed stream (include/snappy_amd.h).
//
// The host plans (snappy_ranges.h): one unit per (range, block) pair, with where
// the block's byte 0 lands and the clip [lo, hi) inside it.  The plan and the
// ranges' keys are written to pinned memory and uploaded in one copy, so the call
// reads nothing back to size its launches:
//
//   KG0 kr0_range_check (one thread per unit: its compressed bytes lie inside the
//       window, else the range is refused before any load) ->
//   per launch group of at most `slot_cap` edge units:
//     KG4 kr4_decode_range_units (snappy_kernels.hip: k4_body, one wave per unit;
//         interior units to the output, edge units to their staging slot) ->
//     KG6 kr6_clip (slot[lo, hi) to the output) ->
//   KG7 kr7_range_status (keys -> d_status and the first failure)
//
// A range's key: ~0 while nothing failed; below 256 the refusal made before any
// load (-status: the plan's ERR_ARG / ERR_CAPACITY, the check's ERR_TRUNCATED);
// else (unit + 1) << 8 | -status of its lowest failing unit (atomicMin).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "snappy_amd.h"
#include "snappy_ctx.h"
#include "snappy_kernels.h"
#include "snappy_ranges.h"

using namespace snappy_amd;

namespace {

constexpr uint64_t kOffMask = (1ull << SNAPPY_AMD_IDX_OFFSET_BITS) - 1;
constexpr size_t kHead = 64;  // the upload's head: the first failure (u64), padding
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// KG0: one thread per planned unit.  The unit's compressed bytes [entry[u],
// entry[u + 1]) must lie inside the window [w0, w1); where entry u + 1 carries
// skip bits the unit's last element straddles out and is decoded to its end: its
// tag and length bytes (read only once they are known to be resident), then its
// whole size, must be inside too.  Reads the index and at most 5 window bytes.
__global__ __launch_bounds__(256) void kr0_range_check(const snappy_range_unit *__restrict__ plan, uint64_t units,
                                                       const uint64_t *__restrict__ offsets,
                                                       const uint8_t *__restrict__ comp, uint64_t w0, uint64_t w1,
                                                       unsigned long long *__restrict__ keys)
{
    const uint64_t p = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= units) return;
    const uint32_t r = plan[p].range;
    if (keys[r] < 256) return;
    const uint64_t u = plan[p].unit;
    const uint64_t e0 = offsets[u], e1 = offsets[u + 1];
    const uint64_t o0 = e0 & kOffMask, o1 = e1 & kOffMask;
    bool bad = o0 < w0 || o0 > w1 || o1 < w0 || o1 > w1;
    if (!bad && (e1 >> SNAPPY_AMD_IDX_OFFSET_BITS)) {
        // the element at o1: tag, then (a literal) up to 4 length bytes
        bad = o1 >= w1;
        if (!bad) {
            const uint8_t *q = comp + (o1 - w0);
            const uint64_t left = w1 - o1;
            const uint32_t tag = q[0], t = tag & 3, m = tag >> 2;
            uint64_t size;
            if (t == 0) {
                const uint32_t k = m >= 60 ? m - 59 : 0;
                uint64_t len = m;
                if (k) {
                    bad = 1 + k > left;
                    len = 0;
                    for (uint32_t i = 0; i < k && !bad; i++) len |= (uint64_t)q[1 + i] << (8 * i);
                }
                size = 1 + k + len + 1;
            } else {
                size = t == 1 ? 2 : t == 2 ? 3 : 5;
            }
            if (!bad) bad = size > left;
        }
    }
    if (bad) atomicMin(keys + r, (unsigned long long)-SNAPPY_ST_TRUNCATED);
}

// KG6: workgroup b (256 threads) copies the wanted bytes [lo, hi) of planned unit
// first + b's staging slot to the output at land + [lo, hi); interior units and
// the units of a range that has failed leave at once.  The destination is cut at
// its 16-byte boundaries: bytes up to the first, then 16-byte stores when the
// source is 16-aligned there too, else dword stores each funnel-shifted out of
// two aligned source dwords, then the bytes after the last.
__global__ __launch_bounds__(256) void kr6_clip(const snappy_range_unit *__restrict__ plan, uint64_t first,
                                                const unsigned long long *__restrict__ keys,
                                                const uint8_t *__restrict__ slots, uint32_t slot_cap,
                                                uint8_t *__restrict__ out)
{
    const snappy_range_unit e = plan[first + blockIdx.x];
    if (e.edge == 0 || keys[e.range] != ~0ull) return;
    const uint8_t *const src = slots + (uint64_t)((e.edge - 1) % slot_cap) * SNAPPY_BLOCK + e.lo;
    uint8_t *const dst = reinterpret_cast<uint8_t *>(reinterpret_cast<uintptr_t>(out) + e.land + e.lo);
    const uint32_t len = e.hi - e.lo, t = threadIdx.x;
    const uint32_t h0 = (uint32_t)(-reinterpret_cast<uintptr_t>(dst) & 15);
    const uint32_t h = h0 < len ? h0 : len;
    if (t < h) dst[t] = src[t];
    const uint32_t body = (len - h) & ~15u;
    const uint8_t *const s = src + h;
    uint8_t *const d = dst + h;
    const uint32_t sa = (uint32_t)(reinterpret_cast<uintptr_t>(s) & 3);
    if ((reinterpret_cast<uintptr_t>(s) & 15) == 0) {
        for (uint32_t x = 16 * t; x < body; x += 16 * 256)
            *reinterpret_cast<u32x4 *>(d + x) = *reinterpret_cast<const u32x4 *>(s + x);
    } else {
        // (the dword after the last one holding a wanted byte is read only for sa != 0,
        // and then holds the body's last bytes: it lies inside the slot or its 16-byte pad)
        const uint32_t *const s4 = reinterpret_cast<const uint32_t *>(s - sa);
        uint32_t *const d4 = reinterpret_cast<uint32_t *>(d);
        for (uint32_t j = t; j < body / 4; j += 256) {
            const uint32_t lo = s4[j];
            d4[j] = sa ? __builtin_amdgcn_alignbit(s4[j + 1], lo, 8 * sa) : lo;
        }
    }
    const uint32_t done = h + body;
    if (done + t < len) dst[done + t] = src[done + t];
}

// KG7: one thread per range: its key as a status word, and the call's first failure
__global__ __launch_bounds__(256) void kr7_range_status(const unsigned long long *__restrict__ keys, uint64_t count,
                                                        int32_t *__restrict__ status,
                                                        unsigned long long *__restrict__ first)
{
    const uint64_t r = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= count) return;
    const unsigned long long k = keys[r];
    const int32_t st = k == ~0ull ? SNAPPY_ST_OK : -(int32_t)(k & 0xFF);
    if (status) status[r] = st;
    if (st != SNAPPY_ST_OK) atomicMin(first, ((unsigned long long)r << 8) | (uint32_t)-st);
}

uint32_t blocks_of(uint64_t items, uint32_t per) { return (uint32_t)((items + per - 1) / per); }

}  // namespace

// ---- shared with the framed form (snappy_frame_ranges.hip; declared in snappy_kernels.h)
namespace snappy_amd {

// the staging slots of a call: SNAPPY_RANGES_SLOT_CAP, or fewer through the
// test-only SNAPPY_AMD_RANGE_SLOTS (the reuse path without 64 MiB of edge units)
uint32_t ranges_slot_cap()
{
    const char *e = getenv("SNAPPY_AMD_RANGE_SLOTS");
    if (e && *e) {
        const long v = strtol(e, nullptr, 10);
        if (v >= 1 && v <= (long)SNAPPY_RANGES_SLOT_CAP) return (uint32_t)v;
    }
    return SNAPPY_RANGES_SLOT_CAP;
}

void ranges_launch_clip(hipStream_t stream, const snappy_range_unit *plan, uint64_t first, uint32_t units,
                        const unsigned long long *keys, const uint8_t *slots, uint32_t slot_cap, uint8_t *out)
{
    hipLaunchKernelGGL(kr6_clip, dim3(units), dim3(256), 0, stream, plan, first, keys, slots, slot_cap, out);
}

void ranges_launch_status(hipStream_t stream, const unsigned long long *keys, uint64_t count, int32_t *status,
                          unsigned long long *first)
{
    hipLaunchKernelGGL(kr7_range_status, dim3(blocks_of(count, 256)), dim3(256), 0, stream, keys, count, status, first);
}

}  // namespace snappy_amd

extern "C" int snappy_amd_decompress_ranges_device(snappy_amd_ctx *c, const void *d_comp, uint64_t comp_origin,
                                                   size_t comp_bytes, const uint64_t *d_offsets, size_t n,
                                                   uint32_t chunk, int layout, const snappy_amd_range *ranges,
                                                   size_t count, void *d_out, size_t out_bytes, int32_t *d_status,
                                                   int sync)
{
    if (!c || (count && !ranges) || (!d_comp && comp_bytes) || (!d_out && out_bytes)) return SNAPPY_AMD_ERR_ARG;
    if (layout != SNAPPY_AMD_SINGLE && layout != SNAPPY_AMD_STREAMS) return SNAPPY_AMD_ERR_ARG;
    const uint32_t unit = layout == SNAPPY_AMD_SINGLE ? SNAPPY_BLOCK : chunk;
    if (unit == 0 || unit > SNAPPY_BLOCK) return SNAPPY_AMD_ERR_ARG;
    // (k4_body numbers units in 32 bits; a range's key holds its index in 56)
    if (count > 0x7FFFFFFFull || ((uint64_t)n + unit - 1) / unit > 0x7FFFFFFFull) return SNAPPY_AMD_ERR_ARG;
    if (comp_origin > kOffMask || comp_bytes > kOffMask) return SNAPPY_AMD_ERR_ARG;
    if (count == 0) return SNAPPY_AMD_OK;
    HIP_OK(hipSetDevice(c->device));
    if (ctx_stream(c)) return SNAPPY_AMD_ERR_DEVICE;
    (void)hipGetLastError();  // (a pending error that is not this call's, as in compress_launch)

    // ---- the plan, in pinned memory: head | keys | units.  The last call's upload
    // may still read the buffer: wait for it (its event), not for the stream.
    if (c->plan_ev) HIP_OK(hipEventSynchronize(c->plan_ev));
    else HIP_OK(hipEventCreateWithFlags(&c->plan_ev, hipEventDisableTiming));
    int32_t *hst = static_cast<int32_t *>(malloc(count * sizeof(int32_t)));
    if (!hst) return SNAPPY_AMD_ERR_DEVICE;
    uint64_t nunits = 0, nedges = 0;
    int rc = snappy_ranges_plan(n, unit, ranges, count, out_bytes, hst, nullptr, 0, &nunits, &nedges);
    if (rc == SNAPPY_AMD_OK && (nunits > 0x7FFFFFFFull || (nunits && !d_offsets))) rc = SNAPPY_AMD_ERR_ARG;
    const size_t keys_at = kHead, units_at = kHead + count * sizeof(uint64_t);
    const size_t bytes = units_at + (size_t)nunits * sizeof(snappy_range_unit);
    if (rc == SNAPPY_AMD_OK && bytes > c->h_plan_cap) {
        if (c->h_plan) (void)hipHostFree(c->h_plan);
        c->h_plan = nullptr;
        c->h_plan_cap = 0;
        const size_t want = bytes + bytes / 8 + 4096;
        if (hipHostMalloc(reinterpret_cast<void **>(&c->h_plan), want, hipHostMallocDefault) != hipSuccess) {
            c->h_plan = nullptr;
            rc = SNAPPY_AMD_ERR_DEVICE;
        } else {
            c->h_plan_cap = want;
        }
    }
    if (rc != SNAPPY_AMD_OK) {
        free(hst);
        return rc;
    }
    memset(c->h_plan, 0xFF, kHead);
    uint64_t *hkeys = reinterpret_cast<uint64_t *>(c->h_plan + keys_at);
    snappy_range_unit *hunits = reinterpret_cast<snappy_range_unit *>(c->h_plan + units_at);
    (void)snappy_ranges_plan(n, unit, ranges, count, out_bytes, hst, hunits, (size_t)nunits, &nunits, &nedges);
    for (size_t i = 0; i < count; i++) hkeys[i] = hst[i] == SNAPPY_AMD_OK ? ~0ull : (uint64_t)-hst[i];
    free(hst);

    const uint32_t cap = ranges_slot_cap();
    const uint32_t slots_used = (uint32_t)(nedges < cap ? nedges : cap);
    if ((rc = grow(reinterpret_cast<void **>(&c->r_meta), &c->r_meta_cap, bytes))) return rc;
    // (+ 16: the clip's funnel shift reads the aligned dword after a slot's last byte)
    if (slots_used &&
        (rc = grow(reinterpret_cast<void **>(&c->f_scr), &c->f_scr_cap, (size_t)slots_used * SNAPPY_BLOCK + 16)))
        return rc;
    HIP_OK(hipMemcpyAsync(c->r_meta, c->h_plan, bytes, hipMemcpyHostToDevice, c->stream));
    HIP_OK(hipEventRecord(c->plan_ev, c->stream));
    unsigned long long *first = reinterpret_cast<unsigned long long *>(c->r_meta);
    unsigned long long *keys = reinterpret_cast<unsigned long long *>(c->r_meta + keys_at);
    const snappy_range_unit *plan = reinterpret_cast<const snappy_range_unit *>(c->r_meta + units_at);

    if (nunits) {
        hipLaunchKernelGGL(kr0_range_check, dim3(blocks_of(nunits, 256)), dim3(256), 0, c->stream, plan, nunits,
                           d_offsets, static_cast<const uint8_t *>(d_comp), comp_origin,
                           comp_origin + (uint64_t)comp_bytes, keys);
        K4RangeArgs a;
        a.comp_at = reinterpret_cast<uintptr_t>(d_comp) - comp_origin;
        a.win_end = comp_origin + (uint64_t)comp_bytes;
        a.offsets = d_offsets;
        a.n = n;
        a.unit = unit;
        a.hdr_mode = layout == SNAPPY_AMD_SINGLE ? SNAPPY_HDR_FIRST_UNIT : SNAPPY_HDR_EVERY_UNIT;
        a.allow_back = layout == SNAPPY_AMD_SINGLE ? 1u : 0u;
        a.slot_cap = cap;
        a.plan = plan;
        a.keys = keys;
        a.slots = c->f_scr;
        a.out = static_cast<uint8_t *>(d_out);
        // launch groups: consecutive units holding at most `cap` edge units, whose slots
        // (edge ordinal mod cap) are therefore distinct; the next group reuses them
        // after this group's clip, in stream order
        size_t p0 = 0;
        while (p0 < nunits) {
            size_t p1 = p0;
            uint32_t edges = 0;
            while (p1 < nunits && (!hunits[p1].edge || edges < cap)) edges += hunits[p1++].edge ? 1u : 0u;
            a.first = p0;
            hipLaunchKernelGGL(kr4_decode_range_units, dim3((uint32_t)(p1 - p0)), dim3(64), 0, c->stream, a);
            if (edges)
                ranges_launch_clip(c->stream, plan, (uint64_t)p0, (uint32_t)(p1 - p0), keys, c->f_scr, cap,
                                   static_cast<uint8_t *>(d_out));
            p0 = p1;
        }
    }
    ranges_launch_status(c->stream, keys, (uint64_t)count, d_status, first);
    HIP_OK(hipGetLastError());
    if (!sync) return SNAPPY_AMD_OK;
    HIP_OK(hipMemcpyAsync(c->h_total, first, sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
    HIP_OK(hipStreamSynchronize(c->stream));
    return *c->h_total == ~0ull ? SNAPPY_AMD_OK : -(int)(*c->h_total & 0xFF);
}

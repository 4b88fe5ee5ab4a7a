// snappy_container_ranges.hip -- range decode of a Hadoop or snappy-java
// container: the decoded bytes [start, start + length) of many ranges through the
// container's chunk tables, from a resident window of the container, every
// touched chunk checked against its table entries (include/snappy_amd.h,
// DESIGN.md 7.8).
//
// The tables are in HBM, so the plan (snappy_container_ranges.h) runs there and
// one read-back of 64 bytes sizes this file's launches:
//
//   KQ0 kq0_plan (one thread per range: refusals, span, unit count, the staged
//       sizes of its at most two edge chunks) -> K3 (the unit counts' scan) ->
//   KQ1 kq1_pack (one thread, over the ranges in order: each edge chunk's place in
//       the staging area and the launch groups) -> read-back ->
//   KQ2 kq2_expand (one thread per unit: its snappy_range_unit) ->
//   KQ3 kq3_tables (one thread per non-empty unit: the table stage) ->
//   KQ4 kq4_derive (a range with a failing unit is refused here, before any
//       decode; every other unit becomes one record of the derived batch: its
//       payload's place in the window, and where it decodes to: the output for an
//       interior unit, its staging place for an edge unit) ->
//   per launch group:
//     the long-record decode of the group's records (snappy_long_records.hip: its
//         plan, the per-record walk of chunks above 65,536 bytes, both K4 passes,
//         the records' status words) ->
//     KQ5 kq5_fold (a failing record's status into its range's key) ->
//     KQ6 kq6_clip (staged[lo, hi) to the output) ->
//   KG7 kr7_range_status (snappy_ranges.hip: keys -> d_status and the first failure)
//
// The long-record decode sizes its own launches by its own 64-byte read-back, one
// per launch group.  A range's key is that of snappy_ranges.hip: ~0 while nothing
// failed; below 256 the refusal made before any decode (-status: the plan's, or
// its lowest failing unit's in the table stage); else (chunk + 1) << 8 | -status
// of its lowest chunk that failed to decode (atomicMin).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <vector>

#include "snappy_amd.h"
#include "snappy_container.h"
#include "snappy_container_ranges.h"
#include "snappy_ctx.h"
#include "snappy_kernels.h"

using namespace snappy_amd;

namespace {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// what the host reads back once the plan is made (64 bytes, through c->h_total)
struct ContainerPlan {
    uint64_t units;   // the scan's total
    uint64_t sum;     // the unit counts added up in 64 bits (the scan's 32-bit partial sums
                      // hold whenever this is below 2^31)
    uint64_t first;   // KG7: min over failing ranges of range << 8 | -status (~0: none)
    uint64_t groups;  // KQ1: launch groups (>= 1)
    uint64_t stage;   // KQ1: bytes of the staging area the fullest group uses
    uint64_t emax;    // KQ1: the longest edge chunk's staged size
    uint64_t pad[2];
};
static_assert(sizeof(ContainerPlan) == 64, "read back through the context's 64 pinned bytes");

// the per-range tables of a call in c->f_meta: 100 bytes per range, and 88
struct RangeTables {
    ContainerPlan *plan;
    unsigned long long *keys, *hkeys;  // hkeys: the table stage's lowest failing unit, (chunk + 1) << 8 | -status
    uint64_t *ubase;                   // count + 1: each range's first unit
    uint64_t *u0;                      // each range's first chunk
    uint64_t *eplace;                  // 2 count: the staging place of the range's first / last edge chunk
    uint64_t *gstart;                  // 2 count + 2: each launch group's first unit
    snappy_amd_range *ranges;
    uint32_t *nunits;
    uint32_t *esize;                   // 2 count: the staged size of those chunks / 16 (0: not an edge unit)
};
size_t range_bytes(size_t count) { return sizeof(ContainerPlan) + 24 + count * (16 + 8 + 8 + 16 + 16 + 24 + 4 + 8); }
RangeTables range_tables(uint8_t *m, size_t count)
{
    RangeTables t;
    t.plan = reinterpret_cast<ContainerPlan *>(m);
    t.keys = reinterpret_cast<unsigned long long *>(m + sizeof(ContainerPlan));
    t.hkeys = t.keys + count;
    t.ubase = reinterpret_cast<uint64_t *>(t.hkeys + count);
    t.u0 = t.ubase + count + 1;
    t.eplace = t.u0 + count;
    t.gstart = t.eplace + 2 * count;
    t.ranges = reinterpret_cast<snappy_amd_range *>(t.gstart + 2 * count + 2);
    t.nunits = reinterpret_cast<uint32_t *>(t.ranges + count);
    t.esize = t.nunits + count;
    return t;
}

// the per-unit tables of a call in c->k5buf: 68 bytes per unit
struct UnitTables {
    snappy_range_unit *plan;
    uint64_t *comp, *outp;  // the derived batch: (offset in the window, length), (address, length); (0, 0) twice
                            // for a unit that is not decoded
    int32_t *ustatus;       // the records' status words of the long-record decode
};
size_t unit_bytes(size_t units) { return units * (32 + 16 + 16 + 4); }
UnitTables unit_tables(uint8_t *m, size_t units)
{
    UnitTables t;
    t.plan = reinterpret_cast<snappy_range_unit *>(m);
    t.comp = reinterpret_cast<uint64_t *>(t.plan + units);
    t.outp = t.comp + 2 * units;
    t.ustatus = reinterpret_cast<int32_t *>(t.outp + 2 * units);
    return t;
}

// KQ0: one thread per range
__global__ __launch_bounds__(256) void kq0_plan(RangeTables t, uint64_t count, const uint64_t *__restrict__ outp,
                                                uint64_t nchunks, uint64_t out_bytes)
{
    const uint64_t r = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= count) return;
    const snappy_amd_range g = t.ranges[r];
    uint64_t u0, u1, k;
    const int32_t st = snappy_container_span(outp, nchunks, g, out_bytes, &u0, &u1, &k);
    uint32_t e0 = 0, e1 = 0;
    if (k) {
        snappy_range_unit e;
        // (an edge unit's chunk holds 1 .. 2^30 bytes: its staged size / 16 fits 32 bits)
        if (snappy_container_unit(outp, g, (uint32_t)r, u0, u1, u0, &e))
            e0 = (uint32_t)(snappy_container_stage_size(outp[2 * u0 + 1]) >> 4);
        if (u1 != u0 && snappy_container_unit(outp, g, (uint32_t)r, u0, u1, u1, &e))
            e1 = (uint32_t)(snappy_container_stage_size(outp[2 * u1 + 1]) >> 4);
        atomicAdd(reinterpret_cast<unsigned long long *>(&t.plan->sum), (unsigned long long)k);
    }
    t.keys[r] = st == SNAPPY_AMD_OK ? ~0ull : (unsigned long long)-st;
    t.hkeys[r] = ~0ull;
    t.u0[r] = u0;
    t.nunits[r] = (uint32_t)k;  // (k <= nchunks < 2^31)
    t.esize[2 * r] = e0;
    t.esize[2 * r + 1] = e1;
}

// KQ1: one thread walks the ranges in order and packs their edge chunks into the
// staging area (snappy_container_pack): a chunk that does not fit behind the ones
// before it opens a launch group, whose first unit is that chunk's.  The walk is
// serial because a place depends on every place before it; it reads 16 bytes per
// range, in order.
__global__ __launch_bounds__(64) void kq1_pack(RangeTables t, uint64_t count, uint64_t budget)
{
    if (threadIdx.x != 0) return;
    uint64_t fill = 0, groups = 1, stage = 0, emax = 0;
    t.gstart[0] = 0;
    for (uint64_t r = 0; r < count; r++) {
        for (uint32_t w = 0; w < 2; w++) {
            const uint64_t need = (uint64_t)t.esize[2 * r + w] << 4;
            if (!need) continue;
            uint64_t place;
            if (snappy_container_pack(budget, need, &fill, &place))
                t.gstart[groups++] = t.ubase[r] + (w ? t.nunits[r] - 1u : 0u);
            t.eplace[2 * r + w] = place;
            stage = fill > stage ? fill : stage;
            emax = need > emax ? need : emax;
        }
    }
    t.plan->groups = groups;
    t.plan->stage = stage;
    t.plan->emax = emax;
}

// KQ2: one thread per unit p: its range is the last r with ubase[r] <= p (a range
// without units shares its entry with the next one)
__global__ __launch_bounds__(256) void kq2_expand(RangeTables t, uint64_t count, uint64_t units,
                                                  const uint64_t *__restrict__ outp,
                                                  snappy_range_unit *__restrict__ plan)
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
    snappy_range_unit e;
    if (snappy_container_unit(outp, g, r, u0, u1, u, &e)) e.edge = 2u * r + (u == u0 ? 1u : 2u);
    plan[p] = e;
}

// KQ3: one thread per unit.  Reads the tables and at most 5 window bytes, none of
// them outside [w0, w1).
__global__ __launch_bounds__(256) void kq3_tables(RangeTables t, const snappy_range_unit *__restrict__ plan,
                                                  uint64_t units, const uint64_t *__restrict__ comp,
                                                  const uint64_t *__restrict__ outp, uintptr_t comp_at, uint64_t w0,
                                                  uint64_t w1)
{
    const uint64_t p = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= units) return;
    const snappy_range_unit e = plan[p];
    if (e.hi == 0 || t.keys[e.range] < 256) return;
    const uint64_t co = comp[2 * e.unit], cl = comp[2 * e.unit + 1];
    uint8_t w[5] = {};
    if (co >= w0 && co <= w1 && cl <= w1 - co) {
        const uint8_t *f = reinterpret_cast<const uint8_t *>(comp_at + co);
#pragma unroll
        for (uint32_t k = 0; k < 5; k++) w[k] = k < cl ? f[k] : (uint8_t)0;
    }
    const int32_t st = snappy_container_unit_check(w, co, cl, w0, w1, outp[2 * e.unit + 1], e.hi);
    if (st != SNAPPY_AMD_OK) atomicMin(t.hkeys + e.range, ((unsigned long long)(e.unit + 1) << 8) | (uint32_t)-st);
}

// KQ4: one thread per unit.  A range the table stage failed becomes a refused one
// (every one of its units writes the same key).  A unit that will be decoded
// becomes a record of the derived batch: its payload counted from the window's
// first byte, its decoded bytes at an address (the batch's output base is null):
// out + land for an interior unit, its staging place for an edge unit.  Every
// other unit is the record (0, 0) (0, 0), which the long-record plan refuses
// (ERR_HEADER, an empty payload) and KQ5 passes over.
__global__ __launch_bounds__(256) void kq4_derive(RangeTables t, const snappy_range_unit *__restrict__ plan,
                                                  uint64_t units, const uint64_t *__restrict__ comp,
                                                  const uint64_t *__restrict__ outp, uint64_t w0, uintptr_t out,
                                                  uintptr_t stage, uint64_t *__restrict__ dcomp,
                                                  uint64_t *__restrict__ doutp)
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
    dcomp[2 * p] = live ? comp[2 * e.unit] - w0 : 0;
    dcomp[2 * p + 1] = live ? comp[2 * e.unit + 1] : 0;
    doutp[2 * p] = !live ? 0 : e.edge ? stage + t.eplace[e.edge - 1] : out + e.land;
    doutp[2 * p + 1] = live ? outp[2 * e.unit + 1] : 0;
}

// KQ5: one thread per unit of the group: a decoded record's failure is its chunk's
__global__ __launch_bounds__(256) void kq5_fold(const snappy_range_unit *__restrict__ plan, uint64_t first,
                                                uint64_t units, const uint64_t *__restrict__ dcomp,
                                                const int32_t *__restrict__ ustatus,
                                                unsigned long long *__restrict__ keys)
{
    const uint64_t j = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= units) return;
    const uint64_t p = first + j;
    if (dcomp[2 * p + 1] == 0) return;
    const int32_t st = ustatus[p];
    if (st != SNAPPY_AMD_OK)
        atomicMin(keys + plan[p].range, ((unsigned long long)(plan[p].unit + 1) << 8) | (uint32_t)-st);
}

constexpr uint32_t kClipTile = 65536;

// KQ6: workgroup (b, y) (256 threads) copies tile y of the wanted bytes [lo, hi) of
// planned unit first + b from its staging place to the output at land + [lo, hi);
// interior units and the units of a range that has failed leave at once.  The
// destination is cut at its 16-byte boundaries, as kr6_clip cuts it: bytes up to
// the first (tile 0), then the body in tiles of 65,536 bytes -- 16-byte stores
// when the source is 16-aligned there too (start and out_offset agree mod 16), else
// dword stores each funnel-shifted out of two aligned source dwords -- then the
// bytes after the last (tile 0).
__global__ __launch_bounds__(256) void kq6_clip(const snappy_range_unit *__restrict__ plan, uint64_t first,
                                                const unsigned long long *__restrict__ keys,
                                                const uint64_t *__restrict__ eplace,
                                                const uint8_t *__restrict__ stage, uint8_t *__restrict__ out)
{
    const snappy_range_unit e = plan[first + blockIdx.x];
    if (e.edge == 0 || keys[e.range] != ~0ull) return;
    const uint32_t len = e.hi - e.lo, t = threadIdx.x, y = blockIdx.y;
    if (y && (uint64_t)y * kClipTile >= len) return;
    const uint8_t *const src = stage + eplace[e.edge - 1] + e.lo;
    uint8_t *const dst = reinterpret_cast<uint8_t *>(reinterpret_cast<uintptr_t>(out) + e.land + e.lo);
    const uint32_t h0 = (uint32_t)(-reinterpret_cast<uintptr_t>(dst) & 15);
    const uint32_t h = h0 < len ? h0 : len;
    const uint32_t body = (len - h) & ~15u;
    if (y == 0) {
        if (t < h) dst[t] = src[t];
        const uint32_t done = h + body;
        if (done + t < len) dst[done + t] = src[done + t];
    }
    const uint32_t b0 = y * kClipTile, b1 = body - b0 < kClipTile ? body : b0 + kClipTile;
    if (b0 >= body) return;
    const uint8_t *const s = src + h;
    uint8_t *const d = dst + h;
    const uint32_t sa = (uint32_t)(reinterpret_cast<uintptr_t>(s) & 3);
    if ((reinterpret_cast<uintptr_t>(s) & 15) == 0) {
        for (uint32_t x = b0 + 16 * t; x < b1; x += 16 * 256)
            *reinterpret_cast<u32x4 *>(d + x) = *reinterpret_cast<const u32x4 *>(s + x);
    } else {
        // (the dword after the last one holding a wanted byte is read only for sa != 0,
        // and then holds the body's last bytes: it lies inside the chunk's staged size)
        const uint32_t *const s4 = reinterpret_cast<const uint32_t *>(s - sa);
        uint32_t *const d4 = reinterpret_cast<uint32_t *>(d);
        for (uint32_t j = b0 / 4 + t; j < b1 / 4; j += 256) {
            const uint32_t lo = s4[j];
            d4[j] = sa ? __builtin_amdgcn_alignbit(s4[j + 1], lo, 8 * sa) : lo;
        }
    }
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

extern "C" int snappy_amd_decompress_container_ranges_device(snappy_amd_ctx *c, const void *d_window,
                                                             uint64_t comp_origin, size_t comp_bytes,
                                                             const uint64_t *d_comp_off_len,
                                                             const uint64_t *d_out_off_len, size_t nchunks,
                                                             const snappy_amd_range *ranges, size_t count, void *d_out,
                                                             size_t out_bytes, int32_t *d_status)
{
    if (!c || (count && !ranges) || (!d_window && comp_bytes) || (!d_out && out_bytes)) return SNAPPY_AMD_ERR_ARG;
    // (a unit's edge word holds 2 range + 2 in 32 bits; the long-record call numbers records in 31)
    if (count > 0x7FFFFFFEull || nchunks > 0x7FFFFFFEull) return SNAPPY_AMD_ERR_ARG;
    if (comp_origin + (uint64_t)comp_bytes < comp_origin) return SNAPPY_AMD_ERR_ARG;
    if (count == 0) return SNAPPY_AMD_OK;
    if (nchunks && (!d_comp_off_len || !d_out_off_len)) return SNAPPY_AMD_ERR_ARG;
    HIP_OK(hipSetDevice(c->device));
    if (ctx_stream(c)) return SNAPPY_AMD_ERR_DEVICE;
    (void)hipGetLastError();  // (a pending error that is not this call's, as in compress_launch)

    // ---- the plan: statuses, spans and unit counts per range, their scan, the packing; one read-back
    int rc;
    if ((rc = grow(reinterpret_cast<void **>(&c->f_meta), &c->f_meta_cap, range_bytes(count)))) return rc;
    const RangeTables t = range_tables(c->f_meta, count);
    const uint64_t budget = (uint64_t)ranges_slot_cap() * SNAPPY_BLOCK;
    HIP_OK(hipMemsetAsync(t.plan, 0, sizeof(ContainerPlan), c->stream));
    HIP_OK(hipMemsetAsync(&t.plan->first, 0xFF, sizeof(uint64_t), c->stream));
    HIP_OK(hipMemcpyAsync(t.ranges, ranges, count * sizeof(snappy_amd_range), hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(kq0_plan, dim3(blocks_of(count, 256)), dim3(256), 0, c->stream, t, (uint64_t)count,
                       d_out_off_len, (uint64_t)nchunks, (uint64_t)out_bytes);
    scan(c, t.nunits, count, t.ubase, &t.plan->units);
    hipLaunchKernelGGL(kq1_pack, dim3(1), dim3(64), 0, c->stream, t, (uint64_t)count, budget);
    HIP_OK(hipGetLastError());
    ContainerPlan *const hp = reinterpret_cast<ContainerPlan *>(c->h_total);
    HIP_OK(hipMemcpyAsync(hp, t.plan, sizeof(ContainerPlan), hipMemcpyDeviceToHost, c->stream));
    HIP_OK(hipStreamSynchronize(c->stream));  // (`ranges` is pageable: its bytes are taken by now, too)
    if (hp->sum > 0x7FFFFFFFull) return SNAPPY_AMD_ERR_ARG;
    const size_t units = (size_t)hp->sum, groups = (size_t)hp->groups, stage = (size_t)hp->stage;
    const uint64_t emax = hp->emax;
    if (groups < 1 || groups > 2 * count + 1) return SNAPPY_AMD_ERR_DEVICE;  // (cannot happen: kq1_pack's)

    if (units) {
        if ((rc = grow(reinterpret_cast<void **>(&c->k5buf), &c->k5buf_cap, unit_bytes(units)))) return rc;
        // (+ 16: room behind the last staged chunk, as the slots of decompress_ranges_device have)
        if (stage && (rc = grow(reinterpret_cast<void **>(&c->f_scr), &c->f_scr_cap, stage + 16))) return rc;
        const UnitTables ut = unit_tables(c->k5buf, units);
        const uintptr_t comp_at = reinterpret_cast<uintptr_t>(d_window) - comp_origin;
        const uint64_t w0 = comp_origin, w1 = comp_origin + (uint64_t)comp_bytes;
        const uint32_t ublocks = blocks_of(units, 256);
        hipLaunchKernelGGL(kq2_expand, dim3(ublocks), dim3(256), 0, c->stream, t, (uint64_t)count, (uint64_t)units,
                           d_out_off_len, ut.plan);
        hipLaunchKernelGGL(kq3_tables, dim3(ublocks), dim3(256), 0, c->stream, t, ut.plan, (uint64_t)units,
                           d_comp_off_len, d_out_off_len, comp_at, w0, w1);
        hipLaunchKernelGGL(kq4_derive, dim3(ublocks), dim3(256), 0, c->stream, t, ut.plan, (uint64_t)units,
                           d_comp_off_len, d_out_off_len, w0, reinterpret_cast<uintptr_t>(d_out),
                           reinterpret_cast<uintptr_t>(c->f_scr), ut.comp, ut.outp);
        HIP_OK(hipGetLastError());
        // launch groups: consecutive units whose edge chunks fit the staging area side by
        // side; the next group reuses it after this group's clip, in stream order.  More
        // than one group: their first units are read back (the only call that reads twice
        // before its decode is one whose edge chunks exceed the budget).
        std::vector<uint64_t> gs(groups + 1, 0);
        gs[groups] = units;
        if (groups > 1) {
            HIP_OK(hipMemcpyAsync(gs.data() + 1, t.gstart + 1, (groups - 1) * sizeof(uint64_t), hipMemcpyDeviceToHost,
                                  c->stream));
            HIP_OK(hipStreamSynchronize(c->stream));
        }
        const uint32_t tiles = emax > kClipTile ? blocks_of(emax, kClipTile) : 1u;
        for (size_t g = 0; g < groups; g++) {
            const uint64_t p0 = gs[g], n = gs[g + 1] - gs[g];
            if (gs[g + 1] < p0 || gs[g + 1] > units) return SNAPPY_AMD_ERR_DEVICE;  // (cannot happen: kq1_pack's)
            if (n == 0) continue;
            if ((rc = long_records_launch_decode(c, d_window, comp_bytes, ut.comp + 2 * p0, (size_t)n, nullptr, 0,
                                                 ut.outp + 2 * p0, nullptr, ut.ustatus + p0, false, 0)))
                return rc;
            hipLaunchKernelGGL(kq5_fold, dim3(blocks_of(n, 256)), dim3(256), 0, c->stream, ut.plan, p0, n, ut.comp,
                               ut.ustatus, t.keys);
            if (stage)
                hipLaunchKernelGGL(kq6_clip, dim3((uint32_t)n, tiles), dim3(256), 0, c->stream, ut.plan, p0, t.keys,
                                   t.eplace, c->f_scr, static_cast<uint8_t *>(d_out));
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

// snappy_long_records.hip -- record batches whose records hold 0 .. 2^30 decoded
// bytes: each record one raw Snappy stream of ceil(L / 65,536) blocks with one
// preamble, as snappy_compress() writes it (include/snappy_amd.h).
//
// A unit is one block of one record (an empty record has one unit, which writes
// or checks its byte 00; a refused record has none).  Units are numbered in
// record order, so record r owns units [ubase[r], ubase[r + 1]) and the table
// entries [tbase[r], tbase[r + 1]): nblk + 1 entries of the SINGLE index format,
// offsets counted from the record's own first compressed byte.
//
// Compress:  KL0 (plan, one thread per record) -> K3 x 2 (ubase, tbase) ->
//            read-back -> KL1 (expansion, one thread per unit) -> K3 (scratch
//            offsets) -> KR1 / KR1-64 over the unit lists -> K3 (unit offsets) ->
//            KR2 -> KL2 (d_offsets and the tables)
// Index:     KL0d -> K3 -> read-back -> KR5 (one wave per record)
// Decode:    KL0d -> K3 x 2 -> read-back -> KL1d -> [KR5] -> KR4 pass 1 -> KR4
//            pass 2 -> KL3 (the records' status words, the first failure)
//
// The match rounds, the emit passes, the walk and the element decode are the
// bodies of snappy_kernels.hip, entered through the unit entry points there.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "snappy_amd.h"
#include "snappy_ctx.h"
#include "snappy_kernels.h"

using namespace snappy_amd;

namespace {

constexpr uint64_t kLongMax = SNAPPY_AMD_LONG_RECORD_MAX;

// what the host reads back once the plan is made (64 bytes, through c->h_total);
// the device copy also holds the expansion's list cursors and pass 1's batch flag
struct LongPlan {
    uint64_t scratch_words;  // the sum of the units' scratch needs
    uint64_t sum;            // bytes of the accepted records
    uint64_t first;          // min over failing records of record << 8 | -status (~0: none)
    uint64_t units;          // K3's total over the records' units
    uint64_t entries;        // K3's total over the records' table entries
    uint32_t n_small, n_big; // units of 1 .. 32,768 bytes (K1r), of 32,769 .. 65,536 (K1r64)
    uint32_t c_small, c_big; // the expansion's cursors into the two lists
    uint32_t longest;        // the longest unit
    uint32_t defer;          // decode: pass 1 deferred a unit of some record
};
static_assert(sizeof(LongPlan) == 64, "read back through the context's 64 pinned bytes");

// the per-record tables of a call in c->r_meta
struct RecTables {
    LongPlan *plan;
    uint64_t *ubase;    // count + 1: each record's first unit
    uint64_t *tbase;    // count + 1: each record's first table entry
    uint32_t *nunits;   // count
    uint32_t *nent;     // count
    int32_t *status;    // count: 0, or the record's refusal / index failure
};
size_t rec_bytes(size_t count) { return sizeof(LongPlan) + (count + 1) * 16 + count * 12; }
RecTables rec_tables(uint8_t *m, size_t count)
{
    RecTables t;
    t.plan = reinterpret_cast<LongPlan *>(m);
    t.ubase = reinterpret_cast<uint64_t *>(m + sizeof(LongPlan));
    t.tbase = t.ubase + count + 1;
    t.nunits = reinterpret_cast<uint32_t *>(t.tbase + count + 1);
    t.nent = t.nunits + count;
    t.status = reinterpret_cast<int32_t *>(t.nent + count);
    return t;
}

// the per-unit tables of a compress call in c->seg_off (a buffer the record
// calls do not otherwise use: the units' segment records live in the token scratch)
struct UnitTables {
    uint64_t *sbase;       // units + 1: each unit's scratch offset (u32 words)
    uint64_t *uoff;        // units + 1: each unit's place in d_out
    uint32_t *urec;        // units: the unit's record
    uint32_t *need;        // units: its scratch need (0: an empty record's unit)
    uint32_t *list_small;  // units
    uint32_t *list_big;    // units
};
size_t unit_bytes(size_t units) { return (units + 1) * 16 + units * 16; }
UnitTables unit_tables(uint32_t *m, size_t units)
{
    UnitTables t;
    t.sbase = reinterpret_cast<uint64_t *>(m);
    t.uoff = t.sbase + units + 1;
    t.urec = reinterpret_cast<uint32_t *>(t.uoff + units + 1);
    t.need = t.urec + units;
    t.list_small = t.need + units;
    t.list_big = t.list_small + units;
    return t;
}

uint32_t blocks_of(uint64_t items, uint32_t per) { return (uint32_t)((items + per - 1) / per); }

__device__ __forceinline__ uint32_t rank_in(uint64_t mask, uint32_t lane)
{
    return (uint32_t)__builtin_popcountll(mask & ((1ull << lane) - 1));
}

__device__ __forceinline__ uint64_t wave_sum(uint64_t v)
{
    for (uint32_t d = 32; d; d >>= 1) v += __shfl_xor(v, d);
    return v;
}

// KL0: one thread per record of a compress call.  Checks the descriptor (the
// length first, so a record above the cap is named without owning its bytes), sets
// the record's status, its units (its blocks; one for an empty record, none for a
// refused one) and its table entries (blocks + 1), and adds what the host sizes
// the launches by: the accepted bytes, the units of each class, their scratch
// words.  No byte of any record is read.
__global__ __launch_bounds__(256) void kl0_plan_compress(const uint64_t *__restrict__ off_len, uint64_t count,
                                                         uint64_t in_bytes, uint32_t *__restrict__ nunits,
                                                         uint32_t *__restrict__ nent, int32_t *__restrict__ status,
                                                         LongPlan *__restrict__ po)
{
    const uint64_t r = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    const uint32_t lane = threadIdx.x & 63;
    const bool live = r < count;
    uint64_t off = 0, L = 0;
    if (live) {
        off = off_len[2 * r];
        L = off_len[2 * r + 1];
    }
    int32_t st = SNAPPY_ST_OK;
    if (L > kLongMax) st = SNAPPY_ST_UNSUPPORTED;
    else if (off > in_bytes || L > in_bytes - off) st = -1;  // SNAPPY_AMD_ERR_ARG
    const bool ok = live && st == SNAPPY_ST_OK;
    if (!ok) L = 0;
    const uint32_t full = (uint32_t)(L / SNAPPY_BLOCK), tail = (uint32_t)(L % SNAPPY_BLOCK);
    const uint32_t nblk = full + (tail ? 1u : 0u);
    if (live) {
        nunits[r] = ok ? (nblk ? nblk : 1u) : 0u;
        nent[r] = nblk + 1;
        status[r] = st;
        if (!ok) atomicMin(reinterpret_cast<unsigned long long *>(&po->first), (r << 8) | (uint32_t)-st);
    }
    const uint32_t small = tail >= 1 && tail <= SNAPPY_K1R_MAX_UNIT ? 1u : 0u;
    const uint32_t big = full + (tail > SNAPPY_K1R_MAX_UNIT ? 1u : 0u);
    const uint64_t words = (uint64_t)full * records_need_words(SNAPPY_BLOCK) + (tail ? records_need_words(tail) : 0u);
    const uint32_t unit_max = full ? SNAPPY_BLOCK : tail;
    const uint64_t s_sum = wave_sum(L), s_small = wave_sum(small), s_big = wave_sum(big), s_words = wave_sum(words);
    uint32_t mx = unit_max;
    for (uint32_t d = 32; d; d >>= 1) {
        const uint32_t o = __shfl_xor(mx, d);
        mx = o > mx ? o : mx;
    }
    if (lane == 0 && s_sum) {
        atomicAdd(reinterpret_cast<unsigned long long *>(&po->sum), s_sum);
        atomicAdd(reinterpret_cast<unsigned long long *>(&po->scratch_words), s_words);
        if (s_small) atomicAdd(&po->n_small, (uint32_t)s_small);
        if (s_big) atomicAdd(&po->n_big, (uint32_t)s_big);
        atomicMax(&po->longest, mx);
    }
}

// KL0d: one thread per record of an index or decode call.  The checks that come
// before anything of a record is loaded or stored, with the short call's
// meanings: a decoded length above the cap UNSUPPORTED, a compressed range
// outside comp_bytes TRUNCATED, an output range outside out_bytes CAPACITY
// (decode only: check_out), an empty compressed range HEADER.
__global__ __launch_bounds__(256) void kl0_plan_decode(const uint64_t *__restrict__ comp_off_len,
                                                       const uint64_t *__restrict__ out_off_len, uint64_t count,
                                                       uint64_t comp_bytes, uint64_t out_bytes, uint32_t check_out,
                                                       uint32_t *__restrict__ nunits, uint32_t *__restrict__ nent,
                                                       int32_t *__restrict__ status)
{
    const uint64_t r = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= count) return;
    const uint64_t co = comp_off_len[2 * r], cl = comp_off_len[2 * r + 1];
    const uint64_t oo = out_off_len[2 * r], ol = out_off_len[2 * r + 1];
    int32_t st = SNAPPY_ST_OK;
    if (ol > kLongMax) st = SNAPPY_ST_UNSUPPORTED;
    else if (co > comp_bytes || cl > comp_bytes - co) st = SNAPPY_ST_TRUNCATED;
    else if (check_out && (oo > out_bytes || ol > out_bytes - oo)) st = SNAPPY_ST_CAPACITY;
    else if (cl == 0) st = SNAPPY_ST_HEADER;
    const uint32_t nblk = st == SNAPPY_ST_OK ? (uint32_t)((ol + SNAPPY_BLOCK - 1) / SNAPPY_BLOCK) : 0u;
    nunits[r] = st == SNAPPY_ST_OK ? (nblk ? nblk : 1u) : 0u;
    nent[r] = nblk + 1;
    status[r] = st;
}

// the record of unit u: the last r with ubase[r] <= u (records without units share
// their successor's base, and own no u)
__device__ __forceinline__ uint32_t record_of(const uint64_t *__restrict__ ubase, uint64_t count, uint64_t u)
{
    uint64_t lo = 0, hi = count;  // ubase[lo] <= u < ubase[hi]
    while (hi - lo > 1) {
        const uint64_t mid = (lo + hi) / 2;
        if (ubase[mid] <= u) lo = mid;
        else hi = mid;
    }
    return (uint32_t)lo;
}

// KL1: one thread per unit finds its record by binary search over the scanned
// unit bases and writes the unit -> record word, the unit's scratch need and its
// preset size and token count (K1r overwrites a matched unit's; an empty record's
// unit keeps size 1, the byte 00), and appends the unit to its class's list (one
// atomic per wave and class).
__global__ __launch_bounds__(256) void kl1_expand_compress(const uint64_t *__restrict__ off_len, uint64_t count,
                                                           const uint64_t *__restrict__ ubase, uint64_t units,
                                                           uint32_t *__restrict__ urec, uint32_t *__restrict__ need,
                                                           uint32_t *__restrict__ list_small,
                                                           uint32_t *__restrict__ list_big, uint32_t *__restrict__ sizes,
                                                           uint32_t *__restrict__ ntok, LongPlan *__restrict__ po)
{
    const uint64_t u = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    const uint32_t lane = threadIdx.x & 63;
    const bool live = u < units;
    uint32_t L = 0;
    if (live) {
        const uint32_t r = record_of(ubase, count, u);
        const uint64_t len = off_len[2 * (uint64_t)r + 1], at = (u - ubase[r]) * SNAPPY_BLOCK;
        L = (uint32_t)(len - at < SNAPPY_BLOCK ? len - at : SNAPPY_BLOCK);
        urec[u] = r;
        need[u] = L ? records_need_words(L) : 0u;
        sizes[u] = L ? 0u : 1u;
        ntok[u] = 0;
    }
    const bool small = live && L >= 1 && L <= SNAPPY_K1R_MAX_UNIT, big = live && L > SNAPPY_K1R_MAX_UNIT;
    const uint64_t ms = __ballot(small), mb = __ballot(big);
    uint32_t bs = 0, bb = 0;
    if (lane == 0) {
        if (ms) bs = atomicAdd(&po->c_small, (uint32_t)__builtin_popcountll(ms));
        if (mb) bb = atomicAdd(&po->c_big, (uint32_t)__builtin_popcountll(mb));
    }
    bs = __builtin_amdgcn_readfirstlane(bs);
    bb = __builtin_amdgcn_readfirstlane(bb);
    if (small) list_small[bs + rank_in(ms, lane)] = (uint32_t)u;
    if (big) list_big[bb + rank_in(mb, lane)] = (uint32_t)u;
}

// KL1d: the unit -> record words of a decode call
__global__ __launch_bounds__(256) void kl1_expand_decode(const uint64_t *__restrict__ ubase, uint64_t count,
                                                         uint64_t units, uint32_t *__restrict__ urec)
{
    const uint64_t u = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (u < units) urec[u] = record_of(ubase, count, u);
}

// KL2: d_offsets and the tables from the units' places.  Thread i < units writes
// its unit's table entry (its place minus the record's start; a record's last
// block also the record's compressed length); thread i <= count writes
// d_offsets[i] (a record's first unit's place; the total for i = count) and the
// one entry 0 of a record without blocks.
__global__ __launch_bounds__(256) void kl2_offsets_tables(const uint64_t *__restrict__ off_len, uint64_t count,
                                                          const uint64_t *__restrict__ ubase,
                                                          const uint64_t *__restrict__ tbase,
                                                          const uint32_t *__restrict__ urec, uint64_t units,
                                                          const uint64_t *__restrict__ uoff,
                                                          uint64_t *__restrict__ offsets, uint64_t *__restrict__ index)
{
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i <= count) {
        offsets[i] = uoff[i < count ? ubase[i] : units];
        if (index && i < count && ubase[i] == ubase[i + 1]) index[tbase[i]] = 0;
    }
    if (index && i < units) {
        const uint32_t r = urec[i];
        const uint64_t u0 = ubase[r], start = uoff[u0];
        uint64_t *const table = index + tbase[r];
        table[i - u0] = uoff[i] - start;
        if (i + 1 == ubase[r + 1] && off_len[2 * (uint64_t)r + 1] != 0) table[i - u0 + 1] = uoff[i + 1] - start;
    }
}

// KL3: one wave per record folds its units' status words into the record's, as
// the SINGLE call reports a stream: the first failing block's status in block
// order, a unit pass 2 left deferred an internal failure.  A record the plan or
// the index failed keeps that status.  *first = min over failing records.
__global__ __launch_bounds__(64) void kl3_record_status(const uint64_t *__restrict__ ubase,
                                                        const int32_t *__restrict__ rstatus,
                                                        const int32_t *__restrict__ ustatus,
                                                        int32_t *__restrict__ status,
                                                        unsigned long long *__restrict__ first)
{
    const uint32_t r = blockIdx.x, lane = threadIdx.x;
    int32_t st = rstatus[r];
    if (st == SNAPPY_ST_OK) {
        const uint64_t u0 = ubase[r], n = ubase[r + 1] - u0;
        const int32_t *s = ustatus + u0 + 2 * (uint64_t)r;
        uint64_t key = ~0ull;  // block << 8 | -status of the first failing block this lane saw
        for (uint64_t b = lane; b < n; b += 64) {
            const int32_t v = s[b];
            if (v != SNAPPY_ST_OK && key == ~0ull) key = (b << 8) | (uint32_t)(v > 0 ? 7 : -v);  // (7: ERR_DEVICE)
        }
        for (uint32_t d = 32; d; d >>= 1) {
            const uint64_t o = __shfl_xor(key, d);
            key = o < key ? o : key;
        }
        if (key != ~0ull) st = -(int32_t)(key & 0xFF);
    }
    if (lane == 0) {
        if (status) status[r] = st;
        if (st != SNAPPY_ST_OK) atomicMin(first, ((unsigned long long)r << 8) | (uint32_t)-st);
    }
}

int call_begin(snappy_amd_ctx *c)
{
    HIP_OK(hipSetDevice(c->device));
    if (ctx_stream(c)) return SNAPPY_AMD_ERR_DEVICE;
    (void)hipGetLastError();  // (a pending error that is not this call's, as in compress_launch)
    return SNAPPY_AMD_OK;
}

int first_status(uint64_t first) { return first == ~0ull ? SNAPPY_AMD_OK : -(int)(first & 0xFF); }

void scan(snappy_amd_ctx *c, const uint32_t *v, uint64_t count, uint64_t *offsets, uint64_t *total)
{
    if (count <= SNAPPY_K3_WAVE_MAX)
        hipLaunchKernelGGL(k3_scan_wave, dim3(1), dim3(64), 0, c->stream, v, count, offsets, total);
    else
        hipLaunchKernelGGL(k3_scan, dim3(1), dim3(1024), 0, c->stream, v, count, offsets, total);
}

// The plan of an index or decode call: the per-record tables in c->r_meta, the
// two scans and the read-back of their totals into *p.
int plan_decode(snappy_amd_ctx *c, size_t comp_bytes, const uint64_t *d_comp_off_len, size_t count, size_t out_bytes,
                const uint64_t *d_out_off_len, bool check_out, RecTables *t, LongPlan *p)
{
    int rc;
    if ((rc = grow(reinterpret_cast<void **>(&c->r_meta), &c->r_meta_cap, rec_bytes(count)))) return rc;
    *t = rec_tables(c->r_meta, count);
    HIP_OK(hipMemsetAsync(t->plan, 0, sizeof(LongPlan), c->stream));
    HIP_OK(hipMemsetAsync(&t->plan->first, 0xFF, sizeof(uint64_t), c->stream));
    hipLaunchKernelGGL(kl0_plan_decode, dim3(blocks_of(count, 256)), dim3(256), 0, c->stream, d_comp_off_len,
                       d_out_off_len, (uint64_t)count, (uint64_t)comp_bytes, (uint64_t)out_bytes, check_out ? 1u : 0u,
                       t->nunits, t->nent, t->status);
    scan(c, t->nunits, count, t->ubase, &t->plan->units);
    scan(c, t->nent, count, t->tbase, &t->plan->entries);
    HIP_OK(hipGetLastError());
    LongPlan *const hp = reinterpret_cast<LongPlan *>(c->h_total);
    HIP_OK(hipMemcpyAsync(hp, t->plan, sizeof(LongPlan), hipMemcpyDeviceToHost, c->stream));
    HIP_OK(hipStreamSynchronize(c->stream));
    *p = *hp;
    return SNAPPY_AMD_OK;
}

}  // namespace

extern "C" {

size_t snappy_amd_max_long_records_output(size_t total_bytes, size_t count)
{
    return total_bytes + total_bytes / 32 + 32 * (count + total_bytes / SNAPPY_BLOCK) + 16;
}

size_t snappy_amd_max_records_index(size_t total_bytes, size_t count)
{
    return total_bytes / SNAPPY_BLOCK + 2 * count;
}

size_t snappy_amd_max_long_records_scratch(size_t total_bytes, size_t count)
{
    // U units and E table entries at the most (the derivation: include/snappy_amd.h)
    const size_t U = total_bytes / SNAPPY_BLOCK + count, E = total_bytes / SNAPPY_BLOCK + 2 * count;
    const size_t need = 2 * total_bytes + total_bytes / 128 + 80 * U + 64 * count + 8 * E + 512;
    // each of the six buffers may carry grow()'s slack: an eighth and a page
    return need + need / 8 + 6 * 4096 + 128;
}

int snappy_amd_compress_long_records_device(snappy_amd_ctx *c, const void *d_in, size_t in_bytes,
                                            const uint64_t *d_in_off_len, size_t count, void *d_out, size_t out_cap,
                                            uint64_t *d_offsets, uint64_t *d_index, size_t index_cap,
                                            int32_t *d_status, size_t *out_len)
{
    if (!c || (!d_in && in_bytes) || !d_offsets || (count && (!d_in_off_len || !d_out))) return SNAPPY_AMD_ERR_ARG;
    if (count > 0x7FFFFFFFull) return SNAPPY_AMD_ERR_ARG;
    int rc = call_begin(c);
    if (rc) return rc;
    if (count == 0) {
        HIP_OK(hipMemsetAsync(d_offsets, 0, sizeof(uint64_t), c->stream));
        if (out_len) *out_len = 0;
        return SNAPPY_AMD_OK;
    }
    if ((rc = grow(reinterpret_cast<void **>(&c->r_meta), &c->r_meta_cap, rec_bytes(count)))) return rc;
    const RecTables t = rec_tables(c->r_meta, count);
    const uint64_t *ol = d_in_off_len;
    const uint8_t *in = static_cast<const uint8_t *>(d_in);

    // ---- the plan: statuses, units and entries per record, their scans; one read-back
    HIP_OK(hipMemsetAsync(t.plan, 0, sizeof(LongPlan), c->stream));
    HIP_OK(hipMemsetAsync(&t.plan->first, 0xFF, sizeof(uint64_t), c->stream));
    hipLaunchKernelGGL(kl0_plan_compress, dim3(blocks_of(count, 256)), dim3(256), 0, c->stream, ol, (uint64_t)count,
                       (uint64_t)in_bytes, t.nunits, t.nent, t.status, t.plan);
    scan(c, t.nunits, count, t.ubase, &t.plan->units);
    scan(c, t.nent, count, t.tbase, &t.plan->entries);
    HIP_OK(hipGetLastError());
    LongPlan *const hp = reinterpret_cast<LongPlan *>(c->h_total);
    HIP_OK(hipMemcpyAsync(hp, t.plan, sizeof(LongPlan), hipMemcpyDeviceToHost, c->stream));
    HIP_OK(hipStreamSynchronize(c->stream));
    const LongPlan p = *hp;
    if (out_cap < snappy_amd_max_long_records_output((size_t)p.sum, count)) return SNAPPY_AMD_ERR_CAPACITY;
    if (d_index && index_cap < p.entries) return SNAPPY_AMD_ERR_CAPACITY;
    if (p.units > 0x7FFFFFFFull) return SNAPPY_AMD_ERR_ARG;
    const size_t units = (size_t)p.units;
    if ((rc = grow(reinterpret_cast<void **>(&c->seg_off), &c->seg_off_cap, unit_bytes(units)))) return rc;
    if ((rc = grow(reinterpret_cast<void **>(&c->sizes), &c->sizes_cap, (units + 1) * sizeof(uint32_t)))) return rc;
    if ((rc = grow(reinterpret_cast<void **>(&c->ntok), &c->ntok_cap, (units + 1) * sizeof(uint32_t)))) return rc;
    // (+ 64: K2 lanes with no literal read 20 bytes at their unit's first token words)
    if ((rc = grow(reinterpret_cast<void **>(&c->tokens), &c->tokens_cap, p.scratch_words * sizeof(uint32_t) + 64)))
        return rc;
    const UnitTables ut = unit_tables(c->seg_off, units);
    uint32_t *scratch = static_cast<uint32_t *>(c->tokens);

    if (units) {
        // ---- the expansion, the scratch offsets, each match kernel over its class
        hipLaunchKernelGGL(kl1_expand_compress, dim3(blocks_of(units, 256)), dim3(256), 0, c->stream, ol,
                           (uint64_t)count, t.ubase, (uint64_t)units, ut.urec, ut.need, ut.list_small, ut.list_big,
                           c->sizes, c->ntok, t.plan);
        scan(c, ut.need, units, ut.sbase, &t.plan->scratch_words);
        if (p.n_small)
            hipLaunchKernelGGL(kr1_match_lunits, dim3(p.n_small), dim3(64), 0, c->stream, in, ol, ut.list_small, ut.urec,
                               t.ubase, ut.sbase, scratch, c->ntok, c->sizes);
        if (p.n_big)
            hipLaunchKernelGGL(kr1_match_lunits64, dim3(p.n_big), dim3(64), 0, c->stream, in, ol, ut.list_big, ut.urec,
                               t.ubase, ut.sbase, scratch, c->ntok, c->sizes);
        HIP_OK(hipGetLastError());
    }
    // ---- every unit's place in d_out, the emit, d_offsets and the tables
    scan(c, c->sizes, units, ut.uoff, c->total);
    if (units) {
        // no more waves per unit than the longest unit has segments (1: only empty records)
        const uint32_t segs = p.longest ? records_segs(p.longest) : 1u;
        hipLaunchKernelGGL(kr2_emit_lunits, dim3((uint32_t)units, segs < SNAPPY_K2_WAVES ? segs : SNAPPY_K2_WAVES),
                           dim3(64), 0, c->stream, in, ol, ut.urec, t.ubase, ut.sbase, scratch, c->ntok, ut.uoff,
                           static_cast<uint8_t *>(d_out));
    }
    const uint64_t threads = units > count + 1 ? units : count + 1;
    hipLaunchKernelGGL(kl2_offsets_tables, dim3(blocks_of(threads, 256)), dim3(256), 0, c->stream, ol, (uint64_t)count,
                       t.ubase, t.tbase, ut.urec, (uint64_t)units, ut.uoff, d_offsets, d_index);
    HIP_OK(hipGetLastError());
    if (d_status)
        HIP_OK(hipMemcpyAsync(d_status, t.status, count * sizeof(int32_t), hipMemcpyDeviceToDevice, c->stream));
    if (out_len) {
        HIP_OK(hipMemcpyAsync(c->h_total, c->total, sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
        HIP_OK(hipStreamSynchronize(c->stream));
        *out_len = (size_t)*c->h_total;
    }
    return first_status(p.first);
}

int snappy_amd_records_index_device(snappy_amd_ctx *c, const void *d_comp, size_t comp_bytes,
                                    const uint64_t *d_comp_off_len, size_t count, const uint64_t *d_out_off_len,
                                    uint64_t *d_index, size_t index_cap, int32_t *d_status)
{
    if (!c || (!d_comp && comp_bytes) || (count && (!d_comp_off_len || !d_out_off_len || !d_index)))
        return SNAPPY_AMD_ERR_ARG;
    if (count > 0x7FFFFFFFull) return SNAPPY_AMD_ERR_ARG;
    if (count == 0) return SNAPPY_AMD_OK;
    int rc = call_begin(c);
    if (rc) return rc;
    RecTables t;
    LongPlan p;
    if ((rc = plan_decode(c, comp_bytes, d_comp_off_len, count, 0, d_out_off_len, false, &t, &p))) return rc;
    if (index_cap < p.entries) return SNAPPY_AMD_ERR_CAPACITY;
    hipLaunchKernelGGL(kr5_index_lrecords, dim3((uint32_t)count), dim3(64), 0, c->stream,
                       static_cast<const uint8_t *>(d_comp), d_comp_off_len, d_out_off_len, t.tbase, d_index, t.status);
    HIP_OK(hipGetLastError());
    if (d_status)
        HIP_OK(hipMemcpyAsync(d_status, t.status, count * sizeof(int32_t), hipMemcpyDeviceToDevice, c->stream));
    return SNAPPY_AMD_OK;
}

int snappy_amd_decompress_long_records_device(snappy_amd_ctx *c, const void *d_comp, size_t comp_bytes,
                                              const uint64_t *d_comp_off_len, size_t count, void *d_out,
                                              size_t out_bytes, const uint64_t *d_out_off_len, const uint64_t *d_index,
                                              int32_t *d_status, int sync)
{
    if (!c || (!d_comp && comp_bytes) || (!d_out && out_bytes) || (count && (!d_comp_off_len || !d_out_off_len)))
        return SNAPPY_AMD_ERR_ARG;
    if (count > 0x7FFFFFFFull) return SNAPPY_AMD_ERR_ARG;
    if (count == 0) return SNAPPY_AMD_OK;
    int rc = call_begin(c);
    if (rc) return rc;
    return long_records_launch_decode(c, d_comp, comp_bytes, d_comp_off_len, count, d_out, out_bytes, d_out_off_len,
                                      d_index, d_status, true, sync);
}

}  // extern "C"

// ---- shared with the container range decode (snappy_container_ranges.hip; declared in
// snappy_kernels.h): the decode of a checked batch on c->stream.  check_out = false: the
// output offsets are the caller's own (they count from d_out, which may be null: then
// they are addresses) and no record is refused for leaving [0, out_bytes).
int snappy_amd::long_records_launch_decode(snappy_amd_ctx *c, const void *d_comp, size_t comp_bytes,
                                           const uint64_t *d_comp_off_len, size_t count, void *d_out, size_t out_bytes,
                                           const uint64_t *d_out_off_len, const uint64_t *d_index, int32_t *d_status,
                                           bool check_out, int sync)
{
    int rc;
    RecTables t;
    LongPlan p;
    if ((rc = plan_decode(c, comp_bytes, d_comp_off_len, count, out_bytes, d_out_off_len, check_out, &t, &p)))
        return rc;
    if (p.units > 0x7FFFFFFFull) return SNAPPY_AMD_ERR_ARG;
    const size_t units = (size_t)p.units;
    // per unit the unit -> record word and a status word, per record pass 2's two words
    const size_t status_words = units + 2 * count;
    if ((rc = grow(reinterpret_cast<void **>(&c->seg_off), &c->seg_off_cap, (units + status_words) * sizeof(uint32_t))))
        return rc;
    uint32_t *urec = c->seg_off;
    int32_t *ustatus = reinterpret_cast<int32_t *>(c->seg_off + units);
    HIP_OK(hipMemsetAsync(ustatus, 0, status_words * sizeof(int32_t), c->stream));
    const uint8_t *base = static_cast<const uint8_t *>(d_comp);
    const uint64_t *index = d_index;
    if (!index) {
        // the tables of a caller that passes none: built in scratch by the one-wave walk
        if ((rc = grow(reinterpret_cast<void **>(&c->d_idx), &c->d_idx_cap, (size_t)p.entries * sizeof(uint64_t))))
            return rc;
        hipLaunchKernelGGL(kr5_index_lrecords, dim3((uint32_t)count), dim3(64), 0, c->stream, base, d_comp_off_len,
                           d_out_off_len, t.tbase, c->d_idx, t.status);
        index = c->d_idx;
    }
    if (units) {
        hipLaunchKernelGGL(kl1_expand_decode, dim3(blocks_of(units, 256)), dim3(256), 0, c->stream, t.ubase,
                           (uint64_t)count, (uint64_t)units, urec);
        K4LongArgs a;
        // the kernels read aligned dwords: pass the base as an aligned pointer + bias
        a.bias = (uint32_t)(reinterpret_cast<uintptr_t>(d_comp) & 3);
        a.comp = base - a.bias;
        a.comp_off_len = d_comp_off_len;
        a.out_off_len = d_out_off_len;
        a.urec = urec;
        a.ubase = t.ubase;
        a.tbase = t.tbase;
        a.index = index;
        a.rstatus = t.status;
        a.ustatus = ustatus;
        a.defer = &t.plan->defer;
        a.out = static_cast<uint8_t *>(d_out);
        hipLaunchKernelGGL(kr4_decode_lunits, dim3((uint32_t)units), dim3(64), 0, c->stream, a);
        hipLaunchKernelGGL(kr4_back_lunits, dim3((uint32_t)units), dim3(64), 0, c->stream, a);
    }
    unsigned long long *first = reinterpret_cast<unsigned long long *>(&t.plan->first);
    hipLaunchKernelGGL(kl3_record_status, dim3((uint32_t)count), dim3(64), 0, c->stream, t.ubase, t.status, ustatus,
                       d_status, first);
    HIP_OK(hipGetLastError());
    if (!sync) return SNAPPY_AMD_OK;
    HIP_OK(hipMemcpyAsync(c->h_total, first, sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
    HIP_OK(hipStreamSynchronize(c->stream));
    return first_status(*c->h_total);
}

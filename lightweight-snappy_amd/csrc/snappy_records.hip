// snappy_records.hip -- record batches: `count` independent raw Snappy streams
// (records) of 0 .. 65,536 decoded bytes each, named by (offset, length) u64
// pairs relative to one base pointer, compressed or decoded in one call
// (include/snappy_amd.h).
//
// Compress:  KR0 (plan) -> K3 (scratch offsets) -> read-back -> KR1 / KR1-64
//            (k1r_body over each class's list) -> K3 (output offsets) -> KR2
// Decode:    KR4 (k4_body pass 1, one wave per record)
// Lengths:   KR5 (one thread per record)
//
// The match rounds, the emit passes and the element decode are the bodies of
// snappy_kernels.hip, entered through record entry points there; this file
// holds the plan pass, the length kernel, the launches and the C entry points.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "snappy_amd.h"
#include "snappy_ctx.h"
#include "snappy_kernels.h"

using namespace snappy_amd;

namespace {

// what the host reads back once the plan is made (48 bytes, through c->h_total)
struct PlanOut {
    uint64_t scratch_words;  // K3's total over the records' scratch needs
    uint64_t sum;            // bytes of the accepted records
    uint64_t first;          // min over refused records of record << 8 | -status (~0: none)
    uint32_t n_small, n_big, n_empty, n_refused;
    uint32_t longest;        // the longest accepted record
    uint32_t pad;
};
static_assert(sizeof(PlanOut) == 48, "read back through the context's 64 pinned bytes");

// the tables of a call in c->r_meta
struct PlanTables {
    PlanOut *out;
    uint64_t *sbase;      // count + 1: each record's scratch offset (u32 words)
    uint32_t *need;       // count: its scratch need (0: not matched)
    uint32_t *list_small; // count: the records of 1 .. 32,768 bytes (K1r), in no particular order
    uint32_t *list_big;   // count: the records of 32,769 .. 65,536 bytes (K1r64)
    int32_t *status;      // count: 0, or the refusal
};
constexpr size_t kPlanHead = 64;
size_t plan_bytes(size_t count) { return kPlanHead + (count + 1) * 8 + count * 16; }
PlanTables plan_tables(uint8_t *m, size_t count)
{
    PlanTables t;
    t.out = reinterpret_cast<PlanOut *>(m);
    t.sbase = reinterpret_cast<uint64_t *>(m + kPlanHead);
    t.need = reinterpret_cast<uint32_t *>(t.sbase + count + 1);
    t.list_small = t.need + count;
    t.list_big = t.list_small + count;
    t.status = reinterpret_cast<int32_t *>(t.list_big + count);
    return t;
}

uint32_t blocks_of(uint64_t items, uint32_t per) { return (uint32_t)((items + per - 1) / per); }

// lanes below this one in a ballot mask
__device__ __forceinline__ uint32_t rank_in(uint64_t mask, uint32_t lane)
{
    return (uint32_t)__builtin_popcountll(mask & ((1ull << lane) - 1));
}

// KR0: one thread per record.  Checks the descriptor, sets the record's class,
// its scratch need, its status word and -- for the records K1r never sees --
// its encoded size (0 refused, 1 empty: the byte 00) and token count; appends it
// to its class's list (one atomic per wave and class) and adds it to the totals.
// No byte of any record is read.
__global__ __launch_bounds__(256) void kr0_plan(const uint64_t *__restrict__ off_len, uint64_t count,
                                                uint64_t in_bytes, uint32_t *__restrict__ need,
                                                uint32_t *__restrict__ list_small, uint32_t *__restrict__ list_big,
                                                int32_t *__restrict__ status, uint32_t *__restrict__ sizes,
                                                uint32_t *__restrict__ ntok, PlanOut *__restrict__ po)
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
    if (L > SNAPPY_BLOCK) st = SNAPPY_ST_UNSUPPORTED;
    else if (off > in_bytes || L > in_bytes - off) st = -1;  // SNAPPY_AMD_ERR_ARG
    const bool ok = live && st == SNAPPY_ST_OK;
    const bool small = ok && L >= 1 && L <= SNAPPY_K1R_MAX_UNIT, big = ok && L > SNAPPY_K1R_MAX_UNIT;
    const bool empty = ok && L == 0, refused = live && !ok;
    if (live) {
        need[r] = small || big ? records_need_words((uint32_t)L) : 0u;
        status[r] = st;
        sizes[r] = empty ? 1u : 0u;  // (a matched record's: K1r writes them)
        ntok[r] = 0;
        if (refused) atomicMin(reinterpret_cast<unsigned long long *>(&po->first), (r << 8) | (uint32_t)-st);
    }
    const uint64_t ms = __ballot(small), mb = __ballot(big), me = __ballot(empty), mr = __ballot(refused);
    uint32_t bs = 0, bb = 0;
    if (lane == 0) {
        if (ms) bs = atomicAdd(&po->n_small, (uint32_t)__builtin_popcountll(ms));
        if (mb) bb = atomicAdd(&po->n_big, (uint32_t)__builtin_popcountll(mb));
        if (me) atomicAdd(&po->n_empty, (uint32_t)__builtin_popcountll(me));
        if (mr) atomicAdd(&po->n_refused, (uint32_t)__builtin_popcountll(mr));
    }
    bs = __builtin_amdgcn_readfirstlane(bs);
    bb = __builtin_amdgcn_readfirstlane(bb);
    if (small) list_small[bs + rank_in(ms, lane)] = (uint32_t)r;
    if (big) list_big[bb + rank_in(mb, lane)] = (uint32_t)r;
    // the wave's byte sum and longest record
    uint64_t sum = ok ? L : 0;
    uint32_t mx = ok ? (uint32_t)L : 0u;
    for (uint32_t d = 32; d; d >>= 1) {
        sum += __shfl_xor(sum, d);
        const uint32_t o = __shfl_xor(mx, d);
        mx = o > mx ? o : mx;
    }
    if (lane == 0 && (ms | mb)) {
        atomicAdd(reinterpret_cast<unsigned long long *>(&po->sum), sum);
        atomicMax(&po->longest, mx);
    }
}

// KR5: one thread per record reads its preamble: a 64-bit LEB128 value under the
// rules of snappy_varint_decode (at most 10 bytes, the last one without the
// continuation bit, all inside the record's range)
__global__ __launch_bounds__(256) void kr5_record_lengths(const uint8_t *__restrict__ comp, uint64_t comp_bytes,
                                                          const uint64_t *__restrict__ off_len, uint64_t count,
                                                          uint64_t *__restrict__ len, int32_t *__restrict__ status)
{
    const uint64_t r = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= count) return;
    const uint64_t off = off_len[2 * r], n = off_len[2 * r + 1];
    int32_t st = SNAPPY_ST_HEADER;
    uint64_t v = 0;
    if (off > comp_bytes || n > comp_bytes - off) {
        st = SNAPPY_ST_TRUNCATED;
    } else {
        for (uint32_t k = 0; k < 10 && k < n; k++) {
            const uint32_t b = comp[off + k];
            v |= (uint64_t)(b & 0x7F) << (7 * k);
            if (!(b & 0x80)) { st = SNAPPY_ST_OK; break; }
        }
    }
    len[r] = st == SNAPPY_ST_OK ? v : 0;
    if (status) status[r] = st;
}

int call_begin(snappy_amd_ctx *c)
{
    HIP_OK(hipSetDevice(c->device));
    if (ctx_stream(c)) return SNAPPY_AMD_ERR_DEVICE;
    (void)hipGetLastError();  // (a pending error that is not this call's, as in compress_launch)
    return SNAPPY_AMD_OK;
}

int first_status(uint64_t first) { return first == ~0ull ? SNAPPY_AMD_OK : -(int)(first & 0xFF); }

}  // namespace

extern "C" {

size_t snappy_amd_max_records_output(size_t total_bytes, size_t count)
{
    return total_bytes + total_bytes / 32 + 32 * count + 16;
}

size_t snappy_amd_max_records_scratch(size_t total_bytes, size_t count)
{
    // tokens + escapes 8 (L / 4 + 2) <= 2 L + 16, segment records 8 ceil((L / 4 + 2) / 256) <= L / 128 + 16,
    // the plan's tables 24, sizes and token counts 8 bytes a record
    const size_t need = 2 * total_bytes + total_bytes / 128 + 64 * count + 256;
    // each of the four buffers may carry grow()'s slack: an eighth and a page
    return need + need / 8 + 4 * 4096 + 128;
}

int snappy_amd_compress_records_device(snappy_amd_ctx *c, const void *d_in, size_t in_bytes,
                                       const uint64_t *d_in_off_len, size_t count, void *d_out, size_t out_cap,
                                       uint64_t *d_offsets, int32_t *d_status, size_t *out_len)
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
    if ((rc = grow(reinterpret_cast<void **>(&c->r_meta), &c->r_meta_cap, plan_bytes(count)))) return rc;
    if ((rc = grow(reinterpret_cast<void **>(&c->sizes), &c->sizes_cap, count * sizeof(uint32_t)))) return rc;
    if ((rc = grow(reinterpret_cast<void **>(&c->ntok), &c->ntok_cap, count * sizeof(uint32_t)))) return rc;
    const PlanTables t = plan_tables(c->r_meta, count);
    const uint64_t *ol = d_in_off_len;
    const uint8_t *in = static_cast<const uint8_t *>(d_in);

    // ---- the plan: classes, lists, scratch needs and their scan; one read-back
    HIP_OK(hipMemsetAsync(t.out, 0, sizeof(PlanOut), c->stream));
    HIP_OK(hipMemsetAsync(&t.out->first, 0xFF, sizeof(uint64_t), c->stream));
    hipLaunchKernelGGL(kr0_plan, dim3(blocks_of(count, 256)), dim3(256), 0, c->stream, ol, (uint64_t)count,
                       (uint64_t)in_bytes, t.need, t.list_small, t.list_big, t.status, c->sizes, c->ntok, t.out);
    if (count <= SNAPPY_K3_WAVE_MAX)
        hipLaunchKernelGGL(k3_scan_wave, dim3(1), dim3(64), 0, c->stream, t.need, (uint64_t)count, t.sbase,
                           &t.out->scratch_words);
    else
        hipLaunchKernelGGL(k3_scan, dim3(1), dim3(1024), 0, c->stream, t.need, (uint64_t)count, t.sbase,
                           &t.out->scratch_words);
    HIP_OK(hipGetLastError());
    PlanOut *const po = reinterpret_cast<PlanOut *>(c->h_total);
    HIP_OK(hipMemcpyAsync(po, t.out, sizeof(PlanOut), hipMemcpyDeviceToHost, c->stream));
    HIP_OK(hipStreamSynchronize(c->stream));
    const PlanOut p = *po;
    if (out_cap < snappy_amd_max_records_output((size_t)p.sum, count)) return SNAPPY_AMD_ERR_CAPACITY;
    // (+ 64: K2 lanes with no literal read 20 bytes at their record's first token words)
    if ((rc = grow(reinterpret_cast<void **>(&c->tokens), &c->tokens_cap, p.scratch_words * sizeof(uint32_t) + 64)))
        return rc;
    uint32_t *scratch = static_cast<uint32_t *>(c->tokens);

    // ---- each match kernel over its own class, the output offsets, the emit
    if (p.n_small)
        hipLaunchKernelGGL(kr1_match_records, dim3(p.n_small), dim3(64), 0, c->stream, in, ol, t.list_small, t.sbase,
                           scratch, c->ntok, c->sizes);
    if (p.n_big)
        hipLaunchKernelGGL(kr1_match_records64, dim3(p.n_big), dim3(64), 0, c->stream, in, ol, t.list_big, t.sbase,
                           scratch, c->ntok, c->sizes);
    HIP_OK(hipGetLastError());
    if (count <= SNAPPY_K3_WAVE_MAX)
        hipLaunchKernelGGL(k3_scan_wave, dim3(1), dim3(64), 0, c->stream, c->sizes, (uint64_t)count, d_offsets, c->total);
    else
        hipLaunchKernelGGL(k3_scan, dim3(1), dim3(1024), 0, c->stream, c->sizes, (uint64_t)count, d_offsets, c->total);
    if (p.n_small + p.n_big + p.n_empty) {
        // no more waves per record than the longest record has segments
        const uint32_t segs = records_segs(p.longest);
        hipLaunchKernelGGL(kr2_emit_records, dim3((uint32_t)count, segs < SNAPPY_K2_WAVES ? segs : SNAPPY_K2_WAVES),
                           dim3(64), 0, c->stream, in, ol, t.status, t.sbase, scratch, c->ntok, d_offsets,
                           static_cast<uint8_t *>(d_out));
    }
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

int snappy_amd_records_length_device(snappy_amd_ctx *c, const void *d_comp, size_t comp_bytes,
                                     const uint64_t *d_comp_off_len, size_t count, uint64_t *d_len, int32_t *d_status)
{
    if (!c || (!d_comp && comp_bytes) || (count && (!d_comp_off_len || !d_len))) return SNAPPY_AMD_ERR_ARG;
    if (count > 0x7FFFFFFFull) return SNAPPY_AMD_ERR_ARG;
    if (count == 0) return SNAPPY_AMD_OK;
    int rc = call_begin(c);
    if (rc) return rc;
    hipLaunchKernelGGL(kr5_record_lengths, dim3(blocks_of(count, 256)), dim3(256), 0, c->stream,
                       static_cast<const uint8_t *>(d_comp), (uint64_t)comp_bytes, d_comp_off_len, (uint64_t)count, d_len,
                       d_status);
    HIP_OK(hipGetLastError());
    return SNAPPY_AMD_OK;
}

int snappy_amd_decompress_records_device(snappy_amd_ctx *c, const void *d_comp, size_t comp_bytes,
                                         const uint64_t *d_comp_off_len, size_t count, void *d_out, size_t out_bytes,
                                         const uint64_t *d_out_off_len, int32_t *d_status, int sync)
{
    if (!c || (!d_comp && comp_bytes) || (!d_out && out_bytes) || (count && (!d_comp_off_len || !d_out_off_len)))
        return SNAPPY_AMD_ERR_ARG;
    if (count > 0x7FFFFFFFull) return SNAPPY_AMD_ERR_ARG;
    if (count == 0) return SNAPPY_AMD_OK;
    int rc = call_begin(c);
    if (rc) return rc;
    // the first-failure word, and the status words of a caller that passes none
    if ((rc = grow(reinterpret_cast<void **>(&c->r_meta), &c->r_meta_cap, kPlanHead + count * sizeof(int32_t))))
        return rc;
    unsigned long long *first = reinterpret_cast<unsigned long long *>(c->r_meta);
    int32_t *status = d_status ? d_status : reinterpret_cast<int32_t *>(c->r_meta + kPlanHead);
    HIP_OK(hipMemsetAsync(first, 0xFF, sizeof(uint64_t), c->stream));
    // the kernel reads aligned dwords: pass the base as an aligned pointer + bias
    const uint32_t bias = (uint32_t)(reinterpret_cast<uintptr_t>(d_comp) & 3);
    const uint8_t *comp = static_cast<const uint8_t *>(d_comp) - bias;
    hipLaunchKernelGGL(kr4_decode_records, dim3((uint32_t)count), dim3(64), 0, c->stream, comp, bias,
                       (uint64_t)comp_bytes, d_comp_off_len, static_cast<uint8_t *>(d_out), (uint64_t)out_bytes,
                       d_out_off_len, status, first);
    HIP_OK(hipGetLastError());
    if (!sync) return SNAPPY_AMD_OK;
    HIP_OK(hipMemcpyAsync(c->h_total, first, sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
    HIP_OK(hipStreamSynchronize(c->stream));
    return first_status(*c->h_total);
}

}  // extern "C"

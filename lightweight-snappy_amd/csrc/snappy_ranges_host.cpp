// snappy_ranges_host.cpp -- range decode over host memory and FILE* (DESIGN.md
// 7.6): bytes [start, start + length) of what snappy_decompress_buffer returns.
// With a sidecar index only the preamble and the compressed window of the blocks
// the range touches are read from the source and uploaded; without one the whole
// stream is uploaded and indexed on the GPU.  A range that is not self-contained
// (foreign streams only) and every failure are settled by the whole-stream
// decoders of snappy_pipeline.cpp, so the statuses are theirs.
#include <hip/hip_runtime_api.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <sys/types.h>

#include <vector>

#include "snappy_amd.h"
#include "snappy_amd_internal.h"
#include "snappy_ctx.h"

namespace {

constexpr uint64_t kOffMask = (1ull << SNAPPY_AMD_IDX_OFFSET_BITS) - 1;

// a compressed stream the host can read at any position
struct Source {
    uint64_t clen = 0;
    const uint8_t *mem = nullptr;  // host memory, or
    FILE *file = nullptr;          // a seekable file whose stream starts at `base`
    off_t base = 0;
    int read(uint64_t off, size_t len, uint8_t *dst) const
    {
        if (off > clen || len > clen - off) return SNAPPY_AMD_ERR_IO;
        if (mem) {
            memcpy(dst, mem + off, len);
            return SNAPPY_AMD_OK;
        }
        if (fseeko(file, base + (off_t)off, SEEK_SET) != 0) return SNAPPY_AMD_ERR_IO;
        return fread(dst, 1, len, file) == len ? SNAPPY_AMD_OK : SNAPPY_AMD_ERR_IO;
    }
};

struct LeaseGuard {
    void *token = nullptr;
    ~LeaseGuard() { if (token) host_ctx_return(token); }
};

// the whole-stream decode, sliced: the fallback of a range that is not
// self-contained and the judge of every failure (with a sidecar: index_fits, the
// decode and sidecar_verdict, as snappy_decompress_file_indexed)
int whole_slice(const Source &src, const uint64_t *idx, size_t count, uint64_t N, uint64_t start, size_t length,
                uint8_t *out)
{
    std::vector<uint8_t> in((size_t)src.clen), full((size_t)(N ? N : 1));
    int rc = src.read(0, (size_t)src.clen, in.data());
    if (rc) return rc;
    size_t len = 0;
    rc = idx ? snappy_amd_host_decompress_idx(in.data(), in.size(), idx, count, full.data(), (size_t)N, &len)
             : snappy_amd_host_decompress(in.data(), in.size(), full.data(), (size_t)N, &len);
    if (rc) return rc;
    if (start > len || length > len - start) return SNAPPY_AMD_ERR_ARG;
    memcpy(out, full.data() + start, length);
    return SNAPPY_AMD_OK;
}

// the sidecar file's bytes -> N and its entries (the checks of the FILE* reader)
int parse_sidecar(const uint8_t *b, size_t bytes, uint64_t *N, std::vector<uint64_t> *ent)
{
    uint64_t h[3];
    if (bytes < sizeof h) return SNAPPY_AMD_ERR_INDEX;
    memcpy(h, b, sizeof h);
    if (h[0] != SNAPPY_AMD_IDX_MAGIC || h[2] > (h[1] >> 16) + 2) return SNAPPY_AMD_ERR_INDEX;
    if ((bytes - sizeof h) / sizeof(uint64_t) != h[2] || (bytes - sizeof h) % sizeof(uint64_t)) return SNAPPY_AMD_ERR_INDEX;
    ent->resize((size_t)h[2]);
    if (h[2]) memcpy(ent->data(), b + sizeof h, (size_t)h[2] * sizeof(uint64_t));
    *N = h[1];
    return SNAPPY_AMD_OK;
}

// out[0, length) = decoded bytes [start, start + length)
int range_core(const Source &src, const uint8_t *sidecar, size_t sidecar_bytes, uint64_t start, uint64_t length,
               uint8_t *out)
{
    if (src.clen == 0) return start == 0 && length == 0 ? SNAPPY_AMD_OK : SNAPPY_AMD_ERR_ARG;
    uint8_t head[10];
    const size_t hn = src.clen < sizeof head ? (size_t)src.clen : sizeof head;
    int rc = src.read(0, hn, head);
    if (rc) return rc;
    uint64_t N = 0;
    const bool have_n = snappy_varint_decode(head, hn, &N) != 0;
    std::vector<uint64_t> ent;
    if (sidecar) {
        uint64_t sN = 0;
        if ((rc = parse_sidecar(sidecar, sidecar_bytes, &sN, &ent))) return rc;
        const uint64_t units = (sN + SNAPPY_AMD_BLOCK - 1) / SNAPPY_AMD_BLOCK;
        if (!have_n || N != sN || ent.size() != units + 1 || (ent[units] & kOffMask) != src.clen)
            return SNAPPY_AMD_ERR_INDEX;
        for (uint64_t i = 0; i < units; i++)
            if ((ent[i] & kOffMask) > (ent[i + 1] & kOffMask)) return SNAPPY_AMD_ERR_INDEX;
    } else if (!have_n) {
        return SNAPPY_AMD_ERR_HEADER;
    }
    if (start > N || length > N - start) return SNAPPY_AMD_ERR_ARG;
    if (length == 0) return SNAPPY_AMD_OK;
    const uint64_t units = (N + SNAPPY_AMD_BLOCK - 1) / SNAPPY_AMD_BLOCK;
    const uint64_t u0 = start / SNAPPY_AMD_BLOCK, u1 = (start + length - 1) / SNAPPY_AMD_BLOCK;
    const uint64_t *idx = sidecar ? ent.data() : nullptr;

    LeaseGuard lease;
    snappy_amd_ctx *c = nullptr;
    if ((rc = host_ctx_lease(&lease.token, &c))) return rc;
    std::vector<uint8_t> win;
    uint64_t w0 = 0, w1 = src.clen;
    bool contained = true;
    if ((rc = grow(reinterpret_cast<void **>(&c->d_idx), &c->d_idx_cap, (size_t)(units + 2) * sizeof(uint64_t))))
        return rc;
    if (idx) {
        // skip bits on the range's first entry or after its last block: elements straddle
        // the window's edges (a foreign stream)
        contained = !(ent[u0] >> SNAPPY_AMD_IDX_OFFSET_BITS) && !(ent[u1 + 1] >> SNAPPY_AMD_IDX_OFFSET_BITS);
        w0 = ent[u0] & kOffMask;
        w1 = ent[u1 + 1] & kOffMask;
    }
    if (contained) {
        win.resize((size_t)(w1 - w0));
        if ((rc = src.read(w0, win.size(), win.data()))) return rc;
        // the window at the address residue its first byte has in the stream, so the
        // kernels' aligned loads see it as the whole-stream decode would
        const size_t pad = (size_t)(w0 & 3);
        if ((rc = grow(reinterpret_cast<void **>(&c->d_a), &c->d_a_cap, win.size() + pad + 16))) return rc;
        HIP_OK(hipMemcpyAsync(c->d_a + pad, win.data(), win.size(), hipMemcpyHostToDevice, c->stream));
        if (idx) {
            HIP_OK(hipMemcpyAsync(c->d_idx, idx, ent.size() * sizeof(uint64_t), hipMemcpyHostToDevice, c->stream));
        } else {
            size_t got = 0;
            if ((rc = snappy_amd_index_device(c, c->d_a, win.size(), c->d_idx, (size_t)units + 1, &got))) return rc;
            uint64_t e[2];
            HIP_OK(hipMemcpy(&e[0], c->d_idx + u0, sizeof(uint64_t), hipMemcpyDeviceToHost));
            HIP_OK(hipMemcpy(&e[1], c->d_idx + u1 + 1, sizeof(uint64_t), hipMemcpyDeviceToHost));
            contained = !(e[0] >> SNAPPY_AMD_IDX_OFFSET_BITS) && !(e[1] >> SNAPPY_AMD_IDX_OFFSET_BITS);
        }
    }
    if (contained) {
        const size_t oo = (size_t)(start & 15);  // 16-byte stores: the output as aligned as the range
        if ((rc = grow(reinterpret_cast<void **>(&c->d_b), &c->d_b_cap, (size_t)length + oo + 16))) return rc;
        const snappy_amd_range r = {start, length, oo};
        rc = snappy_amd_decompress_ranges_device(c, c->d_a + (w0 & 3), w0, win.size(), c->d_idx, (size_t)N,
                                                 SNAPPY_AMD_BLOCK, SNAPPY_AMD_SINGLE, &r, 1, c->d_b,
                                                 (size_t)length + oo, nullptr, 1);
        if (rc == SNAPPY_AMD_OK) {
            HIP_OK(hipMemcpyAsync(out, c->d_b + oo, (size_t)length, hipMemcpyDeviceToHost, c->stream));
            HIP_OK(hipStreamSynchronize(c->stream));
            return SNAPPY_AMD_OK;
        }
        if (rc == SNAPPY_AMD_ERR_DEVICE) return rc;
        // ERR_DEPENDENT: the stream is decoded whole; any other failure is reported as
        // the whole decode reports it
    }
    HIP_OK(hipStreamSynchronize(c->stream));
    // (the whole-stream decoders lease their own context: give this one back first)
    host_ctx_return(lease.token);
    lease.token = nullptr;
    return whole_slice(src, idx, ent.size(), N, start, (size_t)length, out);
}

}  // namespace

extern "C" {

int snappy_decompress_range_buffer(const uint8_t *in, size_t n, const uint8_t *idx, size_t idx_bytes, uint64_t start,
                                   size_t length, uint8_t *out, size_t cap, size_t *out_len)
{
    if (!out_len || (n && !in) || (length && !out)) return SNAPPY_AMD_ERR_ARG;
    *out_len = 0;
    if (length > cap) return SNAPPY_AMD_ERR_CAPACITY;
    Source src;
    src.clen = n;
    src.mem = in;
    const int rc = range_core(src, idx, idx_bytes, start, length, out);
    if (rc == SNAPPY_AMD_OK) *out_len = length;
    return rc;
}

int snappy_decompress_file_range(FILE *file_input, FILE *idx, uint64_t start, uint64_t length, FILE *file_out)
{
    if (!file_input || !file_out) return SNAPPY_AMD_ERR_ARG;
    Source src;
    src.file = file_input;
    src.base = ftello(file_input);
    if (src.base < 0 || fseeko(file_input, 0, SEEK_END) != 0) return SNAPPY_AMD_ERR_UNSUPPORTED;
    const off_t end = ftello(file_input);
    if (end < src.base) return SNAPPY_AMD_ERR_UNSUPPORTED;
    src.clen = (uint64_t)(end - src.base);
    std::vector<uint8_t> side;
    if (idx) {
        uint8_t buf[65536];
        size_t got;
        while ((got = fread(buf, 1, sizeof buf, idx)) > 0) side.insert(side.end(), buf, buf + got);
        if (ferror(idx)) return SNAPPY_AMD_ERR_IO;
        if (side.empty()) return SNAPPY_AMD_ERR_INDEX;
    }
    // (a length no stream of this size can hold is refused before it is allocated)
    if (length / 22 > src.clen) return SNAPPY_AMD_ERR_ARG;
    std::vector<uint8_t> out((size_t)(length ? length : 1));
    const int rc = range_core(src, idx ? side.data() : nullptr, side.size(), start, length, out.data());
    if (rc) return rc;
    if (length && fwrite(out.data(), 1, (size_t)length, file_out) != length) return SNAPPY_AMD_ERR_IO;
    return SNAPPY_AMD_OK;
}

}  // extern "C"

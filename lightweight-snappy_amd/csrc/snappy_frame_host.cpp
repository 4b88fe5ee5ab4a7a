// snappy_frame_host.cpp -- the Snappy framing format over host memory and
// FILE*: host C++ on the device API of snappy_frame.hip, with the pooled host
// contexts of snappy_pipeline.cpp (host_ctx_lease).  No kernel is launched
// here.
//
// The chunk headers are walked on the host: the stream is in host memory, so
// the walk costs nothing beside the H2D copy, and its chunk table is uploaded
// in place of the device walk (KF3).  Both follow snappy_frame_chunk
// (snappy_frame.h).  The FILE* forms are plain loops over the buffer forms,
// one piece (64 MiB) at a time.  Declared in include/snappy_amd.h.
#include <hip/hip_runtime_api.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

#include "snappy_amd.h"
#include "snappy_ctx.h"
#include "snappy_frame.h"

namespace {
// Bytes a call handles at a time: a multiple of the 65,536-byte chunk, so the
// chunks of a piece are those of the whole input.  SNAPPY_AMD_FRAME_PIECE_KB
// (a multiple of 64, read at every call) sets another size: the tests use it
// to cross piece boundaries with small inputs.
size_t piece_bytes()
{
    const char *e = getenv("SNAPPY_AMD_FRAME_PIECE_KB");
    const long kb = e ? atol(e) : 0;
    if (kb >= 64 && kb % 64 == 0 && kb <= (4l << 20)) return (size_t)kb << 10;
    return (size_t)64 << 20;
}

class HostLease {
public:
    HostLease() { rc_ = host_ctx_lease(&token_, &c_); }
    ~HostLease() { if (token_) host_ctx_return(token_); }
    HostLease(const HostLease &) = delete;
    HostLease &operator=(const HostLease &) = delete;
    int rc() const { return rc_; }
    snappy_amd_ctx *ctx() const { return c_; }

private:
    void *token_ = nullptr;
    snappy_amd_ctx *c_ = nullptr;
    int rc_ = SNAPPY_AMD_OK;
};

size_t read_full(FILE *f, uint8_t *b, size_t cap)
{
    size_t n = 0;
    while (n < cap) {
        const size_t got = fread(b + n, 1, cap - n, f);
        if (got == 0) break;
        n += got;
    }
    return n;
}

// Walk in[0..n).  *total = decoded bytes of the whole chunks; *stop = where the
// walk ended: n, or the chunk that failed (every chunk before it is whole, so
// a reader with more bytes coming cuts there on SNAPPY_AMD_ERR_TRUNCATED);
// *chunks (when given) = the chunk table of in[0..*stop): the data chunks'
// positions, then *stop.
int frame_walk_host(const uint8_t *in, size_t n, bool need_ident, std::vector<uint64_t> *chunks, uint64_t *total,
                    size_t *stop)
{
    size_t pos = 0;
    uint64_t sum = 0;
    int first = need_ident, rc = SNAPPY_AMD_OK;
    while (pos < n) {
        uint8_t w[SNAPPY_FRAME_WINDOW] = {};
        const size_t avail = n - pos;
        memcpy(w, in + pos, avail < sizeof(w) ? avail : sizeof(w));
        uint32_t dlen;
        uint64_t adv;
        const int r = snappy_frame_chunk(w, avail, first, &dlen, &adv);
        if (r < 0) {
            rc = r;
            break;
        }
        first = 0;
        if (r == 1) {
            if (chunks) chunks->push_back(pos);
            sum += dlen;
        }
        pos += (size_t)adv;
    }
    if (chunks) chunks->push_back(pos);
    if (total) *total = sum;
    if (stop) *stop = pos;
    return rc;
}

// frame in[0..n) (at most one piece) on context c, *len bytes to out
int frame_compress_piece(snappy_amd_ctx *c, const uint8_t *in, size_t n, uint32_t flags, uint8_t *out, size_t cap,
                         size_t *len)
{
    const size_t units = (n + SNAPPY_AMD_BLOCK - 1) / SNAPPY_AMD_BLOCK;
    int rc;
    if ((rc = grow(reinterpret_cast<void **>(&c->d_a), &c->d_a_cap, n + 16))) return rc;
    if ((rc = grow(reinterpret_cast<void **>(&c->d_b), &c->d_b_cap, snappy_amd_max_frame_output(n)))) return rc;
    if ((rc = grow(reinterpret_cast<void **>(&c->d_idx), &c->d_idx_cap, (units + 1) * sizeof(uint64_t)))) return rc;
    if (n) HIP_OK(hipMemcpyAsync(c->d_a, in, n, hipMemcpyHostToDevice, c->stream));
    if ((rc = snappy_amd_compress_frame_device(c, c->d_a, n, flags, c->d_b, c->d_idx, len))) return rc;
    if (*len > cap) return SNAPPY_AMD_ERR_CAPACITY;
    if (*len) HIP_OK(hipMemcpyAsync(out, c->d_b, *len, hipMemcpyDeviceToHost, c->stream));
    HIP_OK(hipStreamSynchronize(c->stream));
    return SNAPPY_AMD_OK;
}

// decode the data chunks of in[0..n) that a walk found (chunks: its table,
// total: their decoded bytes, <= the room at out) on context c
int frame_decode_piece(snappy_amd_ctx *c, const uint8_t *in, size_t n, const std::vector<uint64_t> &chunks,
                       uint64_t total, uint8_t *out, size_t *out_len)
{
    *out_len = 0;
    const size_t nchunks = chunks.size() - 1;
    if (nchunks == 0) return SNAPPY_AMD_OK;
    int rc;
    if ((rc = grow(reinterpret_cast<void **>(&c->d_a), &c->d_a_cap, n + 16))) return rc;
    if ((rc = grow(reinterpret_cast<void **>(&c->d_b), &c->d_b_cap, total + 16))) return rc;
    if ((rc = grow(reinterpret_cast<void **>(&c->d_idx), &c->d_idx_cap, chunks.size() * sizeof(uint64_t)))) return rc;
    HIP_OK(hipMemcpyAsync(c->d_a, in, n, hipMemcpyHostToDevice, c->stream));
    HIP_OK(hipMemcpyAsync(c->d_idx, chunks.data(), chunks.size() * sizeof(uint64_t), hipMemcpyHostToDevice, c->stream));
    size_t got = 0;
    if ((rc = snappy_amd_decompress_frame_device(c, c->d_a, n, c->d_idx, nchunks, c->d_b, (size_t)total, &got))) return rc;
    if (got) HIP_OK(hipMemcpyAsync(out, c->d_b, got, hipMemcpyDeviceToHost, c->stream));
    HIP_OK(hipStreamSynchronize(c->stream));
    *out_len = got;
    return SNAPPY_AMD_OK;
}
}  // namespace

extern "C" {

int snappy_frame_uncompressed_length(const uint8_t *in, size_t n, uint64_t *len)
{
    if (!len || (!in && n)) return SNAPPY_AMD_ERR_ARG;
    return frame_walk_host(in, n, true, nullptr, len, nullptr);
}

int snappy_compress_frame_buffer(const uint8_t *in, size_t n, uint8_t *out, size_t cap, size_t *out_len)
{
    if (!out_len || (!in && n) || !out) return SNAPPY_AMD_ERR_ARG;
    *out_len = 0;
    HostLease h;
    if (h.rc()) return h.rc();
    // chunk sequences concatenate: every piece after the first without the identifier
    const size_t kPiece = piece_bytes();
    size_t at = 0, done = 0;
    do {
        const size_t piece = n - done < kPiece ? n - done : kPiece;
        size_t len = 0;
        int rc = frame_compress_piece(h.ctx(), in + done, piece, done ? SNAPPY_AMD_FRAME_NO_IDENTIFIER : 0u, out + at,
                                      cap - at, &len);
        if (rc) return rc;
        at += len;
        done += piece;
    } while (done < n);
    *out_len = at;
    return SNAPPY_AMD_OK;
}

int snappy_decompress_frame_buffer(const uint8_t *in, size_t n, uint8_t *out, size_t cap, size_t *out_len)
{
    if (!out_len || (!in && n) || (!out && cap)) return SNAPPY_AMD_ERR_ARG;
    *out_len = 0;
    // malformed streams, short buffers and streams without a data chunk end here, before any device call
    std::vector<uint64_t> chunks;
    uint64_t total = 0;
    int rc = frame_walk_host(in, n, true, &chunks, &total, nullptr);
    if (rc) return rc;
    if (total > cap) return SNAPPY_AMD_ERR_CAPACITY;
    if (chunks.size() == 1) return SNAPPY_AMD_OK;
    HostLease h;
    if (h.rc()) return h.rc();
    return frame_decode_piece(h.ctx(), in, n, chunks, total, out, out_len);
}

int snappy_compress_file_framed(FILE *fin, unsigned long long input_size, FILE *fout)
{
    (void)input_size;
    if (!fin || !fout) return SNAPPY_AMD_ERR_ARG;
    HostLease h;
    if (h.rc()) return h.rc();
    const size_t kPiece = piece_bytes();
    std::vector<uint8_t> in(kPiece), out(snappy_amd_max_frame_output(kPiece));
    bool first = true;
    for (;;) {
        const size_t n = read_full(fin, in.data(), in.size());
        if (ferror(fin)) return SNAPPY_AMD_ERR_IO;
        if (n == 0 && !first) break;
        size_t len = 0;
        int rc = frame_compress_piece(h.ctx(), in.data(), n, first ? 0u : SNAPPY_AMD_FRAME_NO_IDENTIFIER, out.data(),
                                      out.size(), &len);
        if (rc) return rc;
        if (len && fwrite(out.data(), 1, len, fout) != len) return SNAPPY_AMD_ERR_IO;
        first = false;
        if (n < in.size()) break;
    }
    return fflush(fout) ? SNAPPY_AMD_ERR_IO : SNAPPY_AMD_OK;
}

int snappy_decompress_file_framed(FILE *fin, FILE *fout)
{
    if (!fin || !fout) return SNAPPY_AMD_ERR_ARG;
    HostLease h;
    if (h.rc()) return h.rc();
    std::vector<uint8_t> in(piece_bytes()), out;
    std::vector<uint64_t> chunks;
    size_t have = 0;
    bool first = true, eof = false;
    while (!eof) {
        have += read_full(fin, in.data() + have, in.size() - have);
        if (ferror(fin)) return SNAPPY_AMD_ERR_IO;
        eof = have < in.size();
        uint64_t total = 0;
        size_t stop = 0;
        chunks.clear();
        int rc = frame_walk_host(in.data(), have, first, &chunks, &total, &stop);
        if (rc == SNAPPY_AMD_ERR_TRUNCATED && !eof) {
            // the rest comes with the next read: decode the whole chunks now; a
            // chunk larger than the buffer (up to 4 + 2^24 - 1 bytes) needs a larger one
            if (stop == 0) {
                in.resize(in.size() * 2);
                continue;
            }
            rc = SNAPPY_AMD_OK;
        }
        if (rc) return rc;
        if (out.size() < total) out.resize((size_t)total);
        size_t len = 0;
        if ((rc = frame_decode_piece(h.ctx(), in.data(), stop, chunks, total, out.data(), &len))) return rc;
        if (len && fwrite(out.data(), 1, len, fout) != len) return SNAPPY_AMD_ERR_IO;
        memmove(in.data(), in.data() + stop, have - stop);
        have -= stop;
        first = false;
    }
    return fflush(fout) ? SNAPPY_AMD_ERR_IO : SNAPPY_AMD_OK;
}

}  // extern "C"

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
#include <sys/types.h>
#include <unistd.h>
#include <new>
#include <stdexcept>
#include <vector>

#include "snappy_amd.h"
#include "snappy_ctx.h"
#include "snappy_frame.h"
#include "snappy_frame_ranges.h"

namespace {
// Bytes a call handles at a time.  SNAPPY_AMD_FRAME_PIECE_KB (a multiple of 64,
// read at every call) sets another size: the tests use it to cross piece
// boundaries with small inputs.  The compressors cut pieces of compress_piece_bytes:
// a multiple of the chunk size, so the chunks of a piece are those of the whole input.
size_t piece_bytes()
{
    const char *e = getenv("SNAPPY_AMD_FRAME_PIECE_KB");
    const long kb = e ? atol(e) : 0;
    if (kb >= 64 && kb % 64 == 0 && kb <= (4l << 20)) return (size_t)kb << 10;
    return (size_t)64 << 20;
}

// the piece size rounded down to a multiple of `chunk` (1..65,536 <= a piece): at least one chunk
size_t compress_piece_bytes(uint32_t chunk) { return piece_bytes() / chunk * chunk; }

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
// *starts (when given) = the seek table beside it: each data chunk's decoded
// position, then the decoded bytes.
int frame_walk_host(const uint8_t *in, size_t n, bool need_ident, std::vector<uint64_t> *chunks, uint64_t *total,
                    size_t *stop, std::vector<uint64_t> *starts = nullptr)
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
            if (starts) starts->push_back(sum);
            sum += dlen;
        }
        pos += (size_t)adv;
    }
    if (chunks) chunks->push_back(pos);
    if (starts) starts->push_back(sum);
    if (total) *total = sum;
    if (stop) *stop = pos;
    return rc;
}

// frame in[0..n) (at most one piece) in chunks of `chunk` bytes on context c, *len bytes to out
int frame_compress_piece(snappy_amd_ctx *c, const uint8_t *in, size_t n, uint32_t chunk, uint32_t flags, uint8_t *out,
                         size_t cap, size_t *len)
{
    const size_t units = (n + chunk - 1) / chunk;
    int rc;
    if ((rc = grow(reinterpret_cast<void **>(&c->d_a), &c->d_a_cap, n + 16))) return rc;
    if ((rc = grow(reinterpret_cast<void **>(&c->d_b), &c->d_b_cap, snappy_amd_max_frame_output_ex(n, chunk)))) return rc;
    if ((rc = grow(reinterpret_cast<void **>(&c->d_idx), &c->d_idx_cap, (units + 1) * sizeof(uint64_t)))) return rc;
    if (n) HIP_OK(hipMemcpyAsync(c->d_a, in, n, hipMemcpyHostToDevice, c->stream));
    if ((rc = snappy_amd_compress_frame_device_ex(c, c->d_a, n, chunk, flags, c->d_b, c->d_idx, len))) return rc;
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

// ---- range decode ------------------------------------------
// a framed stream the host can read at any position: host memory, or a file
// descriptor whose stream starts at `base` (positional reads: the FILE*'s own
// position and buffer are not touched by the walk)
struct FrameSource {
    uint64_t clen = 0;
    const uint8_t *mem = nullptr;
    int fd = -1;
    off_t base = 0;
    // w = the 16 bytes at pos, zero past the stream's end
    int head(uint64_t pos, uint8_t *w) const
    {
        memset(w, 0, SNAPPY_FRAME_WINDOW);
        const uint64_t avail = clen - pos;
        const size_t want = avail < SNAPPY_FRAME_WINDOW ? (size_t)avail : SNAPPY_FRAME_WINDOW;
        if (mem) {
            memcpy(w, mem + pos, want);
            return SNAPPY_AMD_OK;
        }
        size_t got = 0;
        while (got < want) {
            const ssize_t k = pread(fd, w + got, want - got, base + (off_t)(pos + got));
            if (k <= 0) return SNAPPY_AMD_ERR_IO;
            got += (size_t)k;
        }
        return SNAPPY_AMD_OK;
    }
};

// Hop from header to header until `target` decoded bytes are covered (the chunk
// holding byte target - 1 is the last one looked at) or the stream ends; no
// payload is read.  chunks / starts = the tables of the data chunks seen, closed
// by the position after the last chunk looked at; ends[i] = where data chunk i ends.
int frame_walk_to(const FrameSource &src, uint64_t target, std::vector<uint64_t> *chunks, std::vector<uint64_t> *starts,
                  std::vector<uint64_t> *ends)
{
    uint64_t pos = 0, sum = 0;
    int first = 1;
    while (pos < src.clen) {
        uint8_t w[SNAPPY_FRAME_WINDOW];
        int rc = src.head(pos, w);
        if (rc) return rc;
        uint32_t dlen;
        uint64_t adv;
        const int r = snappy_frame_chunk(w, src.clen - pos, first, &dlen, &adv);
        if (r < 0) return r;
        first = 0;
        if (r == 1) {
            chunks->push_back(pos);
            starts->push_back(sum);
            ends->push_back(pos + adv);
            sum += dlen;
        }
        pos += adv;
        if (sum >= target) break;
    }
    chunks->push_back(pos);
    starts->push_back(sum);
    return SNAPPY_AMD_OK;
}

// out[0, length) = decoded bytes [start, start + length) of the stream; with `own`
// the output is own's, sized only once the walk has shown that the range exists.
// An allocation that fails is SNAPPY_AMD_ERR_DEVICE, as in the other host forms.
int frame_range_walked(const FrameSource &src, FILE *file, uint64_t start, uint64_t length, uint8_t *out,
                       std::vector<uint8_t> *own);
int frame_range_core(const FrameSource &src, FILE *file, uint64_t start, uint64_t length, uint8_t *out,
                     std::vector<uint8_t> *own = nullptr)
{
    try {
        return frame_range_walked(src, file, start, length, out, own);
    } catch (const std::bad_alloc &) {
        return SNAPPY_AMD_ERR_DEVICE;
    } catch (const std::length_error &) {
        return SNAPPY_AMD_ERR_DEVICE;
    }
}

int frame_range_walked(const FrameSource &src, FILE *file, uint64_t start, uint64_t length, uint8_t *out,
                       std::vector<uint8_t> *own)
{
    if (start + length < start) return SNAPPY_AMD_ERR_ARG;
    std::vector<uint64_t> chunks, starts, ends;
    int rc = frame_walk_to(src, start + length, &chunks, &starts, &ends);
    if (rc) return rc;
    const uint64_t nchunks = ends.size();
    const snappy_amd_range whole = {start, length, 0};
    uint64_t u0, u1, k;
    // (a walk that began at the identifier: starts[0] = 0, so ERR_ARG is a range past the decoded bytes)
    if ((rc = snappy_frame_span(starts.data(), nchunks, whole, length, &u0, &u1, &k))) return rc;
    if (k == 0) return SNAPPY_AMD_OK;
    if (own) {
        own->resize((size_t)length);
        out = own->data();
    }
    const uint64_t w0 = chunks[u0], w1 = ends[u1];
    std::vector<uint8_t> win((size_t)(w1 - w0));
    if (src.mem) {
        memcpy(win.data(), src.mem + w0, win.size());
    } else {
        if (fseeko(file, src.base + (off_t)w0, SEEK_SET) != 0) return SNAPPY_AMD_ERR_IO;
        if (fread(win.data(), 1, win.size(), file) != win.size()) return SNAPPY_AMD_ERR_IO;
    }
    HostLease h;
    if (h.rc()) return h.rc();
    snappy_amd_ctx *c = h.ctx();
    // the window at the address residue its first byte has in the stream; the sub-tables
    // of chunks u0 .. u1 + 1, positions and starts absolute; the output as aligned as the range
    const size_t pad = (size_t)(w0 & 3), oo = (size_t)(start & 15), ent = (size_t)k + 1;
    if ((rc = grow(reinterpret_cast<void **>(&c->d_a), &c->d_a_cap, win.size() + pad + 16))) return rc;
    if ((rc = grow(reinterpret_cast<void **>(&c->d_b), &c->d_b_cap, (size_t)length + oo + 16))) return rc;
    if ((rc = grow(reinterpret_cast<void **>(&c->d_idx), &c->d_idx_cap, 2 * ent * sizeof(uint64_t)))) return rc;
    HIP_OK(hipMemcpyAsync(c->d_a + pad, win.data(), win.size(), hipMemcpyHostToDevice, c->stream));
    HIP_OK(hipMemcpyAsync(c->d_idx, chunks.data() + u0, ent * sizeof(uint64_t), hipMemcpyHostToDevice, c->stream));
    HIP_OK(hipMemcpyAsync(c->d_idx + ent, starts.data() + u0, ent * sizeof(uint64_t), hipMemcpyHostToDevice, c->stream));
    const snappy_amd_range r = {start, length, oo};
    if ((rc = snappy_amd_decompress_frame_ranges_device(c, c->d_a + pad, w0, win.size(), c->d_idx, c->d_idx + ent,
                                                        (size_t)k, &r, 1, c->d_b, (size_t)length + oo, nullptr)))
        return rc;
    HIP_OK(hipMemcpyAsync(out, c->d_b + oo, (size_t)length, hipMemcpyDeviceToHost, c->stream));
    HIP_OK(hipStreamSynchronize(c->stream));
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
    return snappy_compress_frame_buffer_ex(in, n, SNAPPY_AMD_BLOCK, 0u, out, cap, out_len);
}

int snappy_compress_frame_buffer_ex(const uint8_t *in, size_t n, uint32_t chunk, uint32_t flags, uint8_t *out,
                                    size_t cap, size_t *out_len)
{
    if (!out_len || (!in && n) || !out) return SNAPPY_AMD_ERR_ARG;
    *out_len = 0;
    if (chunk == 0 || chunk > SNAPPY_FRAME_CHUNK_MAX || (flags & ~SNAPPY_AMD_FRAME_STORE)) return SNAPPY_AMD_ERR_ARG;
    HostLease h;
    if (h.rc()) return h.rc();
    // chunk sequences concatenate: every piece after the first without the identifier
    const size_t kPiece = compress_piece_bytes(chunk);
    size_t at = 0, done = 0;
    do {
        const size_t piece = n - done < kPiece ? n - done : kPiece;
        size_t len = 0;
        int rc = frame_compress_piece(h.ctx(), in + done, piece, chunk,
                                      flags | (done ? SNAPPY_AMD_FRAME_NO_IDENTIFIER : 0u), out + at, cap - at, &len);
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
    return snappy_compress_file_framed_ex(fin, input_size, SNAPPY_AMD_BLOCK, 0u, fout);
}

int snappy_compress_file_framed_ex(FILE *fin, unsigned long long input_size, uint32_t chunk, uint32_t flags, FILE *fout)
{
    (void)input_size;
    if (!fin || !fout) return SNAPPY_AMD_ERR_ARG;
    if (chunk == 0 || chunk > SNAPPY_FRAME_CHUNK_MAX || (flags & ~SNAPPY_AMD_FRAME_STORE)) return SNAPPY_AMD_ERR_ARG;
    HostLease h;
    if (h.rc()) return h.rc();
    const size_t kPiece = compress_piece_bytes(chunk);
    std::vector<uint8_t> in(kPiece), out(snappy_amd_max_frame_output_ex(kPiece, chunk));
    bool first = true;
    for (;;) {
        const size_t n = read_full(fin, in.data(), in.size());
        if (ferror(fin)) return SNAPPY_AMD_ERR_IO;
        if (n == 0 && !first) break;
        size_t len = 0;
        int rc = frame_compress_piece(h.ctx(), in.data(), n, chunk,
                                      flags | (first ? 0u : SNAPPY_AMD_FRAME_NO_IDENTIFIER), out.data(), out.size(),
                                      &len);
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

int snappy_frame_tables(const uint8_t *in, size_t n, uint64_t *chunks, uint64_t *starts, size_t max_chunks,
                        size_t *nchunks_out, uint64_t *len)
{
    if (!in && n) return SNAPPY_AMD_ERR_ARG;
    std::vector<uint64_t> ch, st;
    uint64_t total = 0;
    const int rc = frame_walk_host(in, n, true, &ch, &total, nullptr, &st);
    if (rc) return rc;
    if ((chunks || starts) && ch.size() > max_chunks) return SNAPPY_AMD_ERR_CAPACITY;
    if (chunks) memcpy(chunks, ch.data(), ch.size() * sizeof(uint64_t));
    if (starts) memcpy(starts, st.data(), st.size() * sizeof(uint64_t));
    if (nchunks_out) *nchunks_out = ch.size() - 1;
    if (len) *len = total;
    return SNAPPY_AMD_OK;
}

int snappy_decompress_frame_range_buffer(const uint8_t *in, size_t n, uint64_t start, size_t length, uint8_t *out,
                                         size_t cap, size_t *out_len)
{
    if (!out_len || (n && !in) || (length && !out)) return SNAPPY_AMD_ERR_ARG;
    *out_len = 0;
    if (length > cap) return SNAPPY_AMD_ERR_CAPACITY;
    FrameSource src;
    src.clen = n;
    src.mem = in;
    const int rc = frame_range_core(src, nullptr, start, length, out);
    if (rc == SNAPPY_AMD_OK) *out_len = length;
    return rc;
}

int snappy_decompress_file_frame_range(FILE *file_input, uint64_t start, uint64_t length, FILE *file_out)
{
    if (!file_input || !file_out) return SNAPPY_AMD_ERR_ARG;
    FrameSource src;
    src.fd = fileno(file_input);
    src.base = ftello(file_input);
    if (src.fd < 0 || src.base < 0 || fseeko(file_input, 0, SEEK_END) != 0) return SNAPPY_AMD_ERR_UNSUPPORTED;
    const off_t end = ftello(file_input);
    if (end < src.base) return SNAPPY_AMD_ERR_UNSUPPORTED;
    src.clen = (uint64_t)(end - src.base);
    // (the output is allocated by the core, after the walk has found the range inside the stream)
    std::vector<uint8_t> out;
    const int rc = frame_range_core(src, file_input, start, length, nullptr, &out);
    if (rc) return rc;
    if (length && fwrite(out.data(), 1, (size_t)length, file_out) != length) return SNAPPY_AMD_ERR_IO;
    return fflush(file_out) ? SNAPPY_AMD_ERR_IO : SNAPPY_AMD_OK;
}

}  // extern "C"

// snappy_container_host.cpp -- Hadoop and snappy-java container streams over
// host memory and FILE*: host C++ on the device API of snappy_container.hip,
// with the pooled host contexts of snappy_pipeline.cpp (host_ctx_lease).  No
// kernel is launched here.
//
// The headers are walked on the host: the stream is in host memory, so the
// walk costs nothing beside the H2D copy, and its chunk tables are uploaded in
// place of the device walk (KC1).  Both follow snappy_container_step
// (snappy_container.h).  Large inputs go piece by piece: the compressors in
// pieces that are a multiple of the block, the decoders in runs of whole
// chunks.  The range forms walk only up to the chunk that holds
// the range's last byte, 16 bytes per hop, and hand the span's payloads and
// sub-tables to snappy_amd_decompress_container_ranges_device.  Declared in
// include/snappy_amd.h.
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
#include "snappy_container.h"
#include "snappy_container_ranges.h"
#include "snappy_ctx.h"

namespace {
// Bytes a call handles at a time.  SNAPPY_AMD_CONTAINER_PIECE_KB (read at every
// call) sets another size: the tests use it to cross piece boundaries with
// small inputs.
size_t piece_bytes()
{
    const char *e = getenv("SNAPPY_AMD_CONTAINER_PIECE_KB");
    const long kb = e ? atol(e) : 0;
    if (kb >= 1 && kb <= (4l << 20)) return (size_t)kb << 10;
    return (size_t)64 << 20;
}

// the compressors' piece: the largest multiple of the block inside piece_bytes(), one block at the least
size_t compress_piece(size_t block)
{
    const size_t p = piece_bytes();
    return p < block ? block : p - p % block;
}

bool known(int format) { return format == SNAPPY_AMD_CONTAINER_HADOOP || format == SNAPPY_AMD_CONTAINER_XERIAL; }

size_t block_of(uint32_t block, int format)
{
    if (block) return block;
    return format == SNAPPY_AMD_CONTAINER_HADOOP ? SNAPPY_CONTAINER_HADOOP_BLOCK : SNAPPY_CONTAINER_XERIAL_BLOCK;
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

// the walk's state between the pieces of one stream
struct WalkState {
    int first;   // the snappy-java header is still owed
    uint64_t R;  // bytes left in the open Hadoop block
};

// Walk in[0..n) from state *s.  comp / outp (when given) get the chunk tables,
// offsets counted from in and from the first decoded byte of this call; *total =
// decoded bytes of the whole chunks; *stop = where the walk ended: n, or the
// step that failed (every step before it is whole, so a reader with more bytes
// coming cuts there on SNAPPY_AMD_ERR_TRUNCATED and walks on from *s).  final:
// the stream ends at n (snappy_container_end).
int container_walk_host(const uint8_t *in, size_t n, int format, WalkState *s, bool final, std::vector<uint64_t> *comp,
                        std::vector<uint64_t> *outp, uint64_t *total, size_t *stop)
{
    size_t pos = 0;
    uint64_t sum = 0;
    int rc = SNAPPY_AMD_OK;
    while (pos < n) {
        uint32_t x[4], coff, cl, dlen;
        uint64_t adv;
        const uint64_t avail = n - pos;
        snappy_container_window(in + pos, avail, x);
        const int r = snappy_container_step(x, avail, format, s->first, &s->R, &coff, &cl, &dlen, &adv);
        if (r < 0) {
            rc = r;
            break;
        }
        s->first = 0;
        if (r == 1) {
            if (comp) {
                comp->push_back(pos + coff);
                comp->push_back(cl);
            }
            if (outp) {
                outp->push_back(sum);
                outp->push_back(dlen);
            }
            sum += dlen;
        }
        pos += (size_t)adv;
    }
    if (rc == SNAPPY_AMD_OK && final) rc = snappy_container_end(format, s->first, s->R);
    if (total) *total = sum;
    if (stop) *stop = pos;
    return rc;
}

// compress in[0..n) (at most one piece) on context c, *len bytes to out
int container_compress_piece(snappy_amd_ctx *c, const uint8_t *in, size_t n, uint32_t block, int format, uint32_t flags,
                             uint8_t *out, size_t cap, size_t *len)
{
    const size_t need = snappy_amd_max_container_output(n, block, format);
    int rc;
    if ((rc = grow(reinterpret_cast<void **>(&c->d_a), &c->d_a_cap, n + 16))) return rc;
    if ((rc = grow(reinterpret_cast<void **>(&c->d_b), &c->d_b_cap, need + 16))) return rc;
    if (n) HIP_OK(hipMemcpyAsync(c->d_a, in, n, hipMemcpyHostToDevice, c->stream));
    if ((rc = snappy_amd_compress_container_device(c, c->d_a, n, block, format, flags, c->d_b, need, nullptr, nullptr, 0,
                                                   nullptr, len)))
        return rc;
    if (*len > cap) return SNAPPY_AMD_ERR_CAPACITY;
    if (*len) HIP_OK(hipMemcpyAsync(out, c->d_b, *len, hipMemcpyDeviceToHost, c->stream));
    HIP_OK(hipStreamSynchronize(c->stream));
    return SNAPPY_AMD_OK;
}

// Decode the chunks [i0, i1) of a walk's tables (pairs in comp / outp, offsets
// from `in`) on context c: their bytes of the container go up, the tables are
// rebased to them, the decoded bytes come back to out (the run's own first byte
// at out[0]).
int container_decode_run(snappy_amd_ctx *c, const uint8_t *in, int format, const std::vector<uint64_t> &comp,
                         const std::vector<uint64_t> &outp, size_t i0, size_t i1, uint8_t *out, size_t *out_len)
{
    *out_len = 0;
    if (i0 == i1) return SNAPPY_AMD_OK;
    const size_t nch = i1 - i0;
    const uint64_t c0 = comp[2 * i0], c1 = comp[2 * (i1 - 1)] + comp[2 * (i1 - 1) + 1];
    const uint64_t o0 = outp[2 * i0], o1 = outp[2 * (i1 - 1)] + outp[2 * (i1 - 1) + 1];
    const size_t span = (size_t)(c1 - c0), total = (size_t)(o1 - o0);
    std::vector<uint64_t> tab(4 * nch);
    for (size_t i = 0; i < nch; i++) {
        tab[2 * i] = comp[2 * (i0 + i)] - c0;
        tab[2 * i + 1] = comp[2 * (i0 + i) + 1];
        tab[2 * nch + 2 * i] = outp[2 * (i0 + i)] - o0;
        tab[2 * nch + 2 * i + 1] = outp[2 * (i0 + i) + 1];
    }
    int rc;
    if ((rc = grow(reinterpret_cast<void **>(&c->d_a), &c->d_a_cap, span + 16))) return rc;
    if ((rc = grow(reinterpret_cast<void **>(&c->d_b), &c->d_b_cap, total + 16))) return rc;
    // (the tables go to f_meta: d_idx is the long-record decoder's own scratch)
    if ((rc = grow(reinterpret_cast<void **>(&c->f_meta), &c->f_meta_cap, tab.size() * sizeof(uint64_t)))) return rc;
    uint64_t *d_tab = reinterpret_cast<uint64_t *>(c->f_meta);
    HIP_OK(hipMemcpyAsync(c->d_a, in + c0, span, hipMemcpyHostToDevice, c->stream));
    HIP_OK(hipMemcpyAsync(d_tab, tab.data(), tab.size() * sizeof(uint64_t), hipMemcpyHostToDevice, c->stream));
    HIP_OK(hipStreamSynchronize(c->stream));  // (tab is pageable: its bytes are taken before the call goes on)
    size_t got = 0;
    if ((rc = snappy_amd_decompress_container_device(c, c->d_a, span, format, d_tab, d_tab + 2 * nch, nch, c->d_b, total,
                                                     &got)))
        return rc;
    if (got) HIP_OK(hipMemcpyAsync(out, c->d_b, got, hipMemcpyDeviceToHost, c->stream));
    HIP_OK(hipStreamSynchronize(c->stream));
    *out_len = got;
    return SNAPPY_AMD_OK;
}

// all chunks of a walk, in runs of whole chunks whose container bytes fit a piece (one chunk at the least)
int container_decode_all(snappy_amd_ctx *c, const uint8_t *in, int format, const std::vector<uint64_t> &comp,
                         const std::vector<uint64_t> &outp, uint8_t *out, size_t *out_len)
{
    const size_t nch = comp.size() / 2, kPiece = piece_bytes();
    size_t at = 0;
    for (size_t i0 = 0; i0 < nch;) {
        size_t i1 = i0 + 1;
        while (i1 < nch && comp[2 * i1] + comp[2 * i1 + 1] - comp[2 * i0] <= kPiece) i1++;
        size_t len = 0;
        int rc = container_decode_run(c, in, format, comp, outp, i0, i1, out + at, &len);
        if (rc) return rc;
        at += len;
        i0 = i1;
    }
    *out_len = at;
    return SNAPPY_AMD_OK;
}

// ---- range decode ------------------------------------------
// a container the host can read at any position: host memory, or a file
// descriptor whose stream starts at `base` (positional reads: the FILE*'s own
// position and buffer are not touched by the walk)
struct ContainerSource {
    uint64_t clen = 0;
    const uint8_t *mem = nullptr;
    int fd = -1;
    off_t base = 0;
    // x = the window of snappy_container_step at pos: 16 bytes, zero past the stream's end
    int head(uint64_t pos, uint32_t x[4]) const
    {
        uint8_t w[SNAPPY_CONTAINER_WINDOW] = {};
        const uint64_t avail = clen - pos;
        const size_t want = avail < SNAPPY_CONTAINER_WINDOW ? (size_t)avail : SNAPPY_CONTAINER_WINDOW;
        if (mem) {
            memcpy(w, mem + pos, want);
        } else {
            size_t got = 0;
            while (got < want) {
                const ssize_t k = pread(fd, w + got, want - got, base + (off_t)(pos + got));
                if (k <= 0) return SNAPPY_AMD_ERR_IO;
                got += (size_t)k;
            }
        }
        snappy_container_window(w, want, x);
        return SNAPPY_AMD_OK;
    }
};

// Hop from header to header until `target` decoded bytes are covered (the chunk
// holding byte target - 1 is the last one looked at) or the stream ends, which is
// then checked as the whole-stream walk checks it; no payload beyond the step's 16
// bytes is read.  comp / outp = the tables of the chunks seen; Hadoop's open block
// and the owed snappy-java header are carried from hop to hop.
int container_walk_to(const ContainerSource &src, int format, uint64_t target, std::vector<uint64_t> *comp,
                      std::vector<uint64_t> *outp)
{
    WalkState s = {format == SNAPPY_AMD_CONTAINER_XERIAL, 0};
    uint64_t pos = 0, sum = 0;
    while (sum < target) {
        if (pos >= src.clen) return snappy_container_end(format, s.first, s.R);
        uint32_t x[4], coff, cl, dlen;
        uint64_t adv;
        int rc = src.head(pos, x);
        if (rc) return rc;
        const int r = snappy_container_step(x, src.clen - pos, format, s.first, &s.R, &coff, &cl, &dlen, &adv);
        if (r < 0) return r;
        s.first = 0;
        if (r == 1) {
            comp->push_back(pos + coff);
            comp->push_back(cl);
            outp->push_back(sum);
            outp->push_back(dlen);
            sum += dlen;
        }
        pos += adv;
    }
    return SNAPPY_AMD_OK;
}

// out[0, length) = decoded bytes [start, start + length) of the container; with
// `own` the output is own's, sized only once the walk has shown that the range
// exists.  An allocation that fails is SNAPPY_AMD_ERR_DEVICE, as in the other host forms.
int container_range_walked(const ContainerSource &src, FILE *file, int format, uint64_t start, uint64_t length,
                           uint8_t *out, std::vector<uint8_t> *own)
{
    if (start + length < start) return SNAPPY_AMD_ERR_ARG;
    std::vector<uint64_t> comp, outp;
    int rc = container_walk_to(src, format, start + length, &comp, &outp);
    if (rc) return rc;
    const uint64_t nchunks = outp.size() / 2;
    const snappy_amd_range whole = {start, length, 0};
    uint64_t u0, u1, k;
    // (a walk from the stream's first byte: outp[0] = 0, so ERR_ARG is a range past the decoded bytes)
    if ((rc = snappy_container_span(outp.data(), nchunks, whole, length, &u0, &u1, &k))) return rc;
    if (k == 0) return SNAPPY_AMD_OK;
    if (own) {
        own->resize((size_t)length);
        out = own->data();
    }
    const uint64_t w0 = comp[2 * u0], w1 = comp[2 * u1] + comp[2 * u1 + 1];
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
    // of chunks u0 .. u1, offsets absolute; the output as aligned as the range.  (The tables
    // go to k5copy: f_meta, k5buf and d_idx are the range call's and the decoder's own.)
    const size_t pad = (size_t)(w0 & 3), oo = (size_t)(start & 15), pairs = 2 * (size_t)k;
    if ((rc = grow(reinterpret_cast<void **>(&c->d_a), &c->d_a_cap, win.size() + pad + 16))) return rc;
    if ((rc = grow(reinterpret_cast<void **>(&c->d_b), &c->d_b_cap, (size_t)length + oo + 16))) return rc;
    if ((rc = grow(reinterpret_cast<void **>(&c->k5copy), &c->k5copy_cap, 2 * pairs * sizeof(uint64_t)))) return rc;
    uint64_t *d_tab = reinterpret_cast<uint64_t *>(c->k5copy);
    HIP_OK(hipMemcpyAsync(c->d_a + pad, win.data(), win.size(), hipMemcpyHostToDevice, c->stream));
    HIP_OK(hipMemcpyAsync(d_tab, comp.data() + 2 * u0, pairs * sizeof(uint64_t), hipMemcpyHostToDevice, c->stream));
    HIP_OK(hipMemcpyAsync(d_tab + pairs, outp.data() + 2 * u0, pairs * sizeof(uint64_t), hipMemcpyHostToDevice,
                          c->stream));
    const snappy_amd_range r = {start, length, oo};
    if ((rc = snappy_amd_decompress_container_ranges_device(c, c->d_a + pad, w0, win.size(), d_tab, d_tab + pairs,
                                                            (size_t)k, &r, 1, c->d_b, (size_t)length + oo, nullptr)))
        return rc;
    HIP_OK(hipMemcpyAsync(out, c->d_b + oo, (size_t)length, hipMemcpyDeviceToHost, c->stream));
    HIP_OK(hipStreamSynchronize(c->stream));
    return SNAPPY_AMD_OK;
}

int container_range_core(const ContainerSource &src, FILE *file, int format, uint64_t start, uint64_t length,
                         uint8_t *out, std::vector<uint8_t> *own = nullptr)
{
    try {
        return container_range_walked(src, file, format, start, length, out, own);
    } catch (const std::bad_alloc &) {
        return SNAPPY_AMD_ERR_DEVICE;
    } catch (const std::length_error &) {
        return SNAPPY_AMD_ERR_DEVICE;
    }
}
}  // namespace

extern "C" {

int snappy_container_uncompressed_length(const uint8_t *in, size_t n, int format, uint64_t *len)
{
    if (!len || (!in && n) || !known(format)) return SNAPPY_AMD_ERR_ARG;
    WalkState s = {format == SNAPPY_AMD_CONTAINER_XERIAL, 0};
    return container_walk_host(in, n, format, &s, true, nullptr, nullptr, len, nullptr);
}

int snappy_compress_container_buffer(const uint8_t *in, size_t n, uint32_t block, int format, uint8_t *out, size_t cap,
                                     size_t *out_len)
{
    if (!out_len || (!in && n) || !out || !known(format) || block > SNAPPY_CONTAINER_CHUNK_MAX) return SNAPPY_AMD_ERR_ARG;
    *out_len = 0;
    if (cap < snappy_amd_max_container_output(n, block, format)) return SNAPPY_AMD_ERR_CAPACITY;
    HostLease h;
    if (h.rc()) return h.rc();
    // chunk sequences concatenate: every piece after the first without the stream header
    const size_t kPiece = compress_piece(block_of(block, format));
    size_t at = 0, done = 0;
    do {
        const size_t piece = n - done < kPiece ? n - done : kPiece;
        size_t len = 0;
        int rc = container_compress_piece(h.ctx(), in + done, piece, block, format,
                                          done ? SNAPPY_AMD_CONTAINER_NO_HEADER : 0u, out + at, cap - at, &len);
        if (rc) return rc;
        at += len;
        done += piece;
    } while (done < n);
    *out_len = at;
    return SNAPPY_AMD_OK;
}

int snappy_decompress_container_buffer(const uint8_t *in, size_t n, int format, uint8_t *out, size_t cap, size_t *out_len)
{
    if (!out_len || (!in && n) || (!out && cap) || !known(format)) return SNAPPY_AMD_ERR_ARG;
    *out_len = 0;
    // malformed streams, short buffers and streams without a chunk end here, before any device call
    std::vector<uint64_t> comp, outp;
    uint64_t total = 0;
    WalkState s = {format == SNAPPY_AMD_CONTAINER_XERIAL, 0};
    int rc = container_walk_host(in, n, format, &s, true, &comp, &outp, &total, nullptr);
    if (rc) return rc;
    if (total > cap) return SNAPPY_AMD_ERR_CAPACITY;
    if (comp.empty()) return SNAPPY_AMD_OK;
    HostLease h;
    if (h.rc()) return h.rc();
    return container_decode_all(h.ctx(), in, format, comp, outp, out, out_len);
}

int snappy_compress_file_container(FILE *fin, unsigned long long input_size, uint32_t block, int format, FILE *fout)
{
    (void)input_size;
    if (!fin || !fout || !known(format) || block > SNAPPY_CONTAINER_CHUNK_MAX) return SNAPPY_AMD_ERR_ARG;
    HostLease h;
    if (h.rc()) return h.rc();
    const size_t kPiece = compress_piece(block_of(block, format));
    std::vector<uint8_t> in(kPiece), out(snappy_amd_max_container_output(kPiece, block, format));
    bool first = true;
    for (;;) {
        const size_t n = read_full(fin, in.data(), in.size());
        if (ferror(fin)) return SNAPPY_AMD_ERR_IO;
        if (n == 0 && !first) break;
        size_t len = 0;
        int rc = container_compress_piece(h.ctx(), in.data(), n, block, format,
                                          first ? 0u : SNAPPY_AMD_CONTAINER_NO_HEADER, out.data(), out.size(), &len);
        if (rc) return rc;
        if (len && fwrite(out.data(), 1, len, fout) != len) return SNAPPY_AMD_ERR_IO;
        first = false;
        if (n < in.size()) break;
    }
    return fflush(fout) ? SNAPPY_AMD_ERR_IO : SNAPPY_AMD_OK;
}

int snappy_decompress_file_container(FILE *fin, int format, FILE *fout)
{
    if (!fin || !fout || !known(format)) return SNAPPY_AMD_ERR_ARG;
    HostLease h;
    if (h.rc()) return h.rc();
    std::vector<uint8_t> in(piece_bytes()), out;
    std::vector<uint64_t> comp, outp;
    WalkState s = {format == SNAPPY_AMD_CONTAINER_XERIAL, 0};
    size_t have = 0;
    bool eof = false;
    while (!eof) {
        have += read_full(fin, in.data() + have, in.size() - have);
        if (ferror(fin)) return SNAPPY_AMD_ERR_IO;
        eof = have < in.size();
        uint64_t total = 0;
        size_t stop = 0;
        comp.clear();
        outp.clear();
        int rc = container_walk_host(in.data(), have, format, &s, eof, &comp, &outp, &total, &stop);
        if (rc == SNAPPY_AMD_ERR_TRUNCATED && !eof) {
            // the rest comes with the next read: decode the whole chunks now and carry
            // the cut one over (with the state: Hadoop's open block goes on in the next
            // piece); a chunk larger than the buffer needs a larger one
            if (stop == 0) {
                in.resize(in.size() * 2);
                continue;
            }
            rc = SNAPPY_AMD_OK;
        }
        if (rc) return rc;
        if (out.size() < total) out.resize((size_t)total);
        size_t len = 0;
        if ((rc = container_decode_all(h.ctx(), in.data(), format, comp, outp, out.data(), &len))) return rc;
        if (len && fwrite(out.data(), 1, len, fout) != len) return SNAPPY_AMD_ERR_IO;
        memmove(in.data(), in.data() + stop, have - stop);
        have -= stop;
    }
    return fflush(fout) ? SNAPPY_AMD_ERR_IO : SNAPPY_AMD_OK;
}

int snappy_container_tables(const uint8_t *in, size_t n, int format, uint64_t *comp_off_len, uint64_t *out_off_len,
                            size_t max_chunks, size_t *nchunks_out, uint64_t *len)
{
    if ((!in && n) || !known(format)) return SNAPPY_AMD_ERR_ARG;
    std::vector<uint64_t> comp, outp;
    uint64_t total = 0;
    WalkState s = {format == SNAPPY_AMD_CONTAINER_XERIAL, 0};
    const int rc = container_walk_host(in, n, format, &s, true, &comp, &outp, &total, nullptr);
    if (rc) return rc;
    if (nchunks_out) *nchunks_out = comp.size() / 2;
    if (len) *len = total;
    if ((comp_off_len || out_off_len) && comp.size() / 2 > max_chunks) return SNAPPY_AMD_ERR_CAPACITY;
    if (comp_off_len && !comp.empty()) memcpy(comp_off_len, comp.data(), comp.size() * sizeof(uint64_t));
    if (out_off_len && !outp.empty()) memcpy(out_off_len, outp.data(), outp.size() * sizeof(uint64_t));
    return SNAPPY_AMD_OK;
}

int snappy_decompress_container_range_buffer(const uint8_t *in, size_t n, int format, uint64_t start, size_t length,
                                             uint8_t *out, size_t cap, size_t *out_len)
{
    if (!out_len || (n && !in) || (length && !out) || !known(format)) return SNAPPY_AMD_ERR_ARG;
    *out_len = 0;
    if (length > cap) return SNAPPY_AMD_ERR_CAPACITY;
    ContainerSource src;
    src.clen = n;
    src.mem = in;
    const int rc = container_range_core(src, nullptr, format, start, length, out);
    if (rc == SNAPPY_AMD_OK) *out_len = length;
    return rc;
}

int snappy_decompress_file_container_range(FILE *file_input, int format, uint64_t start, uint64_t length,
                                           FILE *file_out)
{
    if (!file_input || !file_out || !known(format)) return SNAPPY_AMD_ERR_ARG;
    ContainerSource src;
    src.fd = fileno(file_input);
    src.base = ftello(file_input);
    if (src.fd < 0 || src.base < 0 || fseeko(file_input, 0, SEEK_END) != 0) return SNAPPY_AMD_ERR_UNSUPPORTED;
    const off_t end = ftello(file_input);
    if (end < src.base) return SNAPPY_AMD_ERR_UNSUPPORTED;
    src.clen = (uint64_t)(end - src.base);
    // (the output is allocated by the core, after the walk has found the range inside the stream)
    std::vector<uint8_t> out;
    const int rc = container_range_core(src, file_input, format, start, length, nullptr, &out);
    if (rc) return rc;
    if (length && fwrite(out.data(), 1, (size_t)length, file_out) != length) return SNAPPY_AMD_ERR_IO;
    return fflush(file_out) ? SNAPPY_AMD_ERR_IO : SNAPPY_AMD_OK;
}

}  // extern "C"

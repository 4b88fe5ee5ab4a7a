/*
 * snappy_amd.h -- C ABI of the MI355X-native Snappy block codec.
 *
 * The drop-in entry points keep the reference signatures exactly
 * (declared again in snappy_compression.h / snappy_decompression.h /
 * snappy_compression_tree.h so src/cmd.c compiles unchanged):
 *
 *   snappy_compress      <- src/snappy_compression.h:8   (def .c:414-428)
 *   snappy_decompress    <- src/snappy_decompression.h:15 (def .c:345-363)
 *   snappy_compress_bst  <- src/snappy_compression_tree.h:10 (def .c:291-306)
 *
 * Added below them: an in-memory host-buffer API and a
 * device-resident (HBM pointer) batch API.  All compute runs in hand-written
 * HIP kernels for gfx950; there is no CPU fallback in this library.  (The
 * reference's -b BST compressor, a different algorithm with different output
 * and not the GPU path, runs on host threads: snappy_compress_bst.)  Every
 * function returns 0 (SNAPPY_AMD_OK) or a negative error code.
 */
#ifndef SNAPPY_AMD_H
#define SNAPPY_AMD_H

#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- status codes ---------------------------------------------------- */
#define SNAPPY_AMD_OK 0
#define SNAPPY_AMD_ERR_ARG (-1)        /* bad argument (NULL, chunk > 65536, ...) */
#define SNAPPY_AMD_ERR_HEADER (-2)     /* unreadable varint length preamble      */
#define SNAPPY_AMD_ERR_TRUNCATED (-3)  /* element runs past the end of its input  */
#define SNAPPY_AMD_ERR_OFFSET (-4)     /* copy offset 0 or before the block start */
#define SNAPPY_AMD_ERR_OVERRUN (-5)    /* element runs past the declared length   */
#define SNAPPY_AMD_ERR_CAPACITY (-6)   /* caller's output buffer too small        */
#define SNAPPY_AMD_ERR_DEVICE (-7)     /* HIP runtime error / no device           */
#define SNAPPY_AMD_ERR_IO (-8)         /* FILE* read/write failure                */
#define SNAPPY_AMD_ERR_UNSUPPORTED (-9)
#define SNAPPY_AMD_ERR_TIMEOUT (-10)   /* a block waited too long for an earlier one  */
#define SNAPPY_AMD_ERR_INDEX (-11)     /* a sidecar index that does not fit the stream */
#define SNAPPY_AMD_ERR_CHECKSUM (-12)  /* a framed chunk's CRC-32C does not match its decoded bytes */

/* Block size of the reference stream format (src/snappy_compression.c:9). */
#define SNAPPY_AMD_BLOCK 65536u

/* Stream layouts handled by the batch API. */
#define SNAPPY_AMD_SINGLE 0  /* one stream: varint(n) ++ 65536-byte blocks       */
#define SNAPPY_AMD_STREAMS 1 /* n cut into `chunk`-byte pieces, each one stream  */

/* ---- drop-in FILE* API (reference signatures) ------------------------ */
void snappy_compress(FILE *file_input, unsigned long long input_size, FILE *file_compressed);
int snappy_decompress(FILE *file_input, FILE *file_decompressed);
/* the -b mode: the reference's BST-matcher stream, byte for byte, computed by
 * a pool of host threads (<= 16, SNAPPY_AMD_BST_THREADS), one block each */
int snappy_compress_bst(FILE *file_input, unsigned long long input_size, FILE *file_compressed);

/* Status of the last snappy_compress / snappy_decompress call on this
 * thread (the reference signatures cannot return one). */
int snappy_amd_last_status(void);

/* The compile-time knobs of the library's gfx950 kernels, e.g.
 * "compress{measurement=0 k1r_dmax=10 ...} decode{measurement=0 k4_nofar=0 ...}".
 * measurement=1 marks a build that may write wrong bytes (timing experiments)
 * or carries statistics code: never a product library. */
const char *snappy_amd_build_config(void);

/* Sidecar block index (the stream format has no block
 * markers).  File layout, little-endian u64 words: SNAPPY_AMD_IDX_MAGIC, N
 * (decoded bytes), count = ceil(N/65536) + 1, then `count` block-index
 * entries in the format of snappy_amd_decompress_device below (byte offsets
 * from the start of the stream, its varint preamble included; the last entry
 * is the stream length).  With it, decoding skips the index pass. */
#define SNAPPY_AMD_IDX_MAGIC 0x3158444941504e53ull /* "SNPAIDX1" */
/* snappy_compress() that also writes the sidecar index of its output to idx */
int snappy_compress_file_indexed(FILE *file_input, unsigned long long input_size, FILE *file_compressed, FILE *idx);
/* snappy_decompress() using a sidecar index.  SNAPPY_AMD_ERR_INDEX if the
 * index is not this stream's own block index: a malformed file (magic, count,
 * an entry outside the stream or decreasing) is refused before any decoding;
 * an entry moved off an element boundary is refused by the decode (each
 * block's element chain must end exactly at the next entry), and a decode
 * that fails for any other reason is checked against the stream's own index
 * (GPU index pass): a different sidecar -> ERR_INDEX, the same -> the
 * stream's error, as snappy_decompress reports it.  Success implies the
 * sidecar was the stream's index and the output is snappy_decompress's. */
int snappy_decompress_file_indexed(FILE *file_input, FILE *idx, FILE *file_decompressed);

/* ---- varint preamble (src/varint.c) ---------------------------------- */
/* LEB128 of n into out (<= 10 bytes); returns bytes written. varint.c:12-20 */
uint32_t snappy_varint_encode(uint64_t n, uint8_t *out);
/* 64-bit LEB128 decode; returns bytes consumed or 0. (varint.c:28-42 uses
 * `int` and overflows at 2^31; this one does not.) */
uint32_t snappy_varint_decode(const uint8_t *in, size_t n, uint64_t *value);

/* ---- host-memory API -------------------------------------------------- */
/* Upper bound of snappy_compress output for n input bytes. */
size_t snappy_max_compressed_length(size_t n);
/* Same bytes as snappy_compress() on a FILE holding in[0..n); n == 0 gives
 * 0 bytes.  out must hold snappy_max_compressed_length(n). */
int snappy_compress_buffer(const uint8_t *in, size_t n, uint8_t *out, size_t *out_len);
/* Same bytes as snappy_compress_bst() on a FILE holding in[0..n) (the -b
 * stream; snappy_decompress_buffer decodes it).  out must hold
 * snappy_max_compressed_length(n); n == 0 gives 0 bytes. */
int snappy_compress_bst_buffer(const uint8_t *in, size_t n, uint8_t *out, size_t cap, size_t *out_len);
/* Decode one stream; *out_len = declared length. */
int snappy_decompress_buffer(const uint8_t *in, size_t n, uint8_t *out, size_t cap, size_t *out_len);
int snappy_uncompressed_length(const uint8_t *in, size_t n, uint64_t *len);

/* Threads and devices of the host-memory and FILE* calls above.  Each call
 * leases a pooled host context (its own streams, device scratch and pinned
 * staging) of the calling thread's device and returns it when it ends, so
 * calls from several threads run concurrently.  The device is the one set
 * here for the calling thread (-1: back to the default), else the
 * SNAPPY_AMD_DEVICE environment variable (read once), else 0. */
int snappy_amd_host_set_device(int device);
int snappy_amd_host_get_device(void);
/* Free every idle pooled host context (device scratch and pinned staging). */
int snappy_amd_host_release(void);
/* Idle host contexts in the pool (diagnostics). */
size_t snappy_amd_host_pool_size(void);

/* The host-memory API over several devices (a device may be listed more
 * than once).  Compress: the input's 65,536-byte blocks are split into one
 * contiguous range per device (the first range writes the preamble), each
 * compressed on its device by its own thread; once every range's size is
 * known (C1) each device copies its bytes to their place in out (C2).  The
 * bytes equal snappy_compress_buffer's; out must hold
 * snappy_max_compressed_length(n).  Decompress: the first device builds the
 * block index, every device decodes one range of blocks from its part of the
 * stream; a stream whose ranges are not self-contained (elements straddling a
 * range start, copies reaching an earlier range) is decoded whole on the
 * first device instead, so the results equal snappy_decompress_buffer's. */
int snappy_compress_buffer_multi(const int *devices, int ndev, const uint8_t *in, size_t n, uint8_t *out,
                                 size_t *out_len);
int snappy_decompress_buffer_multi(const int *devices, int ndev, const uint8_t *in, size_t n, uint8_t *out,
                                   size_t cap, size_t *out_len);

/* ---- device-resident batch API (all pointers are HBM) ----------------- */
typedef struct snappy_amd_ctx snappy_amd_ctx;

int snappy_amd_create(int device, snappy_amd_ctx **ctx);
void snappy_amd_destroy(snappy_amd_ctx *ctx);
/* Launch on this hipStream_t (NULL = the context's own stream, a blocking
 * stream: ordered after work queued on the legacy default stream).
 *
 * The calls of one context are ordered by its bound stream and by nothing
 * else: every kernel, memset, copy and read-back of a device call goes to the
 * stream bound when the call is made, so a call reads its inputs after the
 * work queued on that stream before it, and work queued there afterwards sees
 * its outputs.  The context's scratch, its result words and the pinned words
 * it reads back through are shared by all its calls and are safe only in that
 * order: one context is used from one thread at a time, on one stream at a
 * time.  A stream may be non-blocking.
 *
 * set_stream itself queues and waits for nothing.  Rebinding a context while
 * work of a queued form (compress_device without out_len, decompress_device_async,
 * sync = 0, crc32c_device, records_length_device) is still in flight on the
 * old stream is for the caller to order: the next call would reuse the scratch
 * on the new stream, and decompress_status reads the status words on the stream
 * bound when it is called, not on the one the decode was launched on.
 *
 * A queued form returns without waiting for the stream, with two exceptions:
 * a call that needs a scratch buffer larger than the context holds frees the
 * old one first, and hipFree waits for the device (so the work still using it
 * has ended: growing is safe, but not asynchronous); and decompress_ranges_device
 * waits for the previous range call's plan upload -- not for its kernels --
 * before it rewrites the pinned plan.  trim and destroy synchronise the bound
 * stream before they free anything. */
int snappy_amd_set_stream(snappy_amd_ctx *ctx, void *hip_stream);
void *snappy_amd_get_stream(snappy_amd_ctx *ctx);

/* Device bytes the context holds as scratch (token lists, segment records,
 * status words, staging of the host-buffer path, index scratch); it grows to
 * the largest call made and is kept.  A record batch (compress_records_device)
 * of `count` records holding `total` bytes needs at most S + S/8 + 16,512 with
 * S = 2 total + total/128 + 64 count + 256 (snappy_amd_max_records_scratch):
 * linear in the bytes and in the count. */
size_t snappy_amd_device_bytes(snappy_amd_ctx *ctx);
/* Release the scratch above (synchronises the context stream); the next call
 * allocates again.  The status words of a decode whose status has not been
 * read yet (decompress_device_async) are kept until it is read.  Used to make
 * room in HBM between phases (bench.py trims before C3, the all-gather of the
 * decoded shards, and between its sub-workloads). */
int snappy_amd_trim(snappy_amd_ctx *ctx);

/* Options of a context (snappy_amd_set_option). */
#define SNAPPY_AMD_OPT_SERIAL_INDEX 1 /* 1: index_device walks the stream with one wave
                                         (the chunk-parallel K5p pass otherwise) */
#define SNAPPY_AMD_OPT_K1R_EXTRA_LDS 2 /* bytes of extra dynamic LDS per K1r unit
                                          (occupancy experiments; default 0) */
int snappy_amd_set_option(snappy_amd_ctx *ctx, int option, int64_t value);

/* Number of units (blocks or streams) for n bytes in a layout. */
size_t snappy_amd_num_units(size_t n, uint32_t chunk, int layout);
/* Capacity d_out must have for compress_device. */
size_t snappy_amd_max_output(size_t n, uint32_t chunk, int layout);

/* Compress d_in[0..n).  layout SINGLE: one stream equal to snappy_compress()
 * (chunk ignored, blocks of 65536).  layout STREAMS: ceil(n/chunk)
 * independent streams, each equal to snappy_compress() of its chunk
 * (1 <= chunk <= 65536), concatenated.  d_offsets (nunits+1 u64, device)
 * receives each unit's byte offset in d_out -- the block index that lets
 * decompress_device run block-parallel.  *out_len (host) gets the total.
 * Asynchronous on the context stream except for the 8-byte total read. */
int snappy_amd_compress_device(snappy_amd_ctx *ctx, const void *d_in, size_t n, uint32_t chunk,
                               int layout, void *d_out, uint64_t *d_offsets, size_t *out_len);

/* Flags for the _ex forms. */
#define SNAPPY_AMD_NO_PREAMBLE 1u /* SINGLE layout: this buffer continues a stream
                                     (a rank > 0 shard): no varint preamble */

/* compress_device with an explicit preamble value and flags; a SINGLE-layout
 * stream sharded over ranks is rank 0 with header_value = the global length
 * and flags 0, every other rank with SNAPPY_AMD_NO_PREAMBLE (n must then be a
 * multiple of 65536 on every rank but the last). */
int snappy_amd_compress_device_ex(snappy_amd_ctx *ctx, const void *d_in, size_t n, uint32_t chunk, int layout,
                                  uint32_t flags, uint64_t header_value, void *d_out, uint64_t *d_offsets,
                                  size_t *out_len);

/* Block index entries (d_offsets, nunits+1 u64): bits [0,40) = byte offset in
 * the stream of the element holding the unit's first output byte; bits
 * [40,64) = how many output bytes of that element precede the unit (0 when
 * the element starts the unit -- always the case for streams this library
 * writes, whose entries are therefore plain offsets).  The last entry is the
 * stream's end.  Non-zero skips arise only in foreign SINGLE streams whose
 * elements cross 65,536-byte output boundaries (snappy_amd_index_device). */
#define SNAPPY_AMD_IDX_OFFSET_BITS 40

/* Decode what compress_device produced (or any stream whose block index is
 * given): n = total decoded bytes, d_offsets = the unit index.  SINGLE
 * layout decodes any valid stream: elements may straddle blocks and copies
 * may reach into earlier blocks (those blocks run in a second, ordered pass).
 * Returns the first failing unit's status (synchronises to read it). */
int snappy_amd_decompress_device(snappy_amd_ctx *ctx, const void *d_comp, const uint64_t *d_offsets,
                                 size_t n, uint32_t chunk, int layout, void *d_out);

/* Same as decompress_device without the status read-back (fully async);
 * fetch the status later with snappy_amd_decompress_status. */
int snappy_amd_decompress_device_async(snappy_amd_ctx *ctx, const void *d_comp, const uint64_t *d_offsets,
                                       size_t n, uint32_t chunk, int layout, void *d_out);
int snappy_amd_decompress_status(snappy_amd_ctx *ctx);
/* decompress with the flags/preamble value of compress_device_ex; sync = 1
 * reads back the status, 0 leaves it for snappy_amd_decompress_status. */
int snappy_amd_decompress_device_ex(snappy_amd_ctx *ctx, const void *d_comp, const uint64_t *d_offsets, size_t n,
                                    uint32_t chunk, int layout, uint32_t flags, uint64_t header_value, void *d_out,
                                    int sync);

/* Build the block index of a SINGLE-layout stream already in HBM (e.g. a
 * file produced by the reference or another encoder): d_offsets gets
 * ceil(N/65536)+1 entries (format above), *n_out the declared length N.
 * max_units = the entries d_offsets can hold (SNAPPY_AMD_ERR_CAPACITY if the
 * stream needs more).
 * SNAPPY_AMD_ERR_UNSUPPORTED only if a straddling element starts past 2^40
 * bytes or covers a boundary more than 2^24 - 1 bytes after its start. */
int snappy_amd_index_device(snappy_amd_ctx *ctx, const void *d_comp, size_t clen, uint64_t *d_offsets,
                            size_t max_units, size_t *n_out);

/* ---- record batches: many independent streams in one call ---------------- */
/* A record is one raw Snappy stream (varint preamble, then elements) of
 * 0..SNAPPY_AMD_RECORD_MAX decoded bytes; a batch is `count` records named by
 * (offset, length) u64 pairs relative to one base pointer (the form
 * snappy_amd_crc32c_device takes): any alignment, any order, gaps allowed --
 * Parquet/ORC pages between their headers, RPC or log records, KV blocks.
 * All three calls run on the context stream.
 *
 * Scratch: a compress call of `count` records holding `total` bytes grows
 * snappy_amd_device_bytes() to at most snappy_amd_max_records_scratch(total,
 * count) = S + S/8 + 16,512 with S = 2 total + total/128 + 64 count + 256:
 * per record of L bytes 8 (L/4 + 2) bytes of tokens and escapes, 8 bytes per 256
 * tokens of segment records and 32 bytes of plan tables, sizes and counts; the
 * eighth and the constant are the slack of the four buffers.  Linear in the
 * bytes and in the count -- not count * 65,536. */
#define SNAPPY_AMD_RECORD_MAX 65536u
/* Capacity d_out must have: total + total/32 + 32 count + 16 (per record the
 * bound of a one-unit SNAPPY_AMD_STREAMS launch). */
size_t snappy_amd_max_records_output(size_t total_bytes, size_t count);
size_t snappy_amd_max_records_scratch(size_t total_bytes, size_t count);

/* Compress record i = d_in[off_i, off_i + len_i) (d_in_off_len: count pairs,
 * device).  A record of len >= 1 becomes exactly the bytes of snappy_compress()
 * on it (the SNAPPY_AMD_STREAMS unit of chunk = len); len == 0 becomes the one
 * byte 00.  The compressed records are packed back to back in d_out;
 * d_offsets (count + 1 u64, device) gets each one's position and the total,
 * *out_len (host) the total.  d_status (count i32, device; may be NULL) gets 0
 * or the record's refusal: SNAPPY_AMD_ERR_UNSUPPORTED for len > 65,536,
 * SNAPPY_AMD_ERR_ARG for a range that leaves [0, in_bytes).  A refused record
 * writes 0 bytes, none of its bytes is loaded, and its neighbours are
 * compressed as usual; the call returns the first refused record's status (0:
 * none).  out_cap below snappy_amd_max_records_output(sum of the accepted
 * lengths, count): SNAPPY_AMD_ERR_CAPACITY, nothing written.  Synchronises
 * twice: for the plan's totals (which size the scratch) and for *out_len. */
int snappy_amd_compress_records_device(snappy_amd_ctx *ctx, const void *d_in, size_t in_bytes,
                                       const uint64_t *d_in_off_len, size_t count, void *d_out, size_t out_cap,
                                       uint64_t *d_offsets, int32_t *d_status, size_t *out_len);

/* Each record's declared length (its preamble: LEB128, the rules of
 * snappy_varint_decode) into d_len[i]; d_status[i] (may be NULL) = 0,
 * SNAPPY_AMD_ERR_HEADER for a malformed or cut preamble, SNAPPY_AMD_ERR_TRUNCATED
 * for a range outside comp_bytes -- both with length 0.  A length above 65,536
 * is returned as it is.  Asynchronous: returns once the kernel is queued. */
int snappy_amd_records_length_device(snappy_amd_ctx *ctx, const void *d_comp, size_t comp_bytes,
                                     const uint64_t *d_comp_off_len, size_t count, uint64_t *d_len,
                                     int32_t *d_status);

/* Decode record i from d_comp[comp_off_i, + comp_len_i) into d_out[out_off_i,
 * + out_len_i).  Any valid stream of any writer; its preamble must equal
 * out_len_i (SNAPPY_AMD_ERR_HEADER otherwise; records_length_device tells a
 * caller that does not know).  A record's bytes and status are those of a
 * one-unit snappy_amd_decompress_device(chunk = out_len_i, SNAPPY_AMD_STREAMS)
 * on the same bytes; a copy reaching before the record's start is
 * SNAPPY_AMD_ERR_OFFSET.  out_len_i == 0 needs the payload 00; an empty
 * compressed range is SNAPPY_AMD_ERR_HEADER.  Checked before any byte of the
 * record is loaded or stored: out_len_i > 65,536 SNAPPY_AMD_ERR_UNSUPPORTED, a
 * compressed range outside comp_bytes SNAPPY_AMD_ERR_TRUNCATED, an output range
 * outside out_bytes SNAPPY_AMD_ERR_CAPACITY.  A failing record may leave a
 * prefix of its own output range written, never a byte outside it; overlapping
 * output ranges are the caller's error.  d_status (count i32, device; may be
 * NULL) gets every record's status (never a positive value).  sync = 1 waits
 * and returns the first failing record's status, sync = 0 returns once queued. */
int snappy_amd_decompress_records_device(snappy_amd_ctx *ctx, const void *d_comp, size_t comp_bytes,
                                         const uint64_t *d_comp_off_len, size_t count, void *d_out, size_t out_bytes,
                                         const uint64_t *d_out_off_len, int32_t *d_status, int sync);

/* ---- long records: records of more than one block ------------------------- */
/* The calls above refuse a record above 65,536 bytes.  These take records of
 * 0..SNAPPY_AMD_LONG_RECORD_MAX decoded bytes -- a Parquet data page, an ORC
 * compression chunk, a large RPC payload -- each one raw Snappy stream, exactly
 * the bytes of snappy_compress(): varint(L), then blocks of 65,536 input bytes,
 * the last one shorter.  Records of 0..65,536 bytes are legal here and give the
 * bytes of the short calls.
 *
 * Block table (d_index, u64): record i has nblk_i = ceil(L_i / 65536) blocks and
 * owns nblk_i + 1 entries; the tables are packed in record order, record i's at
 * entry sum over k < i of (nblk_k + 1).  Entries have the format of
 * snappy_amd_index_device (bits [0,40) an offset, bits [40,64) a skip), their
 * offsets counted from the record's own first compressed byte: entry 0 is 0 (the
 * preamble), entry nblk (nblk >= 1) the record's compressed length; an empty or
 * a refused record owns the one entry 0.  Compress writes the tables; decode and
 * records_index_device find each record's slice by the same rule from the
 * decoded lengths, so a table holds only for the record order it was made for:
 * a caller who reorders records passes NULL or rebuilds it.
 * snappy_amd_max_records_index(total, count) = total/65536 + 2 count entries
 * hold the tables of `count` records of `total` bytes.
 *
 * Scratch: a call grows snappy_amd_device_bytes() to at most
 * snappy_amd_max_long_records_scratch(total, count) = S + S/8 + 24,704 with
 *   S = 2 total + total/128 + 80 U + 64 count + 8 E + 512,
 *   U = total/65536 + count (units: blocks, one per empty record),
 *   E = total/65536 + 2 count (table entries).
 * Per unit of L bytes: 8 (L/4 + 2) bytes of tokens and escapes and 8 bytes per
 * 256 tokens of segment records (<= 2 L + L/128 + 28), 8 bytes of size and token
 * count, 32 bytes of unit tables (record word, scratch need, two list slots,
 * scratch offset, output offset) -- 68, counted as 80; the decode's 8 bytes per
 * unit (record word, status word) reuse the unit tables' buffer.  Per record: 28
 * bytes of plan tables and pass 2's two words, counted as 64.  8 bytes per
 * table entry when decode builds the tables.  The eighth and the constant are
 * the slack of the six buffers.  Linear in the bytes and in the count. */
#define SNAPPY_AMD_LONG_RECORD_MAX (1u << 30)
/* Capacity d_out must have: total + total/32 + 32 (count + total/65536) + 16
 * (the one-unit bound of the short call, taken per block). */
size_t snappy_amd_max_long_records_output(size_t total_bytes, size_t count);
size_t snappy_amd_max_long_records_scratch(size_t total_bytes, size_t count);
size_t snappy_amd_max_records_index(size_t total_bytes, size_t count); /* entries */

/* compress_records_device for long records.  Statuses and packing as there:
 * len > SNAPPY_AMD_LONG_RECORD_MAX is SNAPPY_AMD_ERR_UNSUPPORTED (checked before
 * the range), a range that leaves [0, in_bytes) SNAPPY_AMD_ERR_ARG; a refused
 * record writes 0 bytes, none of its bytes is loaded, it owns one table entry
 * (0), and its neighbours are compressed as usual.  d_index (may be NULL: no
 * table is written) gets the block tables, index_cap = the entries it can hold.
 * out_cap below snappy_amd_max_long_records_output(sum of the accepted lengths,
 * count), or index_cap below the entries needed: SNAPPY_AMD_ERR_CAPACITY, nothing
 * written.  Synchronises twice: for the plan's totals and for *out_len. */
int snappy_amd_compress_long_records_device(snappy_amd_ctx *ctx, const void *d_in, size_t in_bytes,
                                            const uint64_t *d_in_off_len, size_t count, void *d_out, size_t out_cap,
                                            uint64_t *d_offsets, uint64_t *d_index, size_t index_cap,
                                            int32_t *d_status, size_t *out_len);

/* The block tables of records of any writer (d_out_off_len: the decoded lengths;
 * its offsets are not read).  Each record of two or more blocks is walked by one
 * wave inside its own compressed range; its preamble must equal its decoded
 * length (SNAPPY_AMD_ERR_HEADER).  d_status (may be NULL) gets 0 or the
 * record's failure: HEADER, TRUNCATED, OVERRUN, UNSUPPORTED as
 * snappy_amd_index_device reports them, and the range checks of the decode call.
 * A failing record's entries are undefined.  index_cap below the entries needed:
 * SNAPPY_AMD_ERR_CAPACITY.  Synchronises once (the plan's totals); the walk
 * itself is queued. */
int snappy_amd_records_index_device(snappy_amd_ctx *ctx, const void *d_comp, size_t comp_bytes,
                                    const uint64_t *d_comp_off_len, size_t count, const uint64_t *d_out_off_len,
                                    uint64_t *d_index, size_t index_cap, int32_t *d_status);

/* decompress_records_device for long records.  For every record the bytes and
 * the status are those of snappy_amd_index_device followed by
 * snappy_amd_decompress_device(SNAPPY_AMD_SINGLE) on the same compressed bytes:
 * elements may straddle blocks, copies may reach earlier blocks of the same
 * record (a second, ordered pass inside the record); a copy reaching before the
 * record's first output byte is SNAPPY_AMD_ERR_OFFSET.  The preamble must equal
 * out_len_i (SNAPPY_AMD_ERR_HEADER).  d_index = the tables (compress's, or
 * records_index_device's), or NULL: they are built in scratch, and an index
 * failure is the record's status with nothing of it decoded.  A table whose last
 * entry of a record is not its compressed length, or with another entry past
 * it, is SNAPPY_AMD_ERR_INDEX before any load; an entry moved off an element
 * boundary is SNAPPY_AMD_ERR_INDEX as in the SINGLE layout.  Checked before any
 * byte of a record is loaded or stored, with the short call's meanings:
 * out_len_i > SNAPPY_AMD_LONG_RECORD_MAX, a compressed range outside comp_bytes,
 * an output range outside out_bytes, an empty compressed range.  No read leaves
 * the record's compressed range (beyond the aligned dword holding its first
 * byte); a failing record may leave part of its own output range written, never
 * a byte outside it.  d_status, sync and the first failure as in the short
 * call; the call synchronises once in any case, for the plan's totals. */
int snappy_amd_decompress_long_records_device(snappy_amd_ctx *ctx, const void *d_comp, size_t comp_bytes,
                                              const uint64_t *d_comp_off_len, size_t count, void *d_out,
                                              size_t out_bytes, const uint64_t *d_out_off_len, const uint64_t *d_index,
                                              int32_t *d_status, int sync);

/* ---- range decode: bytes [start, start + length) through the block index --- */
/* Random access into a stream whose block index is known (compress_device's
 * d_offsets, the sidecar file, index_device): only the blocks a range touches are
 * decoded, and only their compressed bytes need to be in HBM.
 *
 * d_comp[0, comp_bytes) holds the stream's bytes [comp_origin, comp_origin +
 * comp_bytes): the resident window (comp_origin = 0 and the whole stream is the
 * plain case).  d_offsets is always the stream's full index, units + 1 entries
 * with stream-relative values in the format of snappy_amd_index_device; n, chunk
 * and layout as in decompress_device.  SINGLE: blocks of 65,536 bytes; the
 * preamble is checked only when block 0 is decoded, and must equal n.  STREAMS:
 * units of `chunk` bytes, each with its own preamble.
 *
 * Range i (host memory) writes the stream's decoded bytes [start, start + length)
 * to d_out[out_offset, out_offset + length).  Ranges may overlap in the stream;
 * overlapping output ranges are the caller's error; length == 0 is OK and touches
 * nothing.  The host plans (csrc/snappy_ranges.h): one decode unit per (range,
 * block) pair -- a block that several ranges share is decoded once per range.  A
 * unit that lies wholly inside its range decodes straight into d_out; an edge
 * unit decodes its whole block into a 65,536-byte staging slot in context scratch
 * and a second kernel copies the wanted part out.  At most 1,024 slots (64 MiB,
 * SNAPPY_RANGES_SLOT_CAP) are held: more edge units run in successive launches
 * that reuse them, so scratch stays within 64 MiB plus 32 bytes per planned unit
 * and 8 per range.  The call needs no read-back to size its launches: with sync =
 * 0 it returns once the work is queued.  A range decodes fastest when out_offset
 * and start agree mod 16 (16-byte stores).
 *
 * d_status (count i32, device; may be NULL) gets every range's status; a refused
 * or failing range does not disturb its neighbours; sync = 1 returns the first
 * failing range's status.  In this order, the first three before any byte of the
 * range is loaded or stored:
 *   ERR_ARG        the range leaves [0, n)
 *   ERR_CAPACITY   the output range leaves [0, out_bytes)
 *   ERR_TRUNCATED  one of the range's units has compressed bytes [entry[u],
 *                  entry[u+1]) that are not inside the resident window; if entry
 *                  u+1 carries skip bits, the bytes up to the end of the element
 *                  that straddles out count too
 *   ERR_DEPENDENT  SINGLE only: a unit of the range resumes a copy, or copies from
 *                  before its own block -- what pass 1 of the whole-stream decode
 *                  defers.  This call has no second pass: decode the stream whole.
 *   ERR_OFFSET     STREAMS: a copy reaches before its unit, as in decompress_device
 *   ERR_INDEX, ERR_HEADER, element errors: as the block decode reports them for
 *                  the units decoded; the lowest failing unit of the range wins.  A
 *                  corrupt block outside the ranges is never seen.
 * No byte of d_out outside the ranges is written (a failing range may leave part
 * of its own output range written); no read leaves the resident window, except
 * within the aligned dword that holds its first byte.
 *
 * What success proves: each decoded block's element chain ran from its entry
 * exactly to the next entry.  Unlike the whole-stream decode it does not prove
 * that the first entry of a range is a true element boundary -- the induction
 * from block 0 is missing -- so that entry is taken on the caller's word. */
#define SNAPPY_AMD_ERR_DEPENDENT (-13) /* a block of the range needs bytes of an earlier block */

typedef struct { uint64_t start, length, out_offset; } snappy_amd_range; /* host memory */

int snappy_amd_decompress_ranges_device(snappy_amd_ctx *ctx, const void *d_comp, uint64_t comp_origin,
                                        size_t comp_bytes, const uint64_t *d_offsets, size_t n, uint32_t chunk,
                                        int layout, const snappy_amd_range *ranges, size_t count, void *d_out,
                                        size_t out_bytes, int32_t *d_status, int sync);

/* Host forms: bytes [start, start + length) of snappy_decompress_buffer's output,
 * always exactly that slice.  idx = the sidecar file's bytes (or stream); NULL:
 * no sidecar -- the whole stream is uploaded and indexed on the GPU.  With a
 * sidecar: it is checked as in snappy_decompress_file_indexed, the stream's
 * preamble (its first bytes, at most 10) must equal the sidecar's N
 * (SNAPPY_AMD_ERR_INDEX), only the compressed bytes of the blocks the range
 * touches are read (fseeko in the FILE* form: a file_input that cannot seek is
 * SNAPPY_AMD_ERR_UNSUPPORTED) and uploaded, and only `length` bytes come back.  A
 * range that leaves [0, N) is SNAPPY_AMD_ERR_ARG.  Foreign streams whose range
 * is not self-contained (ERR_DEPENDENT, or skip bits on the range's first entry
 * or on the entry after its last block) are decoded whole and sliced; any other
 * failure with a sidecar loads the whole stream and is judged as in
 * snappy_decompress_file_indexed (ERR_INDEX: not this stream's index). */
int snappy_decompress_range_buffer(const uint8_t *in, size_t n, const uint8_t *idx, size_t idx_bytes, uint64_t start,
                                   size_t length, uint8_t *out, size_t cap, size_t *out_len);
int snappy_decompress_file_range(FILE *file_input, FILE *idx, uint64_t start, uint64_t length, FILE *file_out);

/* ---- Snappy framing format (framing_format.txt of google/snappy) -------- */
/* The file format other Snappy tools exchange: the 10-byte stream identifier
 * ff 06 00 00 "sNaPpY", then chunks -- a type byte, a 24-bit little-endian
 * length, and for data chunks the masked CRC-32C of the chunk's uncompressed
 * bytes in front of the payload.  A data chunk holds at most 65,536
 * uncompressed bytes, as its own raw Snappy stream (type 00) or stored (type
 * 01).  The compressor here cuts the input into chunks of `chunk` bytes
 * (1..65,536; 65,536 for the calls without that argument; the last one may be
 * shorter).  A compressed chunk's payload equals the SNAPPY_AMD_STREAMS unit of
 * that piece.  With SNAPPY_AMD_FRAME_STORE a chunk of R input bytes whose unit
 * has P bytes (preamble included) is written stored (type 01, 24-bit R + 4, the
 * CRC, the R bytes) iff P >= R - R / 8 (integer division): the payload is not
 * one eighth smaller than the bytes.  Without the flag every chunk is type 00.
 * The output is a pure function of (input, chunk, flags).  The
 * decoder takes what other writers emit: stored chunks, padding (fe) and
 * skippable (80..fd) chunks, repeated identifiers, data chunks of any
 * lengths.  Copies cannot reach outside their chunk (ERR_OFFSET).
 *
 * Chunk table (d_chunks, u64): entry i = byte position of data chunk i's
 * header in the stream, entry nchunks = the stream length.  Compress returns
 * it, decode takes it, frame_index_device builds it for a foreign stream.
 *
 * Errors of the framed decoders and walks.  Two stages, each reporting its
 * first failing chunk: every chunk's header is checked before anything is
 * decoded (ERR_HEADER, ERR_TRUNCATED, ERR_UNSUPPORTED, ERR_OVERRUN, ERR_INDEX,
 * then ERR_CAPACITY), so a malformed header in a later chunk is reported ahead
 * of an element or CRC error in an earlier one; among element and CRC errors
 * the first failing chunk wins, and a CRC is checked only where the chunk's
 * decode succeeded:
 *   ERR_HEADER       no or a wrong stream identifier, a later ff chunk that is
 *                    not the identifier, a data chunk shorter than its CRC,
 *                    an unreadable preamble in a compressed chunk
 *   ERR_TRUNCATED    a chunk (or its header) runs past the end
 *   ERR_UNSUPPORTED  a reserved unskippable chunk, types 02..7f
 *   ERR_OVERRUN      a data chunk that decodes to more than 65,536 bytes
 *   ERR_CAPACITY     output (or chunk table) too small; before any decode
 *   ERR_INDEX        a chunk table entry that is not a data chunk's header
 *   ERR_CHECKSUM     CRC mismatch;  element errors as the decoder reports them */
#define SNAPPY_AMD_FRAME_NO_IDENTIFIER 1u /* this buffer continues a framed stream */
#define SNAPPY_AMD_FRAME_STORE 2u   /* a chunk whose payload is not 1/8 smaller than its bytes is stored (type 01) */

/* CRC-32C (polynomial 0x82F63B78 reflected, init and xor-out ffffffff) of
 * `count` byte ranges of d_base: d_off_len holds (offset, length) pairs, any
 * alignment, d_crc gets one u32 each -- masked != 0: the framing format's
 * ((c >> 15) | (c << 17)) + 0xa282ead8.  Asynchronous on the context stream. */
int snappy_amd_crc32c_device(snappy_amd_ctx *ctx, const void *d_base, const uint64_t *d_off_len, size_t count,
                             int masked, uint32_t *d_crc);
/* Capacity d_out must have for compress_frame_device:
 * 10 + 8 ceil(n / 65536) + snappy_amd_max_output(n, 65536, SNAPPY_AMD_STREAMS). */
size_t snappy_amd_max_frame_output(size_t n);
/* Frame d_in[0..n): identifier (unless SNAPPY_AMD_FRAME_NO_IDENTIFIER), then
 * ceil(n / 65536) compressed chunks.  d_chunks receives ceil(n / 65536) + 1
 * entries.  n == 0 writes the identifier alone. */
int snappy_amd_compress_frame_device(snappy_amd_ctx *ctx, const void *d_in, size_t n, uint32_t flags, void *d_out,
                                     uint64_t *d_chunks, size_t *out_len);
/* The same with the chunk size and the store rule (above): chunk = input bytes
 * per data chunk, 1..65,536 (else ERR_ARG, and max_frame_output_ex returns 0);
 * flags = SNAPPY_AMD_FRAME_NO_IDENTIFIER | SNAPPY_AMD_FRAME_STORE (any other bit:
 * ERR_ARG).  compress_frame_device is chunk 65,536 and accepts NO_IDENTIFIER only.
 * Capacity: 10 + 8 ceil(n / chunk) + snappy_amd_max_output(n, chunk,
 * SNAPPY_AMD_STREAMS), whatever the flags (a stored chunk, 8 + R bytes, is never
 * larger than a compressed one's bound).  d_chunks receives ceil(n / chunk) + 1
 * entries; more than 2^31 - 1 chunks is ERR_ARG.  The flag adds no read-back:
 * with out_len == NULL the call is queued on the context stream and returns. */
size_t snappy_amd_max_frame_output_ex(size_t n, uint32_t chunk);
int snappy_amd_compress_frame_device_ex(snappy_amd_ctx *ctx, const void *d_in, size_t n, uint32_t chunk,
                                        uint32_t flags, void *d_out, uint64_t *d_chunks, size_t *out_len);
/* Walk a framed stream in HBM from its identifier: d_chunks (room for
 * max_chunks entries, the closing one included) gets the chunk table,
 * *nchunks_out the data chunks, *n_out the decoded bytes.  One wave follows
 * the headers, one dependent step per chunk.  The stream must begin with the
 * identifier: a continuation piece (SNAPPY_AMD_FRAME_NO_IDENTIFIER) is not
 * indexed on its own -- keep the table its compress call returned. */
int snappy_amd_frame_index_device(snappy_amd_ctx *ctx, const void *d_frame, size_t clen, uint64_t *d_chunks,
                                  size_t max_chunks, size_t *nchunks_out, size_t *n_out);
/* Decode the data chunks a chunk table names into d_out (cap bytes) and check
 * their CRCs; *n_out = decoded bytes.  Every table entry is checked against
 * clen; that the table is complete is the caller's word. */
int snappy_amd_decompress_frame_device(snappy_amd_ctx *ctx, const void *d_frame, size_t clen,
                                       const uint64_t *d_chunks, size_t nchunks, void *d_out, size_t cap,
                                       size_t *n_out);
/* (snappy_amd_last_timings covers the unframed calls only: the framed ones
 * record no events.) */
/* Host memory: out must hold snappy_amd_max_frame_output(n).  Inputs of more
 * than 64 MiB go piece by piece (SNAPPY_AMD_FRAME_PIECE_KB, a multiple of 64,
 * sets another piece size for the buffer and FILE* compressors and the FILE*
 * decoder's read buffer; the bytes written do not depend on it). */
int snappy_compress_frame_buffer(const uint8_t *in, size_t n, uint8_t *out, size_t cap, size_t *out_len);
/* With a chunk size and flags (SNAPPY_AMD_FRAME_STORE only: the host forms place
 * the identifier themselves): out must hold snappy_amd_max_frame_output_ex(n,
 * chunk).  A piece is the piece size rounded down to a multiple of chunk (at
 * least one chunk), so the bytes written do not depend on it.  The forms without
 * these arguments are (65536, 0). */
int snappy_compress_frame_buffer_ex(const uint8_t *in, size_t n, uint32_t chunk, uint32_t flags, uint8_t *out,
                                    size_t cap, size_t *out_len);
int snappy_decompress_frame_buffer(const uint8_t *in, size_t n, uint8_t *out, size_t cap, size_t *out_len);
/* Decoded bytes of a framed stream: the chunk walk on the host (no kernel),
 * the same rules as frame_index_device. */
int snappy_frame_uncompressed_length(const uint8_t *in, size_t n, uint64_t *len);
/* FILE* forms: file_input from its current position to EOF (input_size is
 * not needed: the format stores no total length). */
int snappy_compress_file_framed(FILE *file_input, unsigned long long input_size, FILE *file_compressed);
int snappy_compress_file_framed_ex(FILE *file_input, unsigned long long input_size, uint32_t chunk, uint32_t flags,
                                   FILE *file_compressed);
int snappy_decompress_file_framed(FILE *file_input, FILE *file_decompressed);

/* ---- range decode of a framed stream: seek table, CRC-checked slices ------ */
/* Random access into a framed stream.  Every data chunk is its own raw stream
 * of at most 65,536 bytes under its own CRC, so any chunk decodes alone
 * (ERR_DEPENDENT cannot happen) and a slice comes back verified.  Chunks may
 * have any decoded length, so a byte position is found by a search in the
 * stream's seek table: d_starts, nchunks + 1 u64 entries beside the chunk table,
 * entry i = the decoded position of data chunk i's first byte, entry nchunks =
 * the decoded length.
 *
 * frame_seek_device builds it from a chunk table: every entry's header is
 * checked as decompress_frame_device checks it (the same codes, the first
 * failing entry's), then the lengths are scanned.  *n_out = the decoded length.
 * compress_frame_device's own streams give starts[i] = min(65536 i, n)
 * (compress_frame_device_ex's: min(chunk i, n)).
 * snappy_frame_tables is the same on host memory, with no kernel: the chunk
 * walk of frame_index_device and both tables (room for max_chunks entries each,
 * the closing ones included; either may be NULL). */
int snappy_amd_frame_seek_device(snappy_amd_ctx *ctx, const void *d_frame, size_t clen, const uint64_t *d_chunks,
                                 size_t nchunks, uint64_t *d_starts, size_t *n_out);
int snappy_frame_tables(const uint8_t *in, size_t n, uint64_t *chunks, uint64_t *starts, size_t max_chunks,
                        size_t *nchunks_out, uint64_t *len);
/* d_window[0, comp_bytes) holds the stream's bytes [comp_origin, comp_origin +
 * comp_bytes): the resident window.  d_chunks and d_starts (device) may be any
 * contiguous sub-table, nchunks + 1 entries each, of the stream's tables:
 * positions and starts stay absolute.  Range i (host memory) writes the stream's
 * decoded bytes [start, start + length) to d_out[out_offset, out_offset + length);
 * length == 0 is OK and touches nothing.  The call is synchronous: the tables are
 * in HBM, so the plan (csrc/snappy_frame_ranges.h) runs there and 64 bytes are
 * read back to size the launches (a second read, of 8 bytes per launch group,
 * only with more edge units than staging slots).
 *
 * A range's span: its first chunk u0 is the last i with starts[i] <= start, its
 * last chunk u1 the last i with starts[i] <= start + length - 1, both by binary
 * search.  Every chunk u0..u1 is one decode unit; an empty chunk inside the span
 * is skipped (not read, no effect on the status).  A chunk that lies wholly
 * inside its range decodes straight into d_out; an edge chunk decodes whole into
 * a staging slot, is CRC-checked there, and its wanted part is copied out (the
 * staging rule of decompress_ranges_device: at most 1,024 slots, more edge units
 * in successive launches).  Scratch: 64 MiB at most, 76 bytes per unit, 72 per range.
 *
 * d_status (count i32, device; may be NULL) gets every range's status; the call
 * returns the first failing range's.  In this order:
 *   ERR_ARG        the range leaves [starts[0], starts[nchunks])
 *   ERR_CAPACITY   the output range leaves [0, out_bytes)
 *  (A seek table that is not sorted is not refused here: the search still gives
 *  u0 <= u1.  Its units are refused in the header stage, below.)
 *  then the header stage, over every non-empty unit before anything is decoded; a
 *  range with a failing unit decodes and stores nothing, and its status is its
 *  lowest failing unit's:
 *   ERR_TRUNCATED  the chunk's bytes [chunks[u], chunks[u] + 4 + len) are not all
 *                  inside the window
 *   ERR_HEADER, ERR_UNSUPPORTED, ERR_OVERRUN  the chunk's own header, as the
 *                  framed decoder reports it
 *   ERR_INDEX      the entry is not a data chunk; its decoded length is not
 *                  starts[u + 1] - starts[u]; it runs past chunks[u + 1]; or the
 *                  seek table contradicts itself about the unit, as one that is
 *                  not sorted does (a chunk of more than 65,536 bytes, one inside
 *                  the span that begins before the range or ends after it, an
 *                  empty first or last chunk)
 *  then the decode: element errors and ERR_CHECKSUM, the lowest failing chunk of
 *  the range; a CRC counts only where the chunk's decode succeeded.
 * Guarantees: no byte of d_out outside the accepted ranges' output is written,
 * whatever the tables say (a range that fails while it decodes may leave part of
 * its own output written); no read leaves the window, except within the aligned
 * dword that holds its first byte.  A range's status is what
 * decompress_frame_device returns for a stream made of the identifier and exactly
 * that range's non-empty chunks.  What success proves: each touched chunk agrees
 * with its own header and CRC.  It does not prove that the tables are the
 * stream's tables -- a table of another stream with the same chunk positions and
 * lengths passes -- that stays the caller's word, as in decompress_ranges_device. */
int snappy_amd_decompress_frame_ranges_device(snappy_amd_ctx *ctx, const void *d_window, uint64_t comp_origin,
                                              size_t comp_bytes, const uint64_t *d_chunks, const uint64_t *d_starts,
                                              size_t nchunks, const snappy_amd_range *ranges, size_t count,
                                              void *d_out, size_t out_bytes, int32_t *d_status);
/* Host forms: exactly bytes [start, start + length) of
 * snappy_decompress_frame_buffer's output, or SNAPPY_AMD_ERR_ARG for a range that
 * leaves it.  The buffer form walks the headers on the host and uploads only the
 * chunks of the span and their sub-tables.  The FILE* form hops from header to
 * header with 16-byte reads from the current position (no payload is read, and
 * the walk stops at the chunk holding the range's last byte: a damaged chunk
 * after it is never seen, one before it is the walk's error), then reads the
 * span's chunks with one seek and one read; a file_input that cannot seek is
 * SNAPPY_AMD_ERR_UNSUPPORTED. */
int snappy_decompress_frame_range_buffer(const uint8_t *in, size_t n, uint64_t start, size_t length, uint8_t *out,
                                         size_t cap, size_t *out_len);
int snappy_decompress_file_frame_range(FILE *file_input, uint64_t start, uint64_t length, FILE *file_out);

/* ---- Hadoop and snappy-java container streams ---------------------------- */
/* The two length-prefixed containers most Snappy files on disk are in: the
 * .snappy files of Hadoop's SnappyCodec (Hive, Spark) and the streams of
 * snappy-java's SnappyOutputStream (Spark shuffle blocks, Kafka message sets).
 * Big-endian 32-bit lengths in front of raw Snappy streams; no CRC, no chunk
 * types.  Neither is the framing format above.
 *
 * SNAPPY_AMD_CONTAINER_HADOOP: a sequence of blocks.  A block is BE32 raw_len,
 * then chunks BE32 comp_len | raw stream of comp_len bytes until the chunks'
 * decoded lengths add up to raw_len; raw_len 0 is a block without chunks.  No
 * file header, no trailer: 0 bytes are a valid empty stream.
 * SNAPPY_AMD_CONTAINER_XERIAL: the 16-byte header 82 53 4e 41 50 50 59 00, BE32
 * version, BE32 compatible_version (this library writes 1 and 1), then chunks
 * BE32 comp_len | raw stream.  The header may stand again at any chunk
 * boundary (concatenated streams): its first four bytes mark it.
 *
 * The compressor cuts the input into pieces of `block` bytes (0: the format's
 * default, 131,072 for Hadoop, 32,768 for snappy-java; at most 2^30), each
 * piece one chunk whose payload is exactly the bytes of snappy_compress() on
 * the piece (the record of compress_long_records_device); in Hadoop each chunk
 * is one block.  The output is a pure function of (input, block, format, flags).
 *
 * Chunk tables: two arrays of (offset, length) u64 pairs with one pair per
 * chunk -- d_comp_off_len the payloads' places in the container, d_out_off_len
 * their places in the decoded bytes -- the very arguments of
 * snappy_amd_decompress_long_records_device.
 *
 * Errors of the walks (container_index_device, the host walk, decode without
 * tables), the first failure in stream order:
 *   ERR_TRUNCATED    fewer than 4 bytes where a length stands, a chunk that runs
 *                    past the end, a snappy-java header cut short, a Hadoop
 *                    stream that ends inside a block
 *   ERR_HEADER       comp_len 0, a preamble that does not end inside the chunk's
 *                    first five bytes, an empty or wrongly begun snappy-java stream
 *   ERR_UNSUPPORTED  a chunk that declares more than 2^30 bytes,
 *                    compatible_version above 1 (version is not checked)
 *   ERR_OVERRUN      Hadoop: a chunk that declares more than its block has left
 * The decoders run in two stages: the walk (or the check of the caller's
 * tables against clen) reports its first failure, then ERR_CAPACITY, before
 * anything is decoded; then the chunks are decoded as one long-record batch and
 * the first failing chunk's status is returned with that call's meanings
 * (ERR_OFFSET: a copy reached before its chunk's first byte; ERR_HEADER: a
 * preamble that is not the table's length). */
#define SNAPPY_AMD_CONTAINER_HADOOP 0
#define SNAPPY_AMD_CONTAINER_XERIAL 1
#define SNAPPY_AMD_CONTAINER_NO_HEADER 1u /* snappy-java: this buffer continues a stream (no effect in Hadoop) */

/* Capacity d_out must have for compress_container_device: the stream header,
 * 8 (Hadoop) or 4 bytes per chunk and snappy_amd_max_long_records_output(n,
 * ceil(n / block)).  0 for an unknown format or a block above 2^30. */
size_t snappy_amd_max_container_output(size_t n, uint32_t block, int format);
/* Compress d_in[0..n) into one container.  d_comp_off_len / d_out_off_len
 * (chunks_cap pairs each; either may be NULL) get the chunk tables, *nchunks
 * ceil(n / block), *out_len the container's bytes.  n == 0 writes 0 bytes in
 * Hadoop and the header alone in snappy-java.  Checked before anything is
 * written: an unknown format, flag or block SNAPPY_AMD_ERR_ARG; out_cap below
 * snappy_amd_max_container_output, or (a table given) chunks_cap below
 * ceil(n / block), SNAPPY_AMD_ERR_CAPACITY.  The payloads are compressed into context scratch of
 * snappy_amd_max_long_records_output(n, chunks) bytes by the long-record call
 * and moved between their headers by one more pass.  No byte of d_out at or
 * past *out_len is written. */
int snappy_amd_compress_container_device(snappy_amd_ctx *ctx, const void *d_in, size_t n, uint32_t block, int format,
                                         uint32_t flags, void *d_out, size_t out_cap, uint64_t *d_comp_off_len,
                                         uint64_t *d_out_off_len, size_t chunks_cap, size_t *nchunks, size_t *out_len);
/* Walk a container in HBM: the chunk tables (room for max_chunks pairs each),
 * *nchunks and *n_out, the decoded bytes.  One wave follows the headers, one
 * dependent step per chunk.  A walk failure comes first; more chunks than
 * max_chunks is SNAPPY_AMD_ERR_CAPACITY, with *nchunks the pairs needed. */
int snappy_amd_container_index_device(snappy_amd_ctx *ctx, const void *d_cont, size_t clen, int format,
                                      uint64_t *d_comp_off_len, uint64_t *d_out_off_len, size_t max_chunks,
                                      size_t *nchunks, size_t *n_out);
/* Decode a container into d_out (cap bytes); *n_out = decoded bytes.  With both
 * tables NULL the call walks the container itself (nchunks is not read).  With
 * tables, every pair is checked against clen (a payload outside the container
 * ERR_TRUNCATED, an empty one ERR_HEADER, a length above 2^30 ERR_UNSUPPORTED),
 * *n_out is the end of the last output range, and that the tables are complete
 * is the caller's word. */
int snappy_amd_decompress_container_device(snappy_amd_ctx *ctx, const void *d_cont, size_t clen, int format,
                                           const uint64_t *d_comp_off_len, const uint64_t *d_out_off_len,
                                           size_t nchunks, void *d_out, size_t cap, size_t *n_out);
/* Host memory: out must hold snappy_amd_max_container_output(n, block, format).
 * Inputs of more than 64 MiB go piece by piece, a piece a multiple of the block
 * (the decoders cut at the last whole chunk and carry the rest, Hadoop's open
 * block included); SNAPPY_AMD_CONTAINER_PIECE_KB sets another piece size (the
 * bytes written do not depend on it).  The decoders walk on the host, by the
 * same rule as container_index_device, and upload the tables. */
int snappy_compress_container_buffer(const uint8_t *in, size_t n, uint32_t block, int format, uint8_t *out, size_t cap,
                                     size_t *out_len);
int snappy_decompress_container_buffer(const uint8_t *in, size_t n, int format, uint8_t *out, size_t cap,
                                       size_t *out_len);
/* Decoded bytes of a container: the walk on the host (no kernel). */
int snappy_container_uncompressed_length(const uint8_t *in, size_t n, int format, uint64_t *len);
/* FILE* forms: file_input from its current position to EOF. */
int snappy_compress_file_container(FILE *file_input, unsigned long long input_size, uint32_t block, int format,
                                   FILE *file_compressed);
int snappy_decompress_file_container(FILE *file_input, int format, FILE *file_decompressed);

/* ---- range decode of a container: through its chunk tables --------------- */
/* Random access into a Hadoop or snappy-java container.  Every chunk is one raw
 * stream of its own, so any chunk decodes alone (ERR_DEPENDENT cannot happen);
 * the chunk tables say where every payload is, so the format is not an argument.
 *
 * d_window[0, comp_bytes) holds the container's bytes [comp_origin, comp_origin +
 * comp_bytes): the resident window.  d_comp_off_len and d_out_off_len (device)
 * are nchunks pairs each: the chunk tables of container_index_device or
 * compress_container_device, or any contiguous run of their pairs; offsets stay
 * absolute.  The decoded extent they cover is [off[0], off[nchunks - 1] +
 * len[nchunks - 1]) of d_out_off_len.  Range i (host memory) writes the decoded
 * bytes [start, start + length) to d_out[out_offset, out_offset + length); length
 * == 0 is OK and touches nothing.  The call is synchronous: the tables are in HBM,
 * so the plan (csrc/snappy_container_ranges.h) runs there and 64 bytes are read
 * back to size this call's launches; the long-record decode underneath reads 64
 * bytes of its own per launch group, and a call whose edge chunks exceed the
 * staging budget reads 8 bytes per launch group once more.
 *
 * A range's span: its first chunk u0 is the last i with off[i] <= start, its last
 * chunk u1 the last i with off[i] <= start + length - 1, both by binary search
 * over d_out_off_len.  Every chunk u0..u1 is one decode unit, decoded whole as one
 * record of decompress_long_records_device (a chunk of more than 65,536 bytes gets
 * its block table from that call's per-record walk, and both decode passes run);
 * an empty chunk inside the span is skipped (not read, no effect on the status).
 * A chunk that lies wholly inside its range decodes straight into d_out; an edge
 * chunk (at most two per range) decodes whole into staging in context scratch and
 * its wanted part is copied out.  A chunk that several ranges share is decoded
 * once per range.
 *
 * Staging: the budget is 1,024 x 65,536 bytes (64 MiB; SNAPPY_AMD_RANGE_SLOTS x
 * 65,536 where that is set).  Edge chunks stand at 16-byte-aligned places, in plan
 * order; one that does not fit behind those before it opens the next launch
 * group, which reuses the area.  An edge chunk larger than the budget is a group
 * of its own.  Scratch: a call grows snappy_amd_device_bytes() by at most
 *   max(budget, the largest edge chunk rounded up to 16) + 16 of staging,
 *   + snappy_amd_max_long_records_scratch(T, U) for the derived batch of the
 *     largest launch group (T decoded bytes in U units; at most all units),
 *   + 68 bytes per unit and 100 per range, + 88,
 *   each of the three buffers with grow()'s slack: an eighth and a page.
 *
 * d_status (count i32, device; may be NULL) gets every range's status; the call
 * returns the first failing range's.  In this order:
 *   ERR_ARG        the range leaves the tables' decoded extent, or nchunks == 0
 *                  with length > 0
 *   ERR_CAPACITY   the output range leaves [0, out_bytes)
 *   ERR_INDEX      the search gives u1 < u0 (a table that is not sorted)
 *  then the table stage, over every non-empty unit before anything is decoded; a
 *  range with a failing unit decodes and stores nothing, and its status is its
 *  lowest failing chunk's, for each chunk the first of:
 *   ERR_TRUNCATED  the payload [comp_off, comp_off + comp_len) is not inside the
 *                  window
 *   ERR_HEADER     comp_len == 0
 *   ERR_UNSUPPORTED  a decoded length above 2^30
 *   ERR_INDEX      the tables contradict themselves about the unit: a chunk inside
 *                  the span that begins before the range or ends after it, or does
 *                  not end where the next one begins; an empty first or last chunk
 *   ERR_HEADER     a preamble that does not end inside the payload's first five
 *                  bytes, or is not the table's length
 *  then the decode: element errors of the long-record decode, the lowest failing
 *  chunk of the range.
 * Guarantees: no byte of d_out outside the accepted ranges' output is written,
 * whatever the tables say (a range that fails while it decodes may leave part of
 * its own output written); a refused or failing range never disturbs another; no
 * read leaves the window, except within the aligned dword that holds its first
 * byte.  For a sorted, contiguous table a range's status is what
 * decompress_container_device (tables given) returns for exactly that range's
 * non-empty chunks, when at most one of them fails (of two failing chunks this
 * call names the lower one; that call names a table failure before a decode
 * failure).  What success proves: each touched chunk agrees with its table
 * entries.  It does not prove that the tables are the container's -- that stays
 * the caller's word. */
int snappy_amd_decompress_container_ranges_device(snappy_amd_ctx *ctx, const void *d_window, uint64_t comp_origin,
                                                  size_t comp_bytes, const uint64_t *d_comp_off_len,
                                                  const uint64_t *d_out_off_len, size_t nchunks,
                                                  const snappy_amd_range *ranges, size_t count, void *d_out,
                                                  size_t out_bytes, int32_t *d_status);
/* The chunk tables of a container in host memory: the host walk, no kernel, the
 * same rules as container_index_device.  Room for max_chunks pairs each; either
 * table may be NULL.  *nchunks_out = the chunks, *len = the decoded bytes; more
 * chunks than max_chunks is SNAPPY_AMD_ERR_CAPACITY, with *nchunks_out the pairs
 * needed. */
int snappy_container_tables(const uint8_t *in, size_t n, int format, uint64_t *comp_off_len, uint64_t *out_off_len,
                            size_t max_chunks, size_t *nchunks_out, uint64_t *len);
/* Host forms: exactly bytes [start, start + length) of
 * snappy_decompress_container_buffer's output, or SNAPPY_AMD_ERR_ARG for a range
 * that leaves it.  Both hop from header to header with the walk's own step, 16
 * bytes per hop (the FILE* form with positional reads from the current position;
 * no payload beyond those bytes is read), carrying Hadoop's open block and the
 * owed snappy-java header, and stop at the chunk holding the range's last byte: a
 * damaged chunk after it is never seen, one before it is the walk's error, a
 * stream that ends first is checked as a whole stream's end and is then ERR_ARG.
 * The window [payload of u0, end of payload of u1) is then read with one seek and
 * one read and uploaded at its own address residue with the sub-tables.  A
 * file_input that cannot seek is SNAPPY_AMD_ERR_UNSUPPORTED. */
int snappy_decompress_container_range_buffer(const uint8_t *in, size_t n, int format, uint64_t start, size_t length,
                                             uint8_t *out, size_t cap, size_t *out_len);
int snappy_decompress_file_container_range(FILE *file_input, int format, uint64_t start, uint64_t length,
                                           FILE *file_out);

/* Kernel timing of the last compress/decompress call, measured with HIP
 * events on the launch stream: K1 (block compress), K3 (scan + gather),
 * K4 (block decode), milliseconds. */
int snappy_amd_last_timings(snappy_amd_ctx *ctx, float *k1_ms, float *k3_ms, float *k4_ms);
/* 1 = record the events above on every call (default 0). */
int snappy_amd_enable_timing(snappy_amd_ctx *ctx, int on);

#ifdef __cplusplus
}
#endif
#endif

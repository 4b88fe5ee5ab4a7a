/*
 * cmd.c -- `snappy [-c|-b|-d] [-r] infile outfile`, the CLI of the reference
 * (src/cmd.c:19-105: same flags, same last-two-argv file names, usage +
 * exit(1) on argc < 4), linked against the MI355X library instead of the CPU
 * codec.  -r prints sizes, ratio and MB/s (MB = 1e6 B, wall clock).
 * -i (an addition): with -c also write the sidecar block
 * index <outfile>.idx; with -d decode with <infile>.idx instead of the GPU
 * index pass.
 * -f (an addition): with -c write, with -d read the Snappy framing format
 * (framing_format.txt of google/snappy), the file format of other Snappy
 * tools; not with -b or -i.
 * -k bytes, -s (additions): with -c -f only.  -k gives the input bytes per data
 * chunk (1..65536; 65536 without it), the price of a small -R read; -s writes a
 * chunk whose compressed payload is not one eighth smaller than its bytes as a
 * stored chunk (type 01).
 * -F hadoop|xerial (an addition): with -c write, with -d read the container of
 * Hadoop's SnappyCodec (.snappy files) or of snappy-java's SnappyOutputStream;
 * not with -b, -i or -f.
 * -R start:length (an addition): with -d write only the decoded bytes [start,
 * start + length) of the stream.  With -i only the compressed bytes of the
 * blocks the range touches are read from infile (which must be seekable);
 * without -i the stream is read whole and indexed on the GPU.  With -f the
 * stream is a framed one: its chunk headers are read up to the range's last
 * chunk, then only the range's chunks (infile must be seekable).  Not with -c,
 * -b or -F.
 */
#include <errno.h>
#include <getopt.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

#include "snappy_amd.h"

static void usage(void)
{
    fprintf(stderr,
            "snappy [-c|-d|-b] [-r] [-i] [-f] [-k bytes] [-s] [-F format] [-R start:length] [infile] [outfile]\n"
            "-c compress (MI355X)\n"
            "-b compress with the BST matcher\n"
            "-d decompress (MI355X)\n"
            "-r print results\n"
            "-i -c: also write outfile.idx (block index); -d: use infile.idx\n"
            "-f with -c or -d: the Snappy framing format (chunks with CRC-32C)\n"
            "-k bytes with -c -f: input bytes per chunk, 1..65536 (default 65536)\n"
            "-s with -c -f: store chunks that do not compress by one eighth (type 01)\n"
            "-F hadoop|xerial with -c or -d: the Hadoop SnappyCodec / snappy-java container\n"
            "-R start:length with -d: only the decoded bytes [start, start + length) (-i: read only their blocks;\n"
            "   -f: of a framed stream, reading only their chunks)\n");
    exit(EXIT_FAILURE);
}

static FILE *open_or_die(const char *name, const char *mode)
{
    FILE *f = fopen(name, mode);
    if (!f) {
        fprintf(stderr, "cannot open %s: %s\n", name, strerror(errno));
        exit(EXIT_FAILURE);
    }
    return f;
}

static unsigned long long file_size(FILE *f)
{
    fseek(f, 0, SEEK_END);
    long s = ftell(f);
    fseek(f, 0, SEEK_SET);
    return s < 0 ? 0 : (unsigned long long)s;
}

int main(int argc, char *argv[])
{
    enum { M_COMPRESS, M_BST, M_DECOMPRESS } mode = M_COMPRESS;
    int show = 0, indexed = 0, framed = 0, container = -1, ranged = 0, compress_flag = 0, opt;
    unsigned long long r_start = 0, r_length = 0;
    int chunk_given = 0, store = 0;
    unsigned long chunk = SNAPPY_AMD_BLOCK;
    if (argc < 4) usage();
    while ((opt = getopt(argc, argv, "cbdrifk:sF:R:")) != -1) {
        if (opt == 'c') mode = M_COMPRESS, compress_flag = 1;
        else if (opt == 'b') mode = M_BST;
        else if (opt == 'd') mode = M_DECOMPRESS;
        else if (opt == 'r') show = 1;
        else if (opt == 'i') indexed = 1;
        else if (opt == 'f') framed = 1;
        else if (opt == 's') store = 1;
        else if (opt == 'k') {
            char *end = NULL;
            errno = 0;
            if (optarg[0] < '0' || optarg[0] > '9') usage();
            chunk = strtoul(optarg, &end, 10);
            if (errno || *end || chunk == 0 || chunk > SNAPPY_AMD_BLOCK) usage();
            chunk_given = 1;
        }
        else if (opt == 'F' && strcmp(optarg, "hadoop") == 0) container = SNAPPY_AMD_CONTAINER_HADOOP;
        else if (opt == 'F' && strcmp(optarg, "xerial") == 0) container = SNAPPY_AMD_CONTAINER_XERIAL;
        else if (opt == 'R') {
            /* two unsigned decimal numbers around one colon, nothing else */
            char *end = NULL;
            errno = 0;
            if (optarg[0] < '0' || optarg[0] > '9') usage();
            r_start = strtoull(optarg, &end, 10);
            if (errno || *end != ':' || end[1] < '0' || end[1] > '9') usage();
            r_length = strtoull(end + 1, &end, 10);
            if (errno || *end) usage();
            ranged = 1;
        }
        else usage();
    }
    if (indexed && mode == M_BST) usage();  /* -b writes no block index */
    if (framed && (indexed || mode == M_BST)) usage();  /* a framed stream has its chunk headers; -b is unframed */
    if (container >= 0 && (framed || indexed || mode == M_BST)) usage();  /* one file format at a time */
    if ((chunk_given || store) && !(framed && compress_flag && mode == M_COMPRESS)) usage();  /* -k, -s: the framed writer's */
    if (ranged && (mode != M_DECOMPRESS || compress_flag || container >= 0)) usage();  /* -R: a raw or framed stream's decode */
    const char *in_name = argv[argc - 2], *out_name = argv[argc - 1];
    FILE *in = open_or_die(in_name, "rb");
    FILE *out = open_or_die(out_name, "wb");
    unsigned long long in_size = file_size(in);
    FILE *idx = NULL;
    char name[4096] = "";
    if (indexed) {
        snprintf(name, sizeof(name), "%s.idx", mode == M_COMPRESS ? out_name : in_name);
        idx = open_or_die(name, mode == M_COMPRESS ? "wb" : "rb");
    }

    struct timespec t0, t1;
    clock_gettime(CLOCK_MONOTONIC, &t0);
    int rc = 0;
    if (container >= 0) {
        rc = mode == M_COMPRESS ? snappy_compress_file_container(in, in_size, 0, container, out)
                                : snappy_decompress_file_container(in, container, out);
    } else if (framed && ranged) {
        rc = snappy_decompress_file_frame_range(in, r_start, r_length, out);
        if (rc != 0) fprintf(stderr, "snappy_decompress_file_frame_range: error %d\n", rc);
    } else if (framed) {
        rc = mode == M_COMPRESS ? snappy_compress_file_framed_ex(in, in_size, (uint32_t)chunk,
                                                                 store ? SNAPPY_AMD_FRAME_STORE : 0u, out)
                                : snappy_decompress_file_framed(in, out);
    } else if (mode == M_COMPRESS && idx) {
        rc = snappy_compress_file_indexed(in, in_size, out, idx);
    } else if (mode == M_COMPRESS) {
        snappy_compress(in, in_size, out);
        rc = snappy_amd_last_status();
    } else if (mode == M_BST) {
        rc = snappy_compress_bst(in, in_size, out);
    } else if (ranged) {
        rc = snappy_decompress_file_range(in, idx, r_start, r_length, out);
        if (rc != 0) fprintf(stderr, "snappy_decompress_file_range: error %d\n", rc);
    } else if (idx) {
        rc = snappy_decompress_file_indexed(in, idx, out);
    } else {
        rc = snappy_decompress(in, out);
    }
    clock_gettime(CLOCK_MONOTONIC, &t1);
    fclose(in);
    fclose(out);
    if (idx) fclose(idx);
    if (rc != 0 && idx && mode == M_COMPRESS) remove(name);  /* no partial index left behind */
    double secs = (t1.tv_sec - t0.tv_sec) + 1e-9 * (t1.tv_nsec - t0.tv_nsec);
    if (show) {
        FILE *o = open_or_die(out_name, "rb");
        unsigned long long out_size = file_size(o);
        fclose(o);
        unsigned long long raw = mode == M_DECOMPRESS ? out_size : in_size;
        printf("input %llu bytes, output %llu bytes\n", in_size, out_size);
        if (mode != M_DECOMPRESS && out_size) printf("ratio %f\n", (double)in_size / (double)out_size);
        printf("%f s, %f MB/s (uncompressed bytes)\n", secs, secs > 0 ? raw / (secs * 1e6) : 0.0);
    }
    return rc == 0 ? 0 : 1;
}

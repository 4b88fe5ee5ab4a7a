/*
 * container_walk_check.c -- the shared walk rule of the Hadoop / snappy-java
 * containers (csrc/snappy_container.h) as plain C, meant to be built with
 * -fsanitize=address,undefined and run on its own
 * (test_container_walk_check.py).
 *
 * argv[1] names a file of containers: u32 count, then per container u32 length
 * and its bytes (little-endian).  For every container and both formats the
 * program walks every prefix, then every container with one byte changed (the
 * first `argv[2]` bytes, four changes each), each input in a malloc block of
 * exactly its size, and prints one line per walk: status, chunks, decoded bytes.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "snappy_container.h"

static void walk(const uint8_t *in, size_t n, int format)
{
    /* an exactly sized block: a read past the input is a heap overflow */
    uint8_t *b = (uint8_t *)malloc(n ? n : 1);
    if (!b) exit(2);
    memcpy(b, in, n);
    size_t pos = 0;
    uint64_t R = 0, total = 0, chunks = 0;
    int first = format == SNAPPY_AMD_CONTAINER_XERIAL, st = SNAPPY_AMD_OK;
    while (pos < n) {
        uint32_t x[4], coff, clen, dlen;
        uint64_t adv;
        snappy_container_window(b + pos, n - pos, x);
        const int r = snappy_container_step(x, n - pos, format, first, &R, &coff, &clen, &dlen, &adv);
        if (r < 0) {
            st = r;
            break;
        }
        first = 0;
        if (r == 1) {
            /* the payload the step names lies inside the input */
            if (pos + coff + clen > n || coff + clen != adv) exit(3);
            chunks++;
            total += dlen;
        }
        if (adv == 0) exit(4);
        pos += (size_t)adv;
    }
    if (st == SNAPPY_AMD_OK) st = snappy_container_end(format, first, R);
    printf("%d %llu %llu\n", st, (unsigned long long)chunks, (unsigned long long)total);
    free(b);
}

int main(int argc, char **argv)
{
    if (argc < 3) return 1;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 1;
    const size_t head = (size_t)atol(argv[2]);
    uint32_t count = 0;
    if (fread(&count, 4, 1, f) != 1) return 1;
    static const uint8_t flips[4] = {0x01, 0x80, 0xFF, 0x00};  /* xor masks; 00: set the byte to zero */
    for (uint32_t c = 0; c < count; c++) {
        uint32_t len = 0;
        if (fread(&len, 4, 1, f) != 1) return 1;
        uint8_t *s = (uint8_t *)malloc(len ? len : 1);
        if (!s || (len && fread(s, 1, len, f) != len)) return 1;
        for (int format = 0; format < 2; format++) {
            for (size_t i = 0; i <= len; i++) walk(s, i, format);
            for (size_t i = 0; i < len && i < head; i++) {
                for (int k = 0; k < 4; k++) {
                    const uint8_t keep = s[i];
                    s[i] = flips[k] ? (uint8_t)(keep ^ flips[k]) : 0;
                    walk(s, len, format);
                    s[i] = keep;
                }
            }
        }
        free(s);
    }
    fclose(f);
    return 0;
}

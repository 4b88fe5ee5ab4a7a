/* container_ranges_plan_check.c -- the plan rule of range decode over a container
 * (csrc/snappy_container_ranges.h) as plain C in a stand-alone program, for
 * tests/test_container_ranges_plan_check.py to build with AddressSanitizer and
 * UBSan.  Reads cases from a file -- u64 out_bytes, u64 budget, u32 nchunks, u32
 * count, u32 checks, then nchunks x (u64 offset, length) output pairs, count x (u64
 * start, length, out_offset) and checks x (5 payload bytes, u64 co, cl, w0, w1,
 * size, u32 hi) -- plans each one into exactly sized heap blocks (a counting call,
 * then the filling call; the table in a block of exactly nchunks pairs), packs the
 * edge units and prints what the rule says, one line per case header, range,
 * unit, staged unit and table check, for the test to compare with its Python
 * model. */
#include <inttypes.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "snappy_container_ranges.h"

static int rd(FILE *f, void *p, size_t n) { return fread(p, 1, n, f) == n; }

int main(int argc, char **argv)
{
    if (argc != 2) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    uint32_t cases;
    if (!rd(f, &cases, 4)) return 2;
    for (uint32_t c = 0; c < cases; c++) {
        uint64_t out_bytes, budget;
        uint32_t nchunks, count, checks;
        if (!rd(f, &out_bytes, 8) || !rd(f, &budget, 8) || !rd(f, &nchunks, 4) || !rd(f, &count, 4) || !rd(f, &checks, 4))
            return 2;
        /* (no chunks, no ranges: one byte, so the pointers are real and any access is caught) */
        uint64_t *outp = (uint64_t *)malloc(nchunks ? (size_t)nchunks * 2 * sizeof *outp : 1);
        snappy_amd_range *ranges = (snappy_amd_range *)malloc(count ? count * sizeof *ranges : 1);
        int32_t *status = (int32_t *)malloc(count ? count * sizeof *status : 1);
        if (!outp || !ranges || !status) return 2;
        if (nchunks && !rd(f, outp, (size_t)nchunks * 2 * sizeof *outp)) return 2;
        if (count && !rd(f, ranges, count * sizeof *ranges)) return 2;
        uint64_t nu = 0, ne = 0, nu2 = 0, ne2 = 0;
        int rc = snappy_container_ranges_plan(outp, nchunks, ranges, count, out_bytes, status, NULL, 0, &nu, &ne);
        if (rc != 0) return 3;
        snappy_range_unit *units = (snappy_range_unit *)malloc(nu ? (size_t)nu * sizeof *units : 1);
        if (!units) return 2;
        /* one entry short: the rule must say so and stay inside the block */
        if (nu) {
            snappy_range_unit *few = (snappy_range_unit *)malloc(nu > 1 ? (size_t)(nu - 1) * sizeof *few : 1);
            if (!few) return 2;
            if (snappy_container_ranges_plan(outp, nchunks, ranges, count, out_bytes, status, few, (size_t)(nu - 1), &nu2,
                                             &ne2) != SNAPPY_AMD_ERR_CAPACITY || nu2 != nu || ne2 != ne)
                return 3;
            free(few);
        }
        rc = snappy_container_ranges_plan(outp, nchunks, ranges, count, out_bytes, status, units, (size_t)nu, &nu2, &ne2);
        if (rc != 0 || nu2 != nu || ne2 != ne) return 3;
        printf("case %" PRIu64 " %" PRIu64 "\n", nu, ne);
        for (uint32_t i = 0; i < count; i++) printf("r %d\n", status[i]);
        for (uint64_t k = 0; k < nu; k++)
            printf("u %" PRIu64 " %" PRIu64 " %u %u %u %u\n", units[k].unit, units[k].land, units[k].range, units[k].lo,
                   units[k].hi, units[k].edge);
        /* the packing of the edge units, in plan order: "s <unit index> <place> <opened a group>" */
        uint64_t fill = 0, stage = 0;
        for (uint64_t k = 0; k < nu; k++) {
            if (!units[k].edge) continue;
            uint64_t place;
            const int opened = snappy_container_pack(budget, snappy_container_stage_size(outp[2 * units[k].unit + 1]),
                                                     &fill, &place);
            if (fill > stage) stage = fill;
            printf("s %" PRIu64 " %" PRIu64 " %d\n", k, place, opened);
        }
        printf("stage %" PRIu64 "\n", stage);
        for (uint32_t k = 0; k < checks; k++) {
            uint8_t *w = (uint8_t *)malloc(5);
            uint64_t v[5];
            uint32_t hi;
            if (!w || !rd(f, w, 5) || !rd(f, v, sizeof v) || !rd(f, &hi, 4)) return 2;
            printf("k %d\n", snappy_container_unit_check(w, v[0], v[1], v[2], v[3], v[4], hi));
            free(w);
        }
        free(units);
        free(status);
        free(ranges);
        free(outp);
    }
    fclose(f);
    return 0;
}

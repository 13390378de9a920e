/* copy_host_loop.c -- the one-core yardstick of tools/bench_copy_items.py: the
 * rescue copy of storage.c:1004-1006 with the check a caller could add on the
 * host, memcpy + crc32c() per image, over one wbuf of packed equal images.
 *
 * Usage: copy_host_loop <wbuf bytes> <image bytes> <images> <repeats>
 * Prints the median time of one pass over the wbuf in microseconds.
 */
#define _GNU_SOURCE
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

#include "crc32c.h"

static int cmp(const void *a, const void *b) {
    const double x = *(const double *)a, y = *(const double *)b;
    return (x > y) - (x < y);
}

int main(int argc, char **argv) {
    if (argc != 5) return 2;
    const size_t wbuf = strtoull(argv[1], NULL, 0), nt = strtoull(argv[2], NULL, 0), n = strtoull(argv[3], NULL, 0);
    const int reps = atoi(argv[4]);
    if (nt < 50 || n * nt > wbuf || reps < 1 || reps > 1000) return 2;
    crc32c_init();
    uint8_t *src = malloc(wbuf), *dst = malloc(wbuf);
    double *us = malloc(sizeof(double) * (size_t)reps);
    if (!src || !dst || !us) return 1;
    uint64_t s = 99;
    for (size_t i = 0; i < wbuf; ++i) src[i] = (uint8_t)((s = s * 6364136223846793005ull + 1442695040888963407ull) >> 56);
    for (size_t i = 0; i < n; ++i) {  /* every image carries its CRC */
        const uint32_t c = crc32c(0, src + i * nt + 32, nt - 32);
        memcpy(src + i * nt + 28, &c, 4);
    }
    size_t bad = 0;
    for (int r = -2; r < reps; ++r) {  /* two warm-up passes */
        struct timespec t0, t1;
        clock_gettime(CLOCK_MONOTONIC, &t0);
        for (size_t i = 0; i < n; ++i) {
            const uint8_t *im = src + i * nt;
            uint32_t stored;
            memcpy(dst + i * nt, im, nt);
            memcpy(&stored, im + 28, 4);
            bad += crc32c(0, im + 32, nt - 32) != stored;
        }
        clock_gettime(CLOCK_MONOTONIC, &t1);
        if (r >= 0) us[r] = (t1.tv_sec - t0.tv_sec) * 1e6 + (t1.tv_nsec - t0.tv_nsec) * 1e-3;
    }
    qsort(us, (size_t)reps, sizeof(double), cmp);
    printf("%.2f\n", bad ? -1.0 : us[reps / 2]);
    return bad ? 1 : 0;
}

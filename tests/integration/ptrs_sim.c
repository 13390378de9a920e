/* ptrs_sim.c -- the proxy's read path through crc32c_ptrs_submit.
 *
 * Shape (proxy_internal.c:16-60, :91): every read gets a buffer of its own,
 * malloc(ntotal), the IO thread preads the item image into it and the callback
 * checks crc32c(0, buf + 32, ntotal - 32) against the stored exptime.  No arena
 * holds these buffers, so the batch of one IO thread is a list of pointers.
 * Each thread here mallocs `depth` buffers per batch, fills each with an item
 * image (some torn on purpose: one flipped byte), submits the spans as one
 * pointer job, waits, and compares every CRC with the scalar crc32c() and with
 * exptime.  Two legs:
 *   malloc      the buffers as malloc returns them: pageable, the job runs
 *               alone and its spans are packed;
 *   registered  the buffers carved from a 1 MiB page per thread that the
 *               thread registered once (slabs.c:613-616 mallocs slab pages one
 *               by one: register each there): the jobs of all threads share
 *               launches.
 *
 * Usage: ptrs_sim [--gpu] [threads] [batches_per_thread] [depth]
 * Without --gpu the submit must fail with CRC32C_ENODEV (no CPU fallback).
 * Output: one line of counts per leg; exit status 0 = every check passed.
 */
#define _GNU_SOURCE
#include <pthread.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "crc32c.h"
#include "crc32c_batch.h"

#define ITEM_CAS 2u
#define MAX_DEPTH 64
#define MAX_VAL 16384
#define MAX_IMG (48 + 16 + 8 + MAX_VAL + 2)
#define PAGE_BYTES (1u << 20)

static uint64_t mix(uint64_t *s) { /* splitmix64 */
    uint64_t z = (*s += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}

static uint32_t image_bytes(uint32_t id, uint32_t vlen) {
    char key[16];
    return 48 + (uint32_t)snprintf(key, sizeof key, "key%07u", id) + 1 + vlen + 2 + 8;
}

static void make_item(uint8_t *dst, uint32_t id, uint32_t vlen, uint64_t *rng) {
    char key[16];
    const int nkey = snprintf(key, sizeof key, "key%07u", id);
    const uint32_t nbytes = vlen + 2, ntotal = 48 + nkey + 1 + nbytes + 8;
    uint16_t refcount = 1, flags = ITEM_CAS;
    memset(dst, 0, 48);
    memcpy(dst + 32, &nbytes, 4);
    memcpy(dst + 36, &refcount, 2);
    memcpy(dst + 38, &flags, 2);
    dst[40] = 1;
    dst[41] = (uint8_t)nkey;
    const uint64_t cas = id + 1;
    memcpy(dst + 48, &cas, 8);
    memcpy(dst + 56, key, nkey + 1);
    uint8_t *v = dst + 56 + nkey + 1;
    for (uint32_t i = 0; i < vlen; i += 8) {
        const uint64_t r = mix(rng);
        memcpy(v + i, &r, vlen - i < 8 ? vlen - i : 8);
    }
    v[vlen] = '\r';
    v[vlen + 1] = '\n';
    const uint32_t crc = crc32c(0, dst + 32, ntotal - 32); /* the spill CRC (storage.c:567) */
    memcpy(dst + 28, &crc, 4);
}

struct worker {
    pthread_t tid;
    int id, batches, depth, registered;
    uint8_t *page; /* registered leg: this thread's 1 MiB page */
    uint64_t reads, mismatches, torn, detected, false_bad, rc_fail;
};

static void *io_thread(void *arg) {
    struct worker *w = arg;
    uint64_t rng = 0x7654321ull + (uint64_t)w->id * 0x9e3779b97f4a7c15ull + (uint64_t)w->registered;
    uint8_t *buf[MAX_DEPTH];
    const void *ptrs[MAX_DEPTH];
    uint32_t lens[MAX_DEPTH], out[MAX_DEPTH], stored[MAX_DEPTH];
    int torn[MAX_DEPTH];
    for (int r = 0; r < w->batches; ++r) {
        uint32_t used = 0;
        for (int k = 0; k < w->depth; ++k) { /* one read: its buffer, then the pread */
            const uint32_t id = (uint32_t)(mix(&rng) % 1000000), vlen = (uint32_t)(mix(&rng) % (MAX_VAL + 1));
            const uint32_t nt = image_bytes(id, vlen);
            if (w->registered) {
                buf[k] = w->page + used + mix(&rng) % 16; /* (slab chunks need no alignment here) */
                used += (nt + 31) & ~15u;
            } else {
                buf[k] = malloc(nt);
                if (!buf[k]) {
                    w->rc_fail++;
                    return NULL;
                }
            }
            make_item(buf[k], id, vlen, &rng);
            memcpy(&stored[k], buf[k] + 28, 4);
            torn[k] = mix(&rng) % 53 == 0;
            if (torn[k]) buf[k][32 + mix(&rng) % (nt - 32)] ^= 0x40;
            ptrs[k] = buf[k] + 32;
            lens[k] = nt - 32;
            out[k] = 0xdeadbeefu;
        }
        crc32c_ptr_batch b = {ptrs, lens, 0, NULL, out, (uint64_t)w->depth};
        crc32c_job_t job;
        int rc = crc32c_ptrs_submit(&b, NULL, &job);
        if (!rc) rc = crc32c_batch_wait(job);
        if (rc) w->rc_fail++;
        for (int k = 0; k < w->depth && !rc; ++k) {
            w->reads++;
            if (out[k] != crc32c(0, ptrs[k], lens[k])) w->mismatches++;
            const int bad = out[k] != stored[k]; /* the callback's compare (storage.c:172-178) */
            w->torn += torn[k];
            w->detected += torn[k] && bad;
            w->false_bad += !torn[k] && bad;
        }
        if (!w->registered)
            for (int k = 0; k < w->depth; ++k) free(buf[k]);
    }
    return NULL;
}

static int run_leg(int registered, int threads, int batches, int depth) {
    struct worker *ws = calloc(threads, sizeof *ws);
    uint64_t l0, s0, j0, o0, l1, s1, j1, o1;
    int failed = 0;
    if (crc32c_queue_stats(&l0, &s0, &j0, &o0)) return 1;
    for (int t = 0; t < threads; ++t) {
        ws[t].id = t;
        ws[t].batches = batches;
        ws[t].depth = depth;
        ws[t].registered = registered;
        if (registered) {
            if (posix_memalign((void **)&ws[t].page, 4096, PAGE_BYTES)) return 1;
            memset(ws[t].page, 0, PAGE_BYTES);
            if (crc32c_host_register(ws[t].page, PAGE_BYTES)) return 1;
        }
    }
    for (int t = 0; t < threads; ++t) pthread_create(&ws[t].tid, NULL, io_thread, &ws[t]);
    struct worker sum = {0};
    for (int t = 0; t < threads; ++t) {
        pthread_join(ws[t].tid, NULL);
        sum.reads += ws[t].reads;
        sum.mismatches += ws[t].mismatches;
        sum.torn += ws[t].torn;
        sum.detected += ws[t].detected;
        sum.false_bad += ws[t].false_bad;
        sum.rc_fail += ws[t].rc_fail;
        if (registered) {
            failed |= crc32c_host_unregister(ws[t].page) != CRC32C_OK;
            free(ws[t].page);
        }
    }
    free(ws);
    if (crc32c_queue_stats(&l1, &s1, &j1, &o1)) return 1;
    const uint64_t want = (uint64_t)threads * batches * depth, njobs = (uint64_t)threads * batches;
    printf("leg=%s reads=%llu mismatches=%llu torn=%llu detected=%llu false_bad=%llu rc_fail=%llu launches=%llu "
           "coalesced_jobs=%llu solo_jobs=%llu\n",
           registered ? "registered" : "malloc", (unsigned long long)sum.reads, (unsigned long long)sum.mismatches,
           (unsigned long long)sum.torn, (unsigned long long)sum.detected, (unsigned long long)sum.false_bad,
           (unsigned long long)sum.rc_fail, (unsigned long long)(l1 - l0), (unsigned long long)(j1 - j0),
           (unsigned long long)(o1 - o0));
    failed |= sum.reads != want || sum.mismatches || sum.false_bad || sum.rc_fail || sum.detected != sum.torn;
    /* pageable buffers run alone, registered ones share launches */
    failed |= registered ? (j1 - j0 != njobs || o1 != o0 || l1 - l0 > njobs) : (o1 - o0 != njobs || j1 != j0);
    return failed;
}

int main(int argc, char **argv) {
    int gpu = 0, a = 1;
    if (a < argc && !strcmp(argv[a], "--gpu")) gpu = 1, ++a;
    const int threads = a < argc ? atoi(argv[a++]) : 8;
    const int batches = a < argc ? atoi(argv[a++]) : 100;
    const int depth = a < argc ? atoi(argv[a++]) : 4;
    if (threads < 1 || batches < 1 || depth < 1 || depth > MAX_DEPTH ||
        (uint64_t)depth * (MAX_IMG + 48) > PAGE_BYTES)
        return 2;
    crc32c_init();
    if (!gpu) {
        uint8_t img[256];
        uint64_t rng = 1;
        make_item(img, 1, 100, &rng);
        const void *p = img + 32;
        uint32_t out = 9;
        crc32c_ptr_batch b = {&p, NULL, image_bytes(1, 100) - 32, NULL, &out, 1};
        crc32c_job_t job = NULL;
        const int rc = crc32c_ptrs_submit(&b, NULL, &job);
        printf("crc32c_ptrs_submit without a GPU: %s\n", crc32c_strerror(rc));
        return rc == CRC32C_ENODEV && out == 9 && job == NULL ? 0 : 1;
    }
    if (crc32c_gpu_count() < 1) {
        fprintf(stderr, "ptrs_sim --gpu: no gfx950 device\n");
        return 1;
    }
    const int bad = run_leg(0, threads, batches, depth) | run_leg(1, threads, batches, depth);
    printf(bad ? "ptrs_sim FAILED\n" : "ptrs_sim ok\n");
    return bad;
}

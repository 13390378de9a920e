/* recover_sim.c -- storage_compact_readback over a page with damaged headers
 * through crc32c_recover_pages: salvage_sim.c's
 * page, damage and rescue check, with the walk, its verify and the salvage in
 * one library call and one rescue loop over the merged list.
 *
 * The flow.  crc32c_recover_pages returns every image of the page that the
 * walk reached or the salvage proved, ascending by offset, with its kind and
 * its ITEM_ntotal.  The loop skips kind 0 (reached, but not sane or its CRC
 * does not match), hands every other entry to the rescue check of
 * storage.c:964-975 and takes the image's size from lens[] instead of parsing
 * the header again.  Only the images whose own header was damaged stay lost.
 *
 * The run: as salvage_sim.c (the same generator and seed, so the same page and
 * the same damage): a page of 8 wbufs of stamped images, a key -> offset table
 * as the hash table, two fifths of the items live, one header bit flipped in
 * every 37th live image "on flash".
 *
 * Usage: recover_sim [--gpu]
 * Prints live=<l> reached=<r> salvaged=<s> lost=<x> damaged=<d> as salvage_sim
 * does: reached = live images with an undamaged header that the walk arrived
 * at (kind 1), salvaged = those the salvage added (kind CRC32C_ITEM_SALVAGED),
 * lost = live - reached - salvaged.  Exit status 0 = the run itself worked;
 * the caller judges the counts.
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "crc32c.h"
#include "crc32c_batch.h"

#define WBUF (1u << 20)
#define NWBUF 8u
#define PAGE (NWBUF * WBUF)
#define MAX_ITEMS 8000u
#define ITEM_CAS 2u
#define MAX_VALUE 3000u
#define MAX_IMG (48 + 16 + 8 + MAX_VALUE + 2)
#define GONE UINT64_MAX

static uint32_t rd32(const uint8_t *p) { uint32_t v; memcpy(&v, p, 4); return v; }

static uint64_t ntotal_of(const uint8_t *p) {
    uint16_t flags;
    memcpy(&flags, p + 38, 2);
    return 48ull + p[41] + 1 + rd32(p + 32) + ((flags & 256u) ? 4 : 0) + ((flags & ITEM_CAS) ? 8 : 0);
}

static uint64_t mix(uint64_t *s) {
    uint64_t z = (*s += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}

/* an item image as storage_write leaves it, CRC stored (storage.c:567) */
static uint32_t make_image(uint8_t *img, uint32_t id, uint64_t *rng) {
    char key[16];
    const int nkey = snprintf(key, sizeof key, "key%07u", id);
    const uint32_t vlen = (uint32_t)(mix(rng) % MAX_VALUE), nbytes = vlen + 2;
    const uint32_t nt = 48 + (uint32_t)nkey + 1 + nbytes + 8;
    const uint16_t refc = 1, flags = ITEM_CAS | 1u /* ITEM_LINKED */;
    const uint64_t cas = id + 1;
    memset(img, 0, 48);
    memcpy(img + 32, &nbytes, 4);
    memcpy(img + 36, &refc, 2);
    memcpy(img + 38, &flags, 2);
    img[40] = 17;
    img[41] = (uint8_t)nkey;
    memcpy(img + 48, &cas, 8);
    memcpy(img + 56, key, (size_t)nkey + 1);
    uint8_t *v = img + 56 + nkey + 1;
    for (uint32_t i = 0; i < vlen; ++i) v[i] = (uint8_t)mix(rng);
    v[vlen] = '\r';
    v[vlen + 1] = '\n';
    const uint32_t crc = crc32c(0, img + 32, nt - 32);
    memcpy(img + 28, &crc, 4);
    return nt;
}

static uint64_t where[MAX_ITEMS]; /* the hash table: page offset of each live item's image, or GONE */
static uint8_t damaged[MAX_ITEMS], rescued[MAX_ITEMS];
static uint32_t nitems;

/* storage.c:964-975: the image's key, looked up, must be linked to exactly
 * this offset (`room`: the image's bytes, lens[] of the merged list) */
static int rescue(const uint8_t *page, uint64_t off, uint64_t room) {
    const uint8_t *im = page + off;
    uint16_t flags;
    memcpy(&flags, im + 38, 2);
    const uint32_t nkey = im[41], koff = 48 + ((flags & ITEM_CAS) ? 8 : 0);
    char key[16];
    if (nkey != 10 || koff + nkey > room) return 0;
    memcpy(key, im + koff, nkey);
    key[nkey] = 0;
    if (strncmp(key, "key", 3) != 0) return 0;
    char *end = NULL;
    const unsigned long id = strtoul(key + 3, &end, 10);
    if (*end || id >= nitems || where[id] != off || rescued[id]) return 0;
    rescued[id] = 1;
    return 1;
}

int main(int argc, char **argv) {
    int gpu = 0;
    for (int i = 1; i < argc; ++i)
        if (!strcmp(argv[i], "--gpu")) gpu = 1;
    crc32c_init();
    if (!gpu) {
        uint8_t buf[64] = {0};
        uint64_t offs[1] = {9}, n = 9, nbad = 9, nsalvaged = 9;
        uint32_t lens[1] = {9};
        uint8_t kind[1] = {9};
        const int rc = crc32c_recover_pages(buf, sizeof buf, 64, offs, lens, kind, 1, &n, &nbad, &nsalvaged, NULL, NULL,
                                            0, NULL);
        printf("recover_sim: no GPU, recover reports %s\n", crc32c_strerror(rc));
        return rc == CRC32C_ENODEV && offs[0] == 9 && lens[0] == 9 && kind[0] == 9 && n == 9 && nbad == 9 &&
                       nsalvaged == 9
                   ? 0
                   : 1;
    }
    uint8_t *page = calloc(PAGE, 1);
    static uint8_t img[MAX_IMG];
    if (!page) return 1;
    int failures = 0;
    uint64_t rng = 41;

    /* fill the page through wbufs: an image never crosses one, tails stay zero */
    uint64_t used = 0;
    for (;; ++nitems) {
        const uint32_t nt = make_image(img, nitems, &rng);
        if (used % WBUF + nt > WBUF) used = (used / WBUF + 1) * WBUF;
        if (used >= PAGE) break;
        if (nitems >= MAX_ITEMS) {
            fprintf(stderr, "item table too small\n");
            return 1;
        }
        memcpy(page + used, img, nt);
        where[nitems] = used;
        used += nt;
    }

    /* the live set, and the damage "on flash": one header bit of every 37th live image */
    uint64_t live = 0, ndamaged = 0;
    for (uint32_t id = 0; id < nitems; ++id) {
        if (mix(&rng) % 5 >= 2) {
            where[id] = GONE;
            continue;
        }
        if (live++ % 37 == 11) {
            uint8_t *im = page + where[id];
            switch (ndamaged % 3) {
                case 0: im[41] = 0; break;                                   /* nkey: ends the walk */
                case 1: im[32 + mix(&rng) % 2] ^= (uint8_t)(1u << (mix(&rng) % 8)); break; /* nbytes */
                default: im[38] ^= ITEM_CAS; break;                          /* it_flags */
            }
            damaged[id] = 1;
            ++ndamaged;
        }
    }

    uint64_t reached = 0, salvaged = 0;
    const uint64_t cap = 2 * (PAGE / 50) + NWBUF; /* the walk's bound and the salvage's, together */
    uint64_t *offs = malloc(cap * 8);
    uint32_t *lens = malloc(cap * 4);
    uint8_t *kind = malloc(cap);
    uint64_t n = 0, nbad = 0, nsalvaged = 0, scanned = 0, ncand = 0;
    if (!offs || !lens || !kind) return 1;
    const int rc = crc32c_recover_pages(page, PAGE, WBUF, offs, lens, kind, cap, &n, &nbad, &nsalvaged, &scanned,
                                        &ncand, 0, NULL);
    if (rc != CRC32C_OK || n > cap) {
        fprintf(stderr, "crc32c_recover_pages: %s\n", crc32c_strerror(rc));
        ++failures;
        n = 0;
    }
    /* the one rescue loop: what the walk could not vouch for is skipped, and the image's size is lens[k] */
    for (uint64_t k = 0; k < n; ++k) {
        if (kind[k] == 0) continue;
        /* (a vouched-for image is sane, so its size is the header's; the list ascends) */
        if (lens[k] != ntotal_of(page + offs[k]) || (k && offs[k - 1] >= offs[k])) ++failures;
        const int got = rescue(page, offs[k], lens[k]);
        if (kind[k] == CRC32C_ITEM_SALVAGED) salvaged += got;
        else reached += got;
    }
    printf("recover_sim: %llu entries, walk bad %llu, salvage found %llu of %llu candidates in %llu offsets\n",
           (unsigned long long)n, (unsigned long long)nbad, (unsigned long long)nsalvaged, (unsigned long long)ncand,
           (unsigned long long)scanned);
    free(offs);
    free(lens);
    free(kind);
    /* an image whose own header is damaged is never counted as rescued */
    uint64_t good = 0;
    for (uint32_t id = 0; id < nitems; ++id) {
        if (rescued[id] && damaged[id]) ++failures; /* (a verified image has an intact header) */
        good += rescued[id] && !damaged[id];
    }
    if (good != reached + salvaged) ++failures;
    printf("recover_sim: recover_pages, %u items, failures %d\n", nitems, failures);
    printf("live=%llu reached=%llu salvaged=%llu lost=%llu damaged=%llu\n", (unsigned long long)live,
           (unsigned long long)reached, (unsigned long long)salvaged, (unsigned long long)(live - reached - salvaged),
           (unsigned long long)ndamaged);
    free(page);
    return failures == 0 ? 0 : 1;
}

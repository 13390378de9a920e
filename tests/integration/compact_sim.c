/* compact_sim.c -- the device-walk stamp hook under
 * compaction: images copied verbatim with their stored CRC must keep it.
 *
 * Reference flow.  storage_write (storage.c:499-593) copies an item image
 * into a wbuf and stores crc32c() of [32, ITEM_ntotal) in exptime
 * (storage.c:567).  storage_compact_readback (storage.c:950-1070) reads a page
 * back and rewrites the images worth keeping into new wbufs verbatim, stored
 * CRC included (storage.c:1004-1006), next to freshly written items.  A read
 * compares the CRC of what it got with exptime (storage.c:159-178,
 * badcrc_from_extstore).
 *
 * Batched flow.  The writer leaves exptime 0 and one call in _submit_wbuf
 *   crc32c_stamp_pages(w->buf, w->size - w->free, w->size, ..., CRC32C_KEEP_STAMPED, NULL)
 * stamps the fresh images and verifies the carried ones without touching them.
 * A byte that flipped on flash in a carried image therefore still fails the
 * read-back compare.  Stamping every image instead (--launder: the same call
 * without the flag, what a list-based hook over all images does) gives the
 * damaged bytes a fresh, valid CRC and the damage is served as a hit.
 *
 * The run: fill wbufs with fresh images and flush them to a page file through
 * the hook; read the pages back, flip one byte in a known subset of a seeded
 * selection of images (the flash damage) and rewrite the selection verbatim
 * into new wbufs that also receive fresh images; read every live image back
 * and check it as storage.c:159-178 does.
 *
 * Usage: compact_sim [--gpu] [--launder]
 * Prints badcrc=<n> expected=<m> kept=<k> stamped=<s> (expected: the damaged
 * images).  Exit status 0 = the run itself worked; the caller judges the
 * counts.
 */
#define _GNU_SOURCE
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>

#include "crc32c.h"
#include "crc32c_batch.h"

#define WBUF (1u << 20)
#define NITEMS 6000u       /* first generation */
#define MAX_ITEMS 12000u   /* with the fresh items written during compaction */
#define ITEM_CAS 2u
#define MAX_VALUE 6000u
#define MAX_IMG (48 + 16 + 8 + MAX_VALUE + 2)
#define PER_WBUF_CAP (WBUF / 50 + 1)  /* an image is at least 50 bytes */

static uint32_t rd32(const uint8_t *p) { uint32_t v; memcpy(&v, p, 4); return v; }

static uint32_t ntotal_of(const uint8_t *p) {
    uint16_t flags;
    memcpy(&flags, p + 38, 2);
    return 48 + p[41] + 1 + rd32(p + 32) + ((flags & ITEM_CAS) ? 8 : 0);
}

static uint64_t mix(uint64_t *s) {
    uint64_t z = (*s += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}

/* the engine, reduced to one open wbuf and the page file behind it */
static struct {
    int fd;
    uint8_t *wbuf;     /* the open wbuf (page-locked, extstore.c:127-140) */
    uint32_t used;     /* w->size - w->free */
    uint32_t nimg;     /* images in it */
    uint64_t flushed;  /* bytes of the page file written */
} E;

static unsigned hook_flags = CRC32C_KEEP_STAMPED;
static int want_flags;  /* the compaction wbufs ask for per-image flags */
static uint64_t hook_nbad, kept, stamped, hook_items;
static int failures;
static uint64_t where[MAX_ITEMS];  /* file offset of each live item's image */

/* _submit_wbuf (extstore.c:559-570): the hook, the tail memset, the flush */
static void submit_wbuf(void) {
    static uint64_t offs[PER_WBUF_CAP];
    static uint8_t ok[PER_WBUF_CAP];
    uint64_t n = 0, nbad = 0;
    const uint64_t cap = want_flags ? PER_WBUF_CAP : 0;
    const int rc = crc32c_stamp_pages(E.wbuf, E.used, WBUF, cap ? offs : NULL, cap ? ok : NULL, cap, &n, &nbad,
                                      hook_flags, NULL);
    if (rc != CRC32C_OK || n != E.nimg) {
        fprintf(stderr, "hook: %s, %llu images of %u\n", crc32c_strerror(rc), (unsigned long long)n, E.nimg);
        ++failures;
    }
    hook_nbad += nbad;  /* counted like badcrc_from_extstore */
    hook_items += n;
    for (uint64_t i = 0; i < n && i < cap; ++i) {
        kept += ok[i] == CRC32C_ITEM_KEPT;
        stamped += ok[i] == CRC32C_ITEM_STAMPED;
    }
    if (!cap) stamped += n - nbad;  /* (all fresh: the first generation) */
    memset(E.wbuf + E.used, 0, WBUF - E.used);  /* extstore.c:568 */
    if (pwrite(E.fd, E.wbuf, WBUF, (off_t)E.flushed) != (ssize_t)WBUF) ++failures;
    E.flushed += WBUF;
    E.used = E.nimg = 0;
}

/* extstore_write_request + the copy of storage_write / the compaction
 * rewrite: the image's place in the page file */
static uint64_t write_image(const uint8_t *img, uint32_t nt) {
    if (E.used + nt > WBUF) submit_wbuf();
    memcpy(E.wbuf + E.used, img, nt);
    const uint64_t at = E.flushed + E.used;
    E.used += nt;
    ++E.nimg;
    return at;
}

/* a fresh item image as storage_write leaves it: exptime = 0 where
 * storage.c:567 stored the CRC */
static uint32_t fresh_image(uint8_t *img, uint32_t id, uint64_t *rng) {
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
    return nt;
}

int main(int argc, char **argv) {
    int gpu = 0;
    for (int i = 1; i < argc; ++i) {
        if (!strcmp(argv[i], "--gpu")) gpu = 1;
        else if (!strcmp(argv[i], "--launder")) hook_flags = 0;
    }
    crc32c_init();
    if (!gpu) {
        uint8_t buf[64] = {0};
        uint64_t n = 0, nbad = 0;
        const int rc = crc32c_stamp_pages(buf, sizeof buf, sizeof buf, NULL, NULL, 0, &n, &nbad, hook_flags, NULL);
        printf("compact_sim: no GPU, stamp reports %s\n", crc32c_strerror(rc));
        return rc == CRC32C_ENODEV ? 0 : 1;
    }
    FILE *pf = tmpfile();
    E.wbuf = crc32c_host_alloc(WBUF);
    uint8_t *page = malloc(WBUF);  /* the compaction's readback_buf (storage.c:1120) */
    if (!pf || !E.wbuf || !page) {
        fprintf(stderr, "setup failed\n");
        return 1;
    }
    E.fd = fileno(pf);
    static uint8_t img[MAX_IMG];
    uint64_t rng = 11;

    /* first generation: fresh images only */
    for (uint32_t id = 0; id < NITEMS; ++id) {
        const uint32_t nt = fresh_image(img, id, &rng);
        where[id] = write_image(img, nt);
    }
    submit_wbuf();
    const uint64_t gen1_bytes = E.flushed, gen1_items = hook_items;
    if (hook_nbad || gen1_items != NITEMS) ++failures;

    /* compaction: read the pages back; a seeded selection of images is
     * rewritten verbatim, every 7th of them after one of its bytes flipped on
     * flash; fresh items arrive in between */
    static uint8_t damaged[NITEMS];
    static uint64_t old_where[NITEMS];
    memcpy(old_where, where, sizeof old_where);
    uint64_t expected = 0, nrescued = 0;
    uint32_t next_id = NITEMS;
    want_flags = 1;
    for (uint64_t p0 = 0; p0 < gen1_bytes; p0 += WBUF) {
        if (pread(E.fd, page, WBUF, (off_t)p0) != (ssize_t)WBUF) ++failures;
        for (uint32_t id = 0; id < NITEMS; ++id) {
            if (old_where[id] < p0 || old_where[id] >= p0 + WBUF || mix(&rng) % 5 >= 2) continue;
            uint8_t *im = page + (old_where[id] - p0);
            const uint32_t nt = ntotal_of(im);
            if (nrescued++ % 7 == 3) {
                im[48 + mix(&rng) % (nt - 48)] ^= (uint8_t)(1u << (mix(&rng) % 8));
                damaged[id] = 1;
                ++expected;
            }
            /* the rewrite (storage.c:1004-1006): the image as read, CRC included */
            where[id] = write_image(im, nt);  /* the item now lives at its new place */
            if (nrescued % 2 == 0 && next_id < MAX_ITEMS) {
                const uint32_t fid = next_id++;
                const uint32_t fnt = fresh_image(img, fid, &rng);
                where[fid] = write_image(img, fnt);
            }
        }
    }
    submit_wbuf();

    /* read every live image back and check it as storage.c:159-178 does */
    uint64_t badcrc = 0, bad_undamaged = 0, reads = 0;
    for (uint32_t id = 0; id < next_id; ++id) {
        uint8_t hdr[48];
        if (pread(E.fd, hdr, 48, (off_t)where[id]) != 48) ++failures;
        const uint32_t nt = ntotal_of(hdr);
        if (nt > MAX_IMG || pread(E.fd, img, nt, (off_t)where[id]) != (ssize_t)nt) {
            ++failures;
            continue;
        }
        const int bad = crc32c(0, img + 32, nt - 32) != rd32(img + 28);
        badcrc += bad;
        bad_undamaged += bad && !(id < NITEMS && damaged[id]);
        ++reads;
    }
    printf("compact_sim: %s, %llu items then %llu rescued + %u fresh, reads %llu, hook items %llu nbad %llu, "
           "bad but undamaged %llu, failures %d\n",
           hook_flags ? "keep-stamped" : "launder", (unsigned long long)gen1_items, (unsigned long long)nrescued,
           next_id - NITEMS, (unsigned long long)reads, (unsigned long long)hook_items, (unsigned long long)hook_nbad,
           (unsigned long long)bad_undamaged, failures);
    printf("badcrc=%llu expected=%llu kept=%llu stamped=%llu\n", (unsigned long long)badcrc,
           (unsigned long long)expected, (unsigned long long)kept, (unsigned long long)stamped);
    free(page);
    crc32c_host_free(E.wbuf);
    fclose(pf);
    return failures == 0 && bad_undamaged == 0 && reads == next_id ? 0 : 1;
}

/* copy_sim.c -- storage_compact_readback's rescue copy through
 * crc32c_copy_items.
 *
 * Reference flow.  storage_compact_readback (storage.c:933-1072) walks a page
 * it has read back, looks every image up in the hash table
 * (storage.c:964-990) and memcpy's the ones worth keeping verbatim into a new
 * wbuf (storage.c:1004-1006), stored CRC included, then relinks the item to its
 * new place (storage.c:1015-1021).  Nothing is checked: an image that was
 * damaged on flash is carried along and only fails when a client reads it
 * (storage.c:160-178, badcrc_from_extstore).
 *
 * Batched flow.  The walk records (offset, destination) pairs instead of
 * copying, one crc32c_copy_items call after the walk moves the images and says
 * which ones were intact, and only those are relinked; a damaged item is
 * dropped at the moment of the copy.
 *
 * The run: fill and flush wbufs of stamped images into a page file; read the
 * page back into a page-locked readback_buf; flip one byte in a known subset of
 * a seeded live set; reserve the live images' destinations back to back in
 * page-locked wbufs; one call; relink the CRC32C_ITEM_COPIED images; flush the
 * new wbufs; read every linked item back and check it as storage.c:160-178
 * does.  --memcpy runs the reference's unchecked copy instead.
 *
 * Usage: copy_sim [--gpu] [--memcpy]
 * Prints rescued=<r> dropped=<d> expected=<e> badcrc_after=<b> (expected: the
 * damaged live images).  Exit status 0 = the run itself worked; the caller
 * judges the counts.
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
#define NWBUF 8u              /* the page: 8 wbufs */
#define PAGE (NWBUF * WBUF)
#define MAX_ITEMS 4000u
#define ITEM_CAS 2u
#define MAX_VALUE 6000u
#define MAX_IMG (48 + 16 + 8 + MAX_VALUE + 2)
#define GONE UINT64_MAX

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

int main(int argc, char **argv) {
    int gpu = 0, plain = 0;
    for (int i = 1; i < argc; ++i) {
        if (!strcmp(argv[i], "--gpu")) gpu = 1;
        else if (!strcmp(argv[i], "--memcpy")) plain = 1;
    }
    crc32c_init();
    if (!gpu) {
        uint8_t src[64] = {0}, dst[64], ok[1] = {9};
        uint64_t so[1] = {0}, dof[1] = {0}, nbad = 0;
        memset(dst, 0xa5, sizeof dst);
        const int rc = crc32c_copy_items(src, sizeof src, 0, so, dst, sizeof dst, dof, 1, ok, &nbad, 0, NULL);
        printf("copy_sim: no GPU, copy reports %s\n", crc32c_strerror(rc));
        return rc == CRC32C_ENODEV && ok[0] == 9 && dst[0] == 0xa5 ? 0 : 1;
    }
    FILE *pf = tmpfile();
    uint8_t *wbuf = crc32c_host_alloc(WBUF);       /* the open wbuf of the first generation */
    uint8_t *readback = crc32c_host_alloc(PAGE);   /* storage.c:1120 */
    uint8_t *newbufs = crc32c_host_alloc(PAGE);    /* the wbufs compaction writes into */
    if (!pf || !wbuf || !readback || !newbufs) {
        fprintf(stderr, "setup failed\n");
        return 1;
    }
    const int fd = fileno(pf);
    static uint8_t img[MAX_IMG];
    static uint64_t where[MAX_ITEMS];  /* file offset of each linked item's image, or GONE */
    static uint32_t nt_of[MAX_ITEMS];
    int failures = 0;
    uint64_t rng = 23;

    /* fill and flush the page */
    uint32_t nitems = 0, used = 0, flushed = 0;
    memset(wbuf, 0, WBUF);
    for (;; ++nitems) {
        const uint32_t nt = make_image(img, nitems, &rng);
        if (used + nt > WBUF) {
            if (pwrite(fd, wbuf, WBUF, (off_t)flushed) != (ssize_t)WBUF) ++failures;
            flushed += WBUF;
            used = 0;
            memset(wbuf, 0, WBUF);
            if (flushed == PAGE) break;
        }
        if (nitems >= MAX_ITEMS) {
            fprintf(stderr, "item table too small\n");
            return 1;
        }
        memcpy(wbuf + used, img, nt);
        where[nitems] = flushed + used;
        nt_of[nitems] = nt;
        used += nt;
    }

    /* compaction: read the page back, damage a known subset of the live set */
    if (pread(fd, readback, PAGE, 0) != (ssize_t)PAGE) ++failures;
    static uint64_t src_offs[MAX_ITEMS], dst_offs[MAX_ITEMS];
    static uint32_t live_id[MAX_ITEMS];
    static uint8_t damaged[MAX_ITEMS], ok[MAX_ITEMS];
    uint64_t nlive = 0, expected = 0, dst_used = 0;
    for (uint32_t id = 0; id < nitems; ++id) {
        if (mix(&rng) % 5 >= 2) {  /* not worth keeping: the page is freed under it */
            where[id] = GONE;
            continue;
        }
        uint8_t *im = readback + where[id];
        if (nlive % 9 == 4) {
            im[48 + mix(&rng) % (nt_of[id] - 48)] ^= (uint8_t)(1u << (mix(&rng) % 8));
            damaged[id] = 1;
            ++expected;
        }
        /* extstore_write_request: the next free place, never across a wbuf */
        const uint32_t nt = ntotal_of(im);
        if (dst_used % WBUF + nt > WBUF) dst_used = (dst_used / WBUF + 1) * WBUF;
        src_offs[nlive] = where[id];
        dst_offs[nlive] = dst_used;
        live_id[nlive++] = id;
        dst_used += nt;
    }
    const uint64_t dst_bytes = (dst_used + WBUF - 1) / WBUF * WBUF;
    if (dst_bytes > PAGE) {
        fprintf(stderr, "live set larger than a page\n");
        return 1;
    }
    memset(newbufs, 0, dst_bytes);

    uint64_t rescued = 0, dropped = 0, nbad = 0;
    if (plain) {  /* storage.c:1004-1006 and :1015-1021 as they are */
        for (uint64_t k = 0; k < nlive; ++k) {
            memcpy(newbufs + dst_offs[k], readback + src_offs[k], ntotal_of(readback + src_offs[k]));
            where[live_id[k]] = PAGE + dst_offs[k];
            ++rescued;
        }
    } else {
        const int rc = crc32c_copy_items(readback, PAGE, WBUF, src_offs, newbufs, dst_bytes, dst_offs, nlive, ok, &nbad,
                                         0, NULL);
        if (rc != CRC32C_OK) {
            fprintf(stderr, "crc32c_copy_items: %s\n", crc32c_strerror(rc));
            ++failures;
        }
        for (uint64_t k = 0; k < nlive; ++k) {
            const uint32_t id = live_id[k];
            if (ok[k] == CRC32C_ITEM_COPIED) {  /* the relink, behind the verdict */
                where[id] = PAGE + dst_offs[k];
                ++rescued;
            } else {
                where[id] = GONE;  /* dropped: the item is unlinked, counted like badcrc_from_extstore */
                ++dropped;
                if (ok[k] != CRC32C_ITEM_DAMAGED || !damaged[id]) ++failures;
            }
            /* every image was moved verbatim, damaged or not */
            if (memcmp(newbufs + dst_offs[k], readback + src_offs[k], nt_of[id]) != 0) ++failures;
        }
        if (nbad != dropped) ++failures;
    }
    /* the destination wbufs are submitted only now */
    if (pwrite(fd, newbufs, dst_bytes, (off_t)PAGE) != (ssize_t)dst_bytes) ++failures;

    /* read every linked item back and check it as storage.c:160-178 does */
    uint64_t badcrc = 0, bad_undamaged = 0, reads = 0;
    for (uint32_t id = 0; id < nitems; ++id) {
        if (where[id] == GONE) continue;
        uint8_t hdr[48];
        if (pread(fd, hdr, 48, (off_t)where[id]) != 48) ++failures;
        const uint32_t nt = ntotal_of(hdr);
        if (nt > MAX_IMG || pread(fd, img, nt, (off_t)where[id]) != (ssize_t)nt) {
            ++failures;
            continue;
        }
        const int bad = crc32c(0, img + 32, nt - 32) != rd32(img + 28);
        badcrc += bad;
        bad_undamaged += bad && !damaged[id];
        ++reads;
    }
    printf("copy_sim: %s, %u items, %llu live, reads %llu, nbad %llu, bad but undamaged %llu, failures %d\n",
           plain ? "memcpy" : "copy_items", nitems, (unsigned long long)nlive, (unsigned long long)reads,
           (unsigned long long)nbad, (unsigned long long)bad_undamaged, failures);
    printf("rescued=%llu dropped=%llu expected=%llu badcrc_after=%llu\n", (unsigned long long)rescued,
           (unsigned long long)dropped, (unsigned long long)expected, (unsigned long long)badcrc);
    crc32c_host_free(newbufs);
    crc32c_host_free(readback);
    crc32c_host_free(wbuf);
    fclose(pf);
    return failures == 0 && bad_undamaged == 0 && reads == rescued ? 0 : 1;
}

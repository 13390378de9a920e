/* salvage_sim.c -- storage_compact_readback over a page with damaged headers,
 * with and without crc32c_salvage_pages.
 *
 * Reference flow.  storage_compact_readback (storage.c:950-1072) walks each
 * wbuf of the page it read back from its first byte, image to image by
 * ITEM_ntotal, until nkey == 0 or fewer than 48 bytes are left, and rescues an
 * image only when its key is still linked to exactly this page and offset
 * (storage.c:964-975).  One flipped header bit therefore ends or derails the
 * walk, and every live image packed behind it in that wbuf is lost when the
 * page is freed, silently: the hash table still points at it.
 *
 * Batched flow.  crc32c_verify_pages walks and verifies the page, then
 * crc32c_salvage_pages takes the walk's lists and returns the intact images
 * the walk did not reach; the same rescue loop, with the same key and offset
 * check, runs over both lists.  Only the images whose own header was damaged
 * stay lost.
 *
 * The run: readback_page.h's page with the header damage alone
 * (DAMAGE_HEADERS): one header bit (nkey, nbytes or it_flags, in turn) of
 * every 37th live image flipped "on flash", then the read-back either way.
 *
 * Usage: salvage_sim [--gpu] [--walk]
 * Prints live=<l> reached=<r> salvaged=<s> lost=<x> damaged=<d>: reached = live
 * images with an undamaged header that the walk arrived at, salvaged = those
 * the salvage added, lost = live - reached - salvaged.  Exit status 0 = the run
 * itself worked; the caller judges the counts.
 */
#include "readback_page.h"

int main(int argc, char **argv) {
    int gpu = 0, walk_only = 0;
    for (int i = 1; i < argc; ++i) {
        if (!strcmp(argv[i], "--gpu")) gpu = 1;
        else if (!strcmp(argv[i], "--walk")) walk_only = 1;
    }
    crc32c_init();
    if (!gpu) {
        uint8_t buf[64] = {0};
        uint64_t o1[1] = {9}, nfound = 9;
        const int rc = crc32c_salvage_pages(buf, sizeof buf, 64, NULL, NULL, 0, o1, 1, &nfound, NULL, NULL, 0, NULL);
        printf("salvage_sim: no GPU, salvage reports %s\n", crc32c_strerror(rc));
        return rc == CRC32C_ENODEV && o1[0] == 9 && nfound == 9 ? 0 : 1;
    }
    uint8_t *page = malloc(PAGE);
    struct page_counts c;
    if (!page || page_build(page, NULL, DAMAGE_HEADERS, &c) != 0) return 1;

    uint64_t reached = 0, salvaged = 0;
    if (walk_only) { /* storage.c:950-1072 as it is: no CRC is checked and the rescue check may read up to the wbuf's
                      * end, which readback_page.h's reference_walk does otherwise */
        for (uint32_t w = 0; w < NWBUF; ++w) {
            uint64_t off = 0;
            while (off + 48 <= WBUF && page[w * (uint64_t)WBUF + off + 41] != 0) {
                const uint64_t o = w * (uint64_t)WBUF + off;
                reached += rescue(page, o, WBUF - off, NULL);
                off += ntotal_of(page + o);
            }
        }
    } else { /* (the walk's list has ok[] for kind[] and no lens[]: it is not readback_page.h's list) */
        const uint64_t room = PAGE / 50 + NWBUF;
        uint64_t *walked = malloc(room * 8), *found = malloc(room * 8);
        uint8_t *ok = malloc(room);
        uint64_t nwalked = 0, nbad = 0, nfound = 0, scanned = 0, ncand = 0;
        if (!walked || !found || !ok) return 1;
        int rc = crc32c_verify_pages(page, PAGE, WBUF, walked, ok, room, &nwalked, &nbad, 0, NULL);
        if (rc != CRC32C_OK || nwalked > room) {
            fprintf(stderr, "crc32c_verify_pages: %s\n", crc32c_strerror(rc));
            ++failures;
            nwalked = 0;
        }
        for (uint64_t k = 0; k < nwalked; ++k)
            if (ok[k]) reached += rescue(page, walked[k], WBUF - walked[k] % WBUF, NULL);
        rc = crc32c_salvage_pages(page, PAGE, WBUF, walked, ok, nwalked, found, room, &nfound, &scanned, &ncand, 0,
                                  NULL);
        if (rc != CRC32C_OK || nfound > room) {
            fprintf(stderr, "crc32c_salvage_pages: %s\n", crc32c_strerror(rc));
            ++failures;
            nfound = 0;
        }
        for (uint64_t k = 0; k < nfound; ++k) salvaged += rescue(page, found[k], WBUF - found[k] % WBUF, NULL);
        printf("salvage_sim: walk items %llu bad %llu, salvage found %llu of %llu candidates in %llu offsets\n",
               (unsigned long long)nwalked, (unsigned long long)nbad, (unsigned long long)nfound,
               (unsigned long long)ncand, (unsigned long long)scanned);
        free(walked);
        free(found);
        free(ok);
    }
    /* an image whose own header is damaged is never counted as rescued */
    uint64_t good = 0;
    for (uint32_t id = 0; id < nitems; ++id) {
        if (rescued[id] && damaged[id]) {
            if (walk_only) --reached;  /* (the walk met it by its key; its size can no longer be trusted) */
            else ++failures;           /* (a verified image has an intact header) */
        }
        good += rescued[id] && !damaged[id];
    }
    if (good != reached + salvaged) ++failures;
    printf("salvage_sim: %s, %u items, failures %d\n", walk_only ? "walk" : "verify_pages + salvage_pages", nitems,
           failures);
    printf("live=%llu reached=%llu salvaged=%llu lost=%llu damaged=%llu\n", (unsigned long long)c.live,
           (unsigned long long)reached, (unsigned long long)salvaged, (unsigned long long)(c.live - reached - salvaged),
           (unsigned long long)c.ndamaged);
    free(page);
    return failures == 0 ? 0 : 1;
}

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
 * The run: as salvage_sim.c, readback_page.h's page with the header damage
 * alone (DAMAGE_HEADERS).
 *
 * Usage: recover_sim [--gpu]
 * Prints live=<l> reached=<r> salvaged=<s> lost=<x> damaged=<d> as salvage_sim
 * does: reached = live images with an undamaged header that the walk arrived
 * at (kind 1), salvaged = those the salvage added (kind CRC32C_ITEM_SALVAGED),
 * lost = live - reached - salvaged.  Exit status 0 = the run itself worked;
 * the caller judges the counts.
 */
#include "readback_page.h"

int main(int argc, char **argv) {
    int gpu = 0;
    for (int i = 1; i < argc; ++i)
        if (!strcmp(argv[i], "--gpu")) gpu = 1;
    crc32c_init();
    if (!gpu) {
        uint8_t buf[64] = {0};
        uint64_t o1[1] = {9}, n1 = 9, nbad = 9, nsalvaged = 9;
        uint32_t lens1[1] = {9};
        uint8_t kind1[1] = {9};
        const int rc = crc32c_recover_pages(buf, sizeof buf, 64, o1, lens1, kind1, 1, &n1, &nbad, &nsalvaged, NULL, NULL,
                                            0, NULL);
        printf("recover_sim: no GPU, recover reports %s\n", crc32c_strerror(rc));
        return rc == CRC32C_ENODEV && o1[0] == 9 && lens1[0] == 9 && kind1[0] == 9 && n1 == 9 && nbad == 9 &&
                       nsalvaged == 9
                   ? 0
                   : 1;
    }
    uint8_t *page = malloc(PAGE);
    struct page_counts c;
    if (!page || page_build(page, NULL, DAMAGE_HEADERS, &c) != 0) return 1;

    uint64_t reached = 0, salvaged = 0;
    uint64_t nbad = 0, nsalvaged = 0, scanned = 0, ncand = 0;
    /* the walk's bound and the salvage's, together */
    if (list_alloc(2 * (PAGE / 50) + NWBUF) != 0) return 1;
    /* (not recover(): this sim prints the call's own counts) */
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
        const int got = rescue(page, offs[k], lens[k], NULL);
        if (kind[k] == CRC32C_ITEM_SALVAGED) salvaged += got;
        else reached += got;
    }
    printf("recover_sim: %llu entries, walk bad %llu, salvage found %llu of %llu candidates in %llu offsets\n",
           (unsigned long long)n, (unsigned long long)nbad, (unsigned long long)nsalvaged, (unsigned long long)ncand,
           (unsigned long long)scanned);
    list_free();
    /* an image whose own header is damaged is never counted as rescued */
    uint64_t good = 0;
    for (uint32_t id = 0; id < nitems; ++id) {
        if (rescued[id] && damaged[id]) ++failures; /* (a verified image has an intact header) */
        good += rescued[id] && !damaged[id];
    }
    if (good != reached + salvaged) ++failures;
    printf("recover_sim: recover_pages, %u items, failures %d\n", nitems, failures);
    printf("live=%llu reached=%llu salvaged=%llu lost=%llu damaged=%llu\n", (unsigned long long)c.live,
           (unsigned long long)reached, (unsigned long long)salvaged, (unsigned long long)(c.live - reached - salvaged),
           (unsigned long long)c.ndamaged);
    free(page);
    return failures == 0 ? 0 : 1;
}

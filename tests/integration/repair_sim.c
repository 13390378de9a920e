/* repair_sim.c -- storage_compact_readback over a page with damaged headers and
 * damaged data, through crc32c_recover_pages and crc32c_repair_items
 * (INTEGRATION.md section 4e): readback_page.h's page with recover_sim.c's
 * header damage and bits flipped inside live images added to it (DAMAGE_BITS).
 *
 * Three flows over the same bytes:
 *   reference  the walk of storage.c:950-1072 with the scalar crc32c: an image
 *              whose CRC fails is skipped, a damaged header ends the wbuf;
 *   recover    crc32c_recover_pages alone: one rescue loop over its merged list,
 *              kind 0 skipped;
 *   repair     crc32c_recover_pages, then crc32c_repair_items over the entries
 *              with kind == 0 && lens != 0 (reached, sane, CRC failing); the
 *              repaired ones join the rescue loop.
 *
 * The damage "on flash": one header bit of every 37th live image, as in
 * recover_sim.c; of the other live images every 7th has one bit of its stored
 * CRC or of the bytes it covers flipped, every fifth of those a second bit.
 *
 * What the rule cannot fix is counted by the sim's own CPU search
 * (crc32c_locate_bit over each damaged live image with the length the sim gave
 * it): a flipped length bit, damage of more than one bit, and -- the flow's own
 * limit -- damaged images that crc32c_recover_pages does not list at all,
 * because they lie behind a header that ended their wbuf's walk and the
 * salvage reports intact images only.
 *
 * Usage: repair_sim [--gpu]
 * Prints live=<l> lost_reference=<a> lost_recover=<b> lost_repair=<c>
 * repaired=<r> unrepairable=<u> length=<x> multi=<y> unlisted=<z> (u = x + y +
 * z).  Exit status 0 = the run itself worked; the caller judges the counts.
 */
#include "readback_page.h"

int main(int argc, char **argv) {
    int gpu = 0;
    for (int i = 1; i < argc; ++i)
        if (!strcmp(argv[i], "--gpu")) gpu = 1;
    crc32c_init();
    if (!gpu) {
        uint8_t buf[64] = {0};
        uint64_t o1[1] = {0}, bit[1] = {9}, nrep = 9, nbad = 9;
        uint8_t ok[1] = {9};
        const int rc = crc32c_repair_items(buf, sizeof buf, 0, o1, 1, 0, ok, bit, &nrep, &nbad, 0, NULL);
        printf("repair_sim: no GPU, repair reports %s\n", crc32c_strerror(rc));
        return rc == CRC32C_ENODEV && ok[0] == 9 && bit[0] == 9 && nrep == 9 && nbad == 9 ? 0 : 1;
    }
    uint8_t *page = malloc(PAGE), *pristine = malloc(PAGE);
    struct page_counts c;
    if (!page || !pristine || page_build(page, pristine, DAMAGE_BITS, &c) != 0) return 1;

    /* flow 1, the reference */
    reference_walk(page);
    const uint64_t got_reference = count_rescued();

    /* flow 2: crc32c_recover_pages alone */
    if (list_alloc(2 * (PAGE / 50) + NWBUF) != 0) return 1;
    uint64_t *bad = malloc(cap * 8), *bit = malloc(cap * 8);
    uint8_t *ok = malloc(cap);
    if (!bad || !bit || !ok) return 1;
    const uint64_t lost_recover = lost_now(page, c.live);
    memset(rescued, 0, sizeof rescued);

    /* flow 3: the same list, the damaged sane entries repaired first */
    uint64_t m = item_list(bad, NULL, NULL), nrep = 0, nrbad = 0, repaired_live = 0;
    const int rc = crc32c_repair_items(page, PAGE, WBUF, bad, m, 0, ok, bit, &nrep, &nrbad, 0, NULL);
    if (rc != CRC32C_OK) {
        fprintf(stderr, "crc32c_repair_items: %s\n", crc32c_strerror(rc));
        ++failures;
        m = 0;
    }
    for (uint64_t k = 0, j = 0; k < n; ++k) {
        int take = kind[k] != 0;
        if (kind[k] == 0 && lens[k] != 0 && j < m) {
            take = ok[j] == CRC32C_ITEM_REPAIRED || ok[j] == 1;
            ++j;
        }
        uint32_t id = 0;
        if (take && rescue(page, offs[k], lens[k], &id) && kind[k] == 0) {
            ++repaired_live;
            /* a repaired image is the image that was written */
            if (memcmp(page + offs[k], pristine + offs[k], size_of[id]) != 0) ++failures;
        }
    }
    const uint64_t got_repair = count_rescued();
    mark_listed();
    printf("repair_sim: %llu entries, %llu given to the repair, %llu repaired, %llu not\n", (unsigned long long)n,
           (unsigned long long)m, (unsigned long long)nrep, (unsigned long long)nrbad);

    /* the sim's own count of what the rule cannot fix, from the bytes as they were read (the repairs undone) */
    uint64_t c_length = 0, c_multi = 0, c_unlisted = 0;
    for (uint32_t id = 0; id < nitems; ++id) {
        if (where[id] == GONE || !damaged[id]) continue;
        const uint8_t *im = page + where[id];
        const uint32_t nt = size_of[id];
        if (rescued[id]) continue; /* (repaired: counted above against the pristine bytes) */
        const uint64_t q = crc32c_locate_bit(crc32c(0, im + 32, nt - 32), rd32(im + 28), nt - 32);
        if (q == CRC32C_NO_BIT) ++c_multi;
        else if (length_bit(224 + q)) ++c_length;
        else if (!listed[id]) ++c_unlisted;
        else ++failures; /* one bit, no length bit, listed: the repair should have taken it */
    }
    list_free(); free(bad); free(bit); free(ok);
    printf("repair_sim: %u items, %llu header-damaged, %llu data-damaged, failures %d\n", nitems,
           (unsigned long long)c.ndamaged, (unsigned long long)c.ndata, failures);
    printf("live=%llu lost_reference=%llu lost_recover=%llu lost_repair=%llu repaired=%llu unrepairable=%llu "
           "length=%llu multi=%llu unlisted=%llu\n",
           (unsigned long long)c.live, (unsigned long long)(c.live - got_reference), (unsigned long long)lost_recover,
           (unsigned long long)(c.live - got_repair), (unsigned long long)repaired_live,
           (unsigned long long)(c_length + c_multi + c_unlisted), (unsigned long long)c_length,
           (unsigned long long)c_multi, (unsigned long long)c_unlisted);
    free(page);
    free(pristine);
    return failures == 0 ? 0 : 1;
}

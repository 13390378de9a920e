/* header_sim.c -- storage_compact_readback over a page with damaged headers and
 * damaged data, through crc32c_recover_pages, crc32c_repair_headers and
 * crc32c_repair_items (INTEGRATION.md sections 4e and 4f): readback_page.h's
 * page with recover_sim.c's header damage and single length bits and data bits
 * flipped inside other live images added to it (DAMAGE_LENGTHS).
 *
 * The flow over the bytes, each stage's loss counted by a read-back and rescue
 * loop of its own (crc32c_recover_pages, kind 0 skipped):
 *   recover   crc32c_recover_pages alone;
 *   headers   the list of INTEGRATION.md 4f (header_list: every kind 0 entry,
 *             every wbuf's walk end that is no entry) given to
 *             crc32c_repair_headers, the page walked again, and so on while a
 *             round repairs a header: a wbuf's walk reaches its second
 *             damaged header only when the first one is right;
 *   items     crc32c_repair_items over the entries with kind == 0 && lens != 0
 *             of the last walk.
 *
 * The damage "on flash": one header bit of every 37th live image, as in
 * recover_sim.c (nkey zeroed -- two bits of a 10-byte key's length, no rule
 * fixes that --, an nbytes bit, the ITEM_CAS bit); of the other live images
 * every 11th has one of the 42 length bits flipped, every 7th of the rest one
 * bit of its stored CRC or of the bytes it covers, every fifth of those a second.
 *
 * What no rule can fix is counted by the sim itself from the pristine bytes and
 * the layout it wrote, not from any list of the flow: damage of more than one
 * bit, and one-bit damage behind, in its wbuf, a header whose nkey was zeroed
 * (two bits: no rule fixes it, it keeps ending the wbuf's walk, and the salvage
 * behind it reports intact images only).  Any other image that does not come
 * back -- intact, or with one bit flipped in front of every such header of its
 * wbuf -- is a failure of the run.
 *
 * Usage: header_sim [--gpu]
 * Prints live=<l> lost_recover=<a> lost_headers=<b> lost_items=<c>
 * headers_repaired=<h> items_repaired=<i> rounds=<r> unrepairable=<u>
 * multi=<x> behind=<y> (u = x + y).  Exit status 0 = the run itself worked;
 * the caller judges the counts.
 */
#include "readback_page.h"

static uint64_t *todo, *bit;
static uint32_t *hlens;
static uint8_t *ok;

int main(int argc, char **argv) {
    int gpu = 0;
    for (int i = 1; i < argc; ++i)
        if (!strcmp(argv[i], "--gpu")) gpu = 1;
    crc32c_init();
    if (!gpu) {
        uint8_t buf[64] = {0}, ok1[1] = {9};
        uint64_t o1[1] = {0}, bit1[1] = {9}, nrep = 9, nbad = 9;
        uint32_t lens1[1] = {9};
        const int rc = crc32c_repair_headers(buf, sizeof buf, 0, o1, 1, ok1, bit1, lens1, &nrep, &nbad, 0, NULL);
        printf("header_sim: no GPU, the header repair reports %s\n", crc32c_strerror(rc));
        return rc == CRC32C_ENODEV && ok1[0] == 9 && bit1[0] == 9 && lens1[0] == 9 && nrep == 9 && nbad == 9 ? 0 : 1;
    }
    uint8_t *page = malloc(PAGE), *pristine = malloc(PAGE);
    struct page_counts c;
    if (!page || !pristine || page_build(page, pristine, DAMAGE_LENGTHS, &c) != 0) return 1;
    const uint64_t live = c.live;

    if (list_alloc(2 * (PAGE / 50) + NWBUF) != 0) return 1;
    todo = malloc((cap + NWBUF) * 8), bit = malloc((cap + NWBUF) * 8);
    hlens = malloc((cap + NWBUF) * 4), ok = malloc(cap + NWBUF);
    if (!todo || !bit || !hlens || !ok) return 1;

    /* stage 1: crc32c_recover_pages alone */
    const uint64_t lost_recover = lost_now(page, live);

    /* stage 2: the headers, round by round (lost_now left the walk's lists behind) */
    uint64_t headers_repaired = 0;
    int rounds = 0;
    for (; rounds < MAX_ROUNDS; ++rounds) {
        const uint64_t m = header_list(todo); /* INTEGRATION.md 4f */
        uint64_t nrep = 0, nleft = 0;
        const int rc = crc32c_repair_headers(page, PAGE, WBUF, todo, m, ok, bit, hlens, &nrep, &nleft, 0, NULL);
        if (rc != CRC32C_OK) {
            fprintf(stderr, "crc32c_repair_headers: %s\n", crc32c_strerror(rc));
            ++failures;
            break;
        }
        headers_repaired += nrep;
        if (nrep == 0) break;
        recover(page);
    }
    const uint64_t lost_headers = lost_now(page, live);

    /* stage 3: the damaged sane entries of the last walk */
    uint64_t items_repaired = 0, nleft = 0;
    const uint64_t m = item_list(todo, NULL, NULL);
    const int rc = crc32c_repair_items(page, PAGE, WBUF, todo, m, 0, ok, bit, &items_repaired, &nleft, 0, NULL);
    if (rc != CRC32C_OK) {
        fprintf(stderr, "crc32c_repair_items: %s\n", crc32c_strerror(rc));
        ++failures;
    }
    const uint64_t lost_items = lost_now(page, live);

    /* the sim's own count of what no rule can fix, from the pristine bytes; a rescued image is the one written */
    uint64_t c_multi = 0, c_behind = 0, first_dead[NWBUF];
    first_dead_of(first_dead);
    for (uint32_t id = 0; id < nitems; ++id) {
        if (where[id] == GONE) continue;
        const uint8_t *im = page + where[id], *was = pristine + where[id];
        if (rescued[id]) {
            if (memcmp(im + 28, was + 28, size_of[id] - 28) != 0) ++failures;
            continue;
        }
        uint64_t which = 0;
        const uint32_t nflipped = flipped_bits(im, was, size_of[id], &which);
        if (nflipped >= 2) ++c_multi;
        else if (nflipped == 1 && at[id] > first_dead[at[id] / WBUF]) ++c_behind;
        else ++failures; /* intact, or one bit in front of every such header: it should have come back */
    }
    printf("header_sim: %u items, %llu header-damaged, %llu with a length bit, %llu data-damaged, failures %d\n", nitems,
           (unsigned long long)c.ndamaged, (unsigned long long)c.nlen, (unsigned long long)c.ndata, failures);
    printf("live=%llu lost_recover=%llu lost_headers=%llu lost_items=%llu headers_repaired=%llu items_repaired=%llu "
           "rounds=%d unrepairable=%llu multi=%llu behind=%llu\n",
           (unsigned long long)live, (unsigned long long)lost_recover, (unsigned long long)lost_headers,
           (unsigned long long)lost_items, (unsigned long long)headers_repaired, (unsigned long long)items_repaired,
           rounds, (unsigned long long)(c_multi + c_behind), (unsigned long long)c_multi,
           (unsigned long long)c_behind);
    list_free(); free(todo); free(bit); free(hlens); free(ok);
    free(page);
    free(pristine);
    return failures == 0 ? 0 : 1;
}

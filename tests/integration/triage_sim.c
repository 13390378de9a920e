/* triage_sim.c -- header_sim.c's read-back of a page with damaged headers and
 * damaged data (readback_page.h's page, DAMAGE_LENGTHS), played twice over the
 * same damaged bytes:
 *   the old flow  header_sim.c's: crc32c_recover_pages, rounds of
 *                 crc32c_repair_headers, crc32c_repair_items over the entries
 *                 with kind == 0 && lens != 0;
 *   the new flow  the same rounds with crc32c_triage_pages in
 *                 crc32c_recover_pages' place, and a repair list that also
 *                 holds every suspect (kind CRC32C_ITEM_SUSPECT) that passes
 *                 the caller's filter of INTEGRATION.md section 4g: a suspect
 *                 whose [o, o + lens) reaches the next kind-1 or kind-4 entry,
 *                 or overlaps an earlier kept suspect, is dropped (a true
 *                 image is disjoint from proven ones; a false repair must not
 *                 write into a proven image).
 * Each stage's loss is counted by a read-back and rescue loop of its own
 * (kinds 0 and 6 skipped).
 *
 * What no rule can fix now is counted by the sim itself from the pristine bytes
 * and the layout it wrote, not from any list of the flow: damage of more than
 * one bit, and one-bit damage behind, in its wbuf, a header whose nkey was
 * zeroed when the bit is a length bit (the image's end is wrong: no candidate)
 * or lies in the final CRLF (no candidate either).  Any other image that does
 * not come back is a failure of the run.
 *
 * Usage: triage_sim [--gpu]
 * Prints live=<l> lost_old=<o> lost_recover=<a> lost_headers=<b> lost_triage=<c>
 * headers_repaired=<h> items_repaired=<i> suspects=<s> suspects_kept=<k>
 * rounds=<r> unrepairable=<u> multi=<x> behind_length=<y> behind_crlf=<z>
 * (u = x + y + z).  Exit status 0 = the run itself worked; the caller judges
 * the counts.
 */
#include "readback_page.h"

static uint64_t *todo, *bit;
static uint32_t *hlens;
static uint8_t *ok;

struct flow {
    uint64_t lost_recover, lost_headers, lost_items, headers_repaired, items_repaired, suspects, suspects_kept;
    int rounds;
};

/* header_sim.c's three stages over `page`, its list from recover() */
static struct flow play(uint8_t *page, uint64_t live) {
    struct flow f;
    memset(&f, 0, sizeof f);
    /* stage 1: the list alone */
    f.lost_recover = lost_now(page, live);

    /* stage 2: the headers, round by round (lost_now left the walk's lists behind) */
    for (; f.rounds < MAX_ROUNDS; ++f.rounds) {
        const uint64_t m = header_list(todo); /* INTEGRATION.md 4f */
        uint64_t nrep = 0, nleft = 0;
        const int rc = crc32c_repair_headers(page, PAGE, WBUF, todo, m, ok, bit, hlens, &nrep, &nleft, 0, NULL);
        if (rc != CRC32C_OK) {
            fprintf(stderr, "crc32c_repair_headers: %s\n", crc32c_strerror(rc));
            ++failures;
            break;
        }
        f.headers_repaired += nrep;
        if (nrep == 0) break;
        recover(page);
    }
    f.lost_headers = lost_now(page, live);

    /* stage 3: the damaged sane entries of the last walk and, in one pass over the ascending list, the suspects
     * that end at or before the next proven entry (kind 1 or 4) and start at or behind the last suspect kept
     *  */
    uint64_t nleft = 0;
    const uint64_t m = item_list(todo, &f.suspects, &f.suspects_kept);
    const int rc = crc32c_repair_items(page, PAGE, WBUF, todo, m, 0, ok, bit, &f.items_repaired, &nleft, 0, NULL);
    if (rc != CRC32C_OK) {
        fprintf(stderr, "crc32c_repair_items: %s\n", crc32c_strerror(rc));
        ++failures;
    }
    f.lost_items = lost_now(page, live);
    return f;
}

int main(int argc, char **argv) {
    int gpu = 0;
    for (int i = 1; i < argc; ++i)
        if (!strcmp(argv[i], "--gpu")) gpu = 1;
    crc32c_init();
    if (!gpu) {
        uint8_t buf[64] = {0}, kind1[1] = {9};
        uint64_t o1[1] = {9}, c[6] = {9, 9, 9, 9, 9, 9};
        uint32_t lens1[1] = {9};
        const int rc = crc32c_triage_pages(buf, sizeof buf, 64, o1, lens1, kind1, 1, &c[0], &c[1], &c[2], &c[3], &c[4],
                                           &c[5], 0, NULL);
        printf("triage_sim: no GPU, the triage reports %s\n", crc32c_strerror(rc));
        int same = kind1[0] == 9 && o1[0] == 9 && lens1[0] == 9;
        for (int i = 0; i < 6; ++i) same &= c[i] == 9;
        return rc == CRC32C_ENODEV && same ? 0 : 1;
    }
    uint8_t *page = malloc(PAGE), *pristine = malloc(PAGE), *old = malloc(PAGE);
    struct page_counts c;
    if (!page || !pristine || !old || page_build(page, pristine, DAMAGE_LENGTHS, &c) != 0) return 1;
    const uint64_t live = c.live;
    memcpy(old, page, PAGE);

    /* (suspects may overlap: their number is bounded by the candidates, not by the page's bytes over 50) */
    if (list_alloc(4 * (PAGE / 50) + NWBUF) != 0) return 1;
    todo = malloc((cap + NWBUF) * 8), bit = malloc((cap + NWBUF) * 8);
    hlens = malloc((cap + NWBUF) * 4), ok = malloc(cap + NWBUF);
    if (!todo || !bit || !hlens || !ok) return 1;

    /* the old flow over a copy of the damaged bytes, then the new one over the page */
    triage = 0;
    const struct flow was = play(old, live);
    triage = 1;
    const struct flow f = play(page, live);

    /* the sim's own count of what no rule can fix, from the pristine bytes; a rescued image is the one written */
    uint64_t c_multi = 0, c_length = 0, c_crlf = 0, first_dead[NWBUF];
    first_dead_of(first_dead);
    for (uint32_t id = 0; id < nitems; ++id) {
        if (where[id] == GONE) continue;
        const uint8_t *im = page + where[id], *was_b = pristine + where[id];
        if (rescued[id]) {
            if (memcmp(im + 28, was_b + 28, size_of[id] - 28) != 0) ++failures;
            continue;
        }
        uint64_t which = 0;
        const uint32_t nflipped = flipped_bits(im, was_b, size_of[id], &which);
        const int behind = at[id] > first_dead[at[id] / WBUF];
        if (nflipped >= 2) ++c_multi;
        else if (nflipped == 1 && behind && length_bit(which)) ++c_length;
        else if (nflipped == 1 && behind && which / 8 >= size_of[id] - 2) ++c_crlf;
        else ++failures; /* intact, one bit in front of every such header, or a suspect: it should have come back */
    }
    printf("triage_sim: %u items, %llu header-damaged, %llu with a length bit, %llu data-damaged, failures %d\n", nitems,
           (unsigned long long)c.ndamaged, (unsigned long long)c.nlen, (unsigned long long)c.ndata, failures);
    printf("live=%llu lost_old=%llu lost_recover=%llu lost_headers=%llu lost_triage=%llu headers_repaired=%llu "
           "items_repaired=%llu suspects=%llu suspects_kept=%llu rounds=%d unrepairable=%llu multi=%llu "
           "behind_length=%llu behind_crlf=%llu\n",
           (unsigned long long)live, (unsigned long long)was.lost_items, (unsigned long long)f.lost_recover,
           (unsigned long long)f.lost_headers, (unsigned long long)f.lost_items,
           (unsigned long long)f.headers_repaired, (unsigned long long)f.items_repaired,
           (unsigned long long)f.suspects, (unsigned long long)f.suspects_kept, f.rounds,
           (unsigned long long)(c_multi + c_length + c_crlf), (unsigned long long)c_multi,
           (unsigned long long)c_length, (unsigned long long)c_crlf);
    list_free(); free(todo); free(bit); free(hlens); free(ok);
    free(page);
    free(pristine);
    free(old);
    return failures == 0 ? 0 : 1;
}

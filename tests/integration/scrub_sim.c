/* scrub_sim.c -- triage_sim.c's read-back of a page with damaged headers and
 * damaged data (readback_page.h's page, DAMAGE_LENGTHS), played twice over the
 * same damaged bytes:
 *   the written-out flow  triage_sim.c's host loop: crc32c_triage_pages, rounds
 *                         of crc32c_repair_headers over the list of
 *                         INTEGRATION.md section 4f, crc32c_repair_items over
 *                         the list of section 4g, one call and two copies of
 *                         the lists a stage;
 *   the scrub             one crc32c_scrub_pages.
 * Each result's loss is counted by a read-back and rescue loop of its own over
 * its final list (kinds 0 and 6 skipped): crc32c_triage_pages for the
 * written-out flow, the list the scrub returned for the scrub.
 *
 * What no rule can fix is counted by the sim itself from the pristine bytes
 * and the layout it wrote, as triage_sim.c counts it.  Any other image that
 * does not come back from the scrub is a failure of the run, and so is a
 * rescued image that differs from its pristine bytes from byte 28, a logged
 * flip that is not in the page, or a page that differs from the damaged one
 * in any other bit.
 *
 * Usage: scrub_sim [--gpu]
 * Prints live=<l> lost_written_out=<a> lost_scrub=<b> calls_written_out=<c>
 * headers_repaired=<h> items_repaired=<i> rounds=<r> nflips=<f> complete=<0|1>
 * unrepairable=<u> multi=<x> behind_length=<y> behind_crlf=<z> (u = x + y + z).
 * Exit status 0 = the run itself worked; the caller judges the counts.
 * Without --gpu: the call must report CRC32C_ENODEV and write nothing.
 */
#include "readback_page.h"

static uint64_t *todo, *bit, *flip_offs, *flip_bits;
static uint32_t *hlens;
static uint8_t *ok, *flip_by;
static uint64_t calls; /* library calls of the written-out flow */

/* recover() with `triage` set, counted */
static void triage_again(uint8_t *page) {
    recover(page);
    ++calls;
}

/* triage_sim.c's host loop; returns with the final list in offs / lens / kind */
static void written_out(uint8_t *page) {
    triage_again(page);
    for (int rounds = 0; rounds < MAX_ROUNDS; ++rounds) {
        const uint64_t m = header_list(todo); /* INTEGRATION.md 4f */
        uint64_t nrep = 0, nleft = 0;
        const int rc = crc32c_repair_headers(page, PAGE, WBUF, todo, m, ok, bit, hlens, &nrep, &nleft, 0, NULL);
        ++calls;
        if (rc != CRC32C_OK) {
            fprintf(stderr, "crc32c_repair_headers: %s\n", crc32c_strerror(rc));
            ++failures;
            break;
        }
        if (nrep == 0) break;
        triage_again(page);
    }
    uint64_t nleft = 0, nrep = 0;
    const uint64_t m = item_list(todo, NULL, NULL); /* INTEGRATION.md 4g */
    const int rc = crc32c_repair_items(page, PAGE, WBUF, todo, m, 0, ok, bit, &nrep, &nleft, 0, NULL);
    ++calls;
    if (rc != CRC32C_OK) {
        fprintf(stderr, "crc32c_repair_items: %s\n", crc32c_strerror(rc));
        ++failures;
    }
    triage_again(page);
}

int main(int argc, char **argv) {
    int gpu = 0;
    for (int i = 1; i < argc; ++i)
        if (!strcmp(argv[i], "--gpu")) gpu = 1;
    crc32c_init();
    if (!gpu) {
        uint8_t buf[64] = {0}, kind1[1] = {9}, by1[1] = {9};
        uint64_t o1[1] = {9}, fo1[1] = {9}, fb1[1] = {9};
        uint32_t lens1[1] = {9};
        crc32c_scrub_out out, was;
        memset(&out, 0x5a, sizeof out);
        out.offsets = o1, out.lens = lens1, out.kind = kind1, out.cap = 1;
        out.flip_offsets = fo1, out.flip_bits = fb1, out.flip_by = by1, out.flip_cap = 1;
        was = out;
        const int rc = crc32c_scrub_pages(buf, sizeof buf, 64, NULL, &out);
        printf("scrub_sim: no GPU, the scrub reports %s\n", crc32c_strerror(rc));
        const int same = memcmp(&out, &was, sizeof out) == 0 && kind1[0] == 9 && by1[0] == 9 && o1[0] == 9 &&
                         fo1[0] == 9 && fb1[0] == 9 && lens1[0] == 9;
        return rc == CRC32C_ENODEV && same ? 0 : 1;
    }
    uint8_t *page = malloc(PAGE), *pristine = malloc(PAGE), *old = malloc(PAGE), *start = malloc(PAGE);
    struct page_counts c;
    if (!page || !pristine || !old || !start || page_build(page, pristine, DAMAGE_LENGTHS, &c) != 0) return 1;
    const uint64_t live = c.live;
    memcpy(old, page, PAGE);
    memcpy(start, page, PAGE);

    /* (suspects may overlap: their number is bounded by the candidates, not by the page's bytes over 50) */
    if (list_alloc(4 * (PAGE / 50) + NWBUF) != 0) return 1;
    todo = malloc((cap + NWBUF) * 8), bit = malloc((cap + NWBUF) * 8);
    hlens = malloc((cap + NWBUF) * 4), ok = malloc(cap + NWBUF);
    flip_offs = malloc(cap * 8), flip_bits = malloc(cap * 8), flip_by = malloc(cap);
    if (!todo || !bit || !hlens || !ok || !flip_offs || !flip_bits || !flip_by) return 1;

    /* the written-out flow over a copy of the damaged bytes ... */
    triage = 1;
    written_out(old);
    const uint64_t lost_written = lost_in_list(old, live);

    /* ... and one scrub over the page: its own list is the read-back */
    crc32c_scrub_out out;
    memset(&out, 0, sizeof out);
    out.offsets = offs, out.lens = lens, out.kind = kind, out.cap = cap;
    out.flip_offsets = flip_offs, out.flip_bits = flip_bits, out.flip_by = flip_by, out.flip_cap = cap;
    const int rc = crc32c_scrub_pages(page, PAGE, WBUF, NULL, &out);
    if (rc != CRC32C_OK || out.nitems > cap || out.nflips > cap) {
        fprintf(stderr, "crc32c_scrub_pages: %s\n", crc32c_strerror(rc));
        ++failures;
        out.nitems = out.nflips = 0;
    }
    n = out.nitems;
    const uint64_t lost_scrub = lost_in_list(page, live);
    /* the log is what changed: replayed on the damaged bytes it gives the page */
    for (uint64_t r = 0; r < out.nflips; ++r)
        start[flip_offs[r] + flip_bits[r] / 8] ^= (uint8_t)(1u << (flip_bits[r] % 8));
    if (memcmp(start, page, PAGE) != 0) ++failures;
    if (out.nflips != out.headers_repaired + out.items_repaired) ++failures;

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
    printf("scrub_sim: %u items, %llu header-damaged, %llu with a length bit, %llu data-damaged, failures %d\n", nitems,
           (unsigned long long)c.ndamaged, (unsigned long long)c.nlen, (unsigned long long)c.ndata, failures);
    printf("live=%llu lost_written_out=%llu lost_scrub=%llu calls_written_out=%llu headers_repaired=%llu "
           "items_repaired=%llu rounds=%u nflips=%llu complete=%u unrepairable=%llu multi=%llu behind_length=%llu "
           "behind_crlf=%llu\n",
           (unsigned long long)live, (unsigned long long)lost_written, (unsigned long long)lost_scrub,
           (unsigned long long)calls, (unsigned long long)out.headers_repaired,
           (unsigned long long)out.items_repaired, out.rounds, (unsigned long long)out.nflips, out.complete,
           (unsigned long long)(c_multi + c_length + c_crlf), (unsigned long long)c_multi,
           (unsigned long long)c_length, (unsigned long long)c_crlf);
    list_free(); free(todo); free(bit); free(hlens); free(ok);
    free(flip_offs); free(flip_bits); free(flip_by);
    free(page);
    free(pristine);
    free(old);
    free(start);
    return failures == 0 ? 0 : 1;
}

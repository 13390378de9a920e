/* gaps_sim.c -- scrub_sim.c's page (readback_page.h's, DAMAGE_LENGTHS)
 * through two crc32c_scrub_pages over the same damaged bytes in one run: one
 * without CRC32C_SCRUB_GAPS and one with it.  Each result's loss is counted by
 * the rescue loop over the list the call returned (kinds 0 and 6 skipped).
 *
 * What the rule cannot fix is counted by the sim itself from the pristine
 * bytes and the layout it wrote, image by image in layout order per wbuf.  An
 * image is lost when
 *   it has two or more flipped bits, or
 *   it is a dead header (nkey zeroed), or
 *   it has one length bit or one bit of its final CRLF flipped, lies behind
 *     its wbuf's first dead header, and the image in front of it is itself
 *     lost (a gap start is the end of a proven image);
 * every other image comes back, the ones off the hash table too (they are the
 * proven images in front of others).  Without the bit the third case loses the
 * image whatever lies in front of it (scrub_sim.c's count).  A live image that
 * does not come back although the sim's count says it does is a failure of the
 * run, and so is a rescued image that differs from its pristine bytes from
 * byte 28, a logged flip that is not in the page, or a page that differs from
 * the damaged one in any other bit.
 *
 * Usage: gaps_sim [--gpu]
 * Prints live=<l> lost_scrub=<a> unrepairable_scrub=<u> lost_gaps=<b>
 * unrepairable_gaps=<v> multi=<x> dead=<d> behind_lost=<y> rounds_scrub=<r>
 * rounds_gaps=<s> headers_repaired=<h> items_repaired=<i> nflips=<f>
 * complete=<0|1> (v = x + d + y counts live images; u = scrub_sim.c's).
 * Exit status 0 = the run itself worked; the caller judges the counts.
 * Without --gpu: the call with the bit must report CRC32C_ENODEV and write
 * nothing.
 */
#include "readback_page.h"

static uint64_t *flip_offs, *flip_bits;
static uint8_t *flip_by;

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
        crc32c_scrub_opts opts;
        memset(&opts, 0, sizeof opts);
        opts.mode = CRC32C_SCRUB_GAPS;
        const int rc = crc32c_scrub_pages(buf, sizeof buf, 64, &opts, &out);
        printf("gaps_sim: no GPU, the scrub reports %s\n", crc32c_strerror(rc));
        const int same = memcmp(&out, &was, sizeof out) == 0 && kind1[0] == 9 && by1[0] == 9 && o1[0] == 9 &&
                         fo1[0] == 9 && fb1[0] == 9 && lens1[0] == 9;
        return rc == CRC32C_ENODEV && same ? 0 : 1;
    }
    uint8_t *page = malloc(PAGE), *pristine = malloc(PAGE), *old = malloc(PAGE), *damaged_bytes = malloc(PAGE);
    struct page_counts c;
    if (!page || !pristine || !old || !damaged_bytes || page_build(page, pristine, DAMAGE_LENGTHS, &c) != 0) return 1;
    const uint64_t live = c.live;
    memcpy(old, page, PAGE);
    memcpy(damaged_bytes, page, PAGE);

    /* (suspects may overlap: their number is bounded by the candidates, not by the page's bytes over 50) */
    if (list_alloc(4 * (PAGE / 50) + NWBUF) != 0) return 1;
    flip_offs = malloc(cap * 8), flip_bits = malloc(cap * 8), flip_by = malloc(cap);
    if (!flip_offs || !flip_bits || !flip_by) return 1;

    /* the sim's own count, from the pristine bytes and the layout (ids are in layout order) */
    static uint8_t back_scrub[MAX_ITEMS], back_gaps[MAX_ITEMS]; /* the image is proven at the end */
    uint64_t c_multi = 0, c_dead = 0, c_behind = 0, u_scrub = 0, first_dead[NWBUF];
    first_dead_of(first_dead);
    for (uint32_t id = 0; id < nitems; ++id) {
        const uint8_t *im = page + at[id], *was_b = pristine + at[id];
        const int is_live = where[id] != GONE;
        uint64_t which = 0;
        const uint32_t nflipped = flipped_bits(im, was_b, size_of[id], &which);
        const int behind = at[id] > first_dead[at[id] / WBUF];
        const int edge = nflipped == 1 && behind && (length_bit(which) || which / 8 >= size_of[id] - 2);
        const int front = id > 0 && at[id - 1] / WBUF == at[id] / WBUF && at[id - 1] + size_of[id - 1] == at[id] &&
                          back_gaps[id - 1];
        back_scrub[id] = !dead[id] && nflipped < 2 && !edge;
        back_gaps[id] = !dead[id] && nflipped < 2 && (!edge || front);
        if (!is_live) continue;
        u_scrub += !back_scrub[id];
        if (dead[id]) ++c_dead;
        else if (nflipped >= 2) ++c_multi;
        else if (!back_gaps[id]) ++c_behind;
    }

    /* one scrub without the bit over a copy, one with it over the page: each list is its own read-back */
    uint64_t lost[2] = {0, 0};
    uint32_t rounds[2] = {0, 0};
    crc32c_scrub_out out;
    for (int g = 0; g < 2; ++g) {
        uint8_t *p = g ? page : old;
        crc32c_scrub_opts opts;
        memset(&opts, 0, sizeof opts);
        opts.mode = g ? CRC32C_SCRUB_GAPS : 0;
        memset(&out, 0, sizeof out);
        out.offsets = offs, out.lens = lens, out.kind = kind, out.cap = cap;
        out.flip_offsets = flip_offs, out.flip_bits = flip_bits, out.flip_by = flip_by, out.flip_cap = cap;
        const int rc = crc32c_scrub_pages(p, PAGE, WBUF, &opts, &out);
        if (rc != CRC32C_OK || out.nitems > cap || out.nflips > cap) {
            fprintf(stderr, "crc32c_scrub_pages: %s\n", crc32c_strerror(rc));
            ++failures;
            out.nitems = out.nflips = 0;
        }
        n = out.nitems;
        lost[g] = lost_in_list(p, live);
        rounds[g] = out.rounds;
        /* the log is what changed: replayed on the damaged bytes it gives the page */
            if (out.nflips != out.headers_repaired + out.items_repaired || out.complete != 1) ++failures;
        /* what came back against the sim's count, and against the pristine bytes */
        const uint8_t *back = g ? back_gaps : back_scrub;
        for (uint32_t id = 0; id < nitems; ++id) {
            if (where[id] == GONE) continue;
            if (rescued[id] != back[id]) ++failures;
            if (rescued[id] && memcmp(p + where[id] + 28, pristine + where[id] + 28, size_of[id] - 28) != 0) ++failures;
        }
    }
    /* the last call's log replayed on the damaged bytes gives the page (old is repaired too: the damaged bytes are
     * kept in `damaged_bytes`) */
    for (uint64_t r = 0; r < out.nflips; ++r)
        damaged_bytes[flip_offs[r] + flip_bits[r] / 8] ^= (uint8_t)(1u << (flip_bits[r] % 8));
    if (memcmp(damaged_bytes, page, PAGE) != 0) ++failures;

    printf("gaps_sim: %u items, %llu header-damaged, %llu with a length bit, %llu data-damaged, failures %d\n", nitems,
           (unsigned long long)c.ndamaged, (unsigned long long)c.nlen, (unsigned long long)c.ndata, failures);
    printf("live=%llu lost_scrub=%llu unrepairable_scrub=%llu lost_gaps=%llu unrepairable_gaps=%llu multi=%llu "
           "dead=%llu behind_lost=%llu rounds_scrub=%u rounds_gaps=%u headers_repaired=%llu items_repaired=%llu "
           "nflips=%llu complete=%u\n",
           (unsigned long long)live, (unsigned long long)lost[0], (unsigned long long)u_scrub,
           (unsigned long long)lost[1], (unsigned long long)(c_multi + c_dead + c_behind),
           (unsigned long long)c_multi, (unsigned long long)c_dead, (unsigned long long)c_behind, rounds[0], rounds[1],
           (unsigned long long)out.headers_repaired, (unsigned long long)out.items_repaired,
           (unsigned long long)out.nflips, out.complete);
    list_free();
    free(flip_offs); free(flip_bits); free(flip_by);
    free(page);
    free(pristine);
    free(old);
    free(damaged_bytes);
    return failures == 0 ? 0 : 1;
}

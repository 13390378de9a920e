/* scrub_bytes_sim.c -- bytes_sim.c's page (readback_page.h's, DAMAGE_BYTES:
 * every tenth data-damaged image has two bits of one byte inverted) through
 * two crc32c_scrub_pages over the same damaged bytes in one run: one with
 * CRC32C_SCRUB_GAPS and one with CRC32C_SCRUB_GAPS | CRC32C_SCRUB_BYTES.  Each
 * result's loss is counted by the rescue loop over the list the call returned
 * (kinds 0 and 6 skipped).
 *
 * No number is fixed in advance.  The run counts, and the caller judges:
 *   by_byte / by_byte_wrong   the images the second run logs
 *       CRC32C_SCRUB_BY_BYTE, and those of them that are no image the sim
 *       wrote or differ from their pristine bytes afterwards;
 *   named / named_rescued     the images with two bits of one byte inverted
 *       (damaged[id] == 3) that the first run's final list names for the item
 *       stage (kind 0 with a length, or a suspect the filter keeps), and those
 *       of them the second run rescues;
 *   regressed                 images the first run rescued and the second
 *       does not.
 * A failure of the run itself: a call that fails, a second log that does not
 * replay to the page, an items_repaired that is not the CRC32C_SCRUB_BY_ITEM
 * entries plus the distinct CRC32C_SCRUB_BY_BYTE offsets, a first run whose
 * log holds a CRC32C_SCRUB_BY_BYTE entry, a run that does not end complete.
 *
 * Usage: scrub_bytes_sim [--gpu]
 * Prints live=<l> lost_gaps=<a> lost_bytes=<b> rounds_gaps=<r> rounds_bytes=<s>
 * by_byte=<n> by_byte_wrong=<w> named=<m> named_rescued=<k> regressed=<g>
 * nflips=<f> items_repaired=<i> samebyte=<x>.  Exit status 0 = the run itself
 * worked.  Without --gpu: the call with both bits must report CRC32C_ENODEV and
 * write nothing.
 */
#include "readback_page.h"

static uint64_t *flip_offs, *flip_bits;
static uint8_t *flip_by;

static uint32_t id_at(uint64_t off) {
    for (uint32_t id = 0; id < nitems; ++id)
        if (at[id] == off) return id;
    return UINT32_MAX;
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
        crc32c_scrub_opts opts;
        memset(&opts, 0, sizeof opts);
        opts.mode = CRC32C_SCRUB_GAPS | CRC32C_SCRUB_BYTES;
        const int rc = crc32c_scrub_pages(buf, sizeof buf, 64, &opts, &out);
        printf("scrub_bytes_sim: no GPU, the scrub reports %s\n", crc32c_strerror(rc));
        const int same = memcmp(&out, &was, sizeof out) == 0 && kind1[0] == 9 && by1[0] == 9 && o1[0] == 9 &&
                         fo1[0] == 9 && fb1[0] == 9 && lens1[0] == 9;
        return rc == CRC32C_ENODEV && same ? 0 : 1;
    }
    uint8_t *page = malloc(PAGE), *pristine = malloc(PAGE), *old = malloc(PAGE), *damaged_bytes = malloc(PAGE);
    struct page_counts c;
    if (!page || !pristine || !old || !damaged_bytes || page_build(page, pristine, DAMAGE_BYTES, &c) != 0) return 1;
    const uint64_t live = c.live;
    memcpy(old, page, PAGE);
    memcpy(damaged_bytes, page, PAGE);

    /* (suspects may overlap: their number is bounded by the candidates, not by the page's bytes over 50) */
    if (list_alloc(4 * (PAGE / 50) + NWBUF) != 0) return 1;
    flip_offs = malloc(cap * 8), flip_bits = malloc(cap * 8), flip_by = malloc(cap);
    uint64_t *todo = malloc(cap * 8);
    if (!flip_offs || !flip_bits || !flip_by || !todo) return 1;

    static uint8_t first_rescued[MAX_ITEMS], named[MAX_ITEMS];
    uint64_t lost[2] = {0, 0}, by_byte = 0, by_byte_wrong = 0, c_named = 0, c_named_rescued = 0, regressed = 0;
    uint32_t rounds[2] = {0, 0};
    crc32c_scrub_out out;
    for (int g = 0; g < 2; ++g) {
        uint8_t *p = g ? page : old;
        crc32c_scrub_opts opts;
        memset(&opts, 0, sizeof opts);
        opts.mode = CRC32C_SCRUB_GAPS | (g ? CRC32C_SCRUB_BYTES : 0);
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
        if (out.complete != 1) ++failures;
        /* the log's stages: items_repaired is the item stage's entries and the byte stage's distinct images */
        uint64_t n_item = 0, n_byte_images = 0, last = UINT64_MAX;
        for (uint64_t r = 0; r < out.nflips; ++r) {
            n_item += flip_by[r] == CRC32C_SCRUB_BY_ITEM;
            if (flip_by[r] != CRC32C_SCRUB_BY_BYTE) {
                last = UINT64_MAX;
                continue;
            }
            if (!g) ++failures; /* (the bit was clear) */
            if (flip_offs[r] == last) continue; /* (an image's bits are consecutive entries) */
            last = flip_offs[r];
            ++n_byte_images;
            const uint32_t id = id_at(last);
            if (id == UINT32_MAX || memcmp(p + last, pristine + last, size_of[id]) != 0) ++by_byte_wrong;
        }
        if (out.items_repaired != n_item + n_byte_images) ++failures;
        if (!g) {
            if (out.nflips != out.headers_repaired + out.items_repaired) ++failures;
            memcpy(first_rescued, rescued, sizeof rescued);
            /* what the first run's final list hands to the item stage, and so would hand to the byte stage */
            const uint64_t m = item_list(todo, NULL, NULL);
            for (uint64_t k = 0; k < m; ++k) {
                const uint32_t id = id_at(todo[k]);
                if (id != UINT32_MAX && where[id] != GONE && damaged[id] == 3) named[id] = 1;
            }
        } else {
            by_byte = n_byte_images;
            for (uint32_t id = 0; id < nitems; ++id) {
                c_named += named[id];
                c_named_rescued += named[id] && rescued[id];
                regressed += first_rescued[id] && !rescued[id];
                if (rescued[id] && memcmp(p + where[id] + 28, pristine + where[id] + 28, size_of[id] - 28) != 0)
                    ++failures;
            }
        }
    }
    /* the second call's log replayed on the damaged bytes gives the page */
    for (uint64_t r = 0; r < out.nflips; ++r)
        damaged_bytes[flip_offs[r] + flip_bits[r] / 8] ^= (uint8_t)(1u << (flip_bits[r] % 8));
    if (memcmp(damaged_bytes, page, PAGE) != 0) ++failures;

    printf("scrub_bytes_sim: %u items, %llu header-damaged, %llu data-damaged (%llu in one byte twice, %llu in two "
           "bytes), failures %d\n",
           nitems, (unsigned long long)c.ndamaged, (unsigned long long)c.ndata, (unsigned long long)c.nsame,
           (unsigned long long)c.ntwo, failures);
    printf("live=%llu lost_gaps=%llu lost_bytes=%llu rounds_gaps=%u rounds_bytes=%u by_byte=%llu by_byte_wrong=%llu "
           "named=%llu named_rescued=%llu regressed=%llu nflips=%llu items_repaired=%llu samebyte=%llu\n",
           (unsigned long long)live, (unsigned long long)lost[0], (unsigned long long)lost[1], rounds[0], rounds[1],
           (unsigned long long)by_byte, (unsigned long long)by_byte_wrong, (unsigned long long)c_named,
           (unsigned long long)c_named_rescued, (unsigned long long)regressed, (unsigned long long)out.nflips,
           (unsigned long long)out.items_repaired, (unsigned long long)c.nsame);
    list_free();
    free(flip_offs); free(flip_bits); free(flip_by); free(todo);
    free(page);
    free(pristine);
    free(old);
    free(damaged_bytes);
    return failures == 0 ? 0 : 1;
}

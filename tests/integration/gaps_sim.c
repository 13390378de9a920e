/* gaps_sim.c -- scrub_sim.c's page (triage_sim.c's generator, seeds and damage)
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
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "crc32c.h"
#include "crc32c_batch.h"

#define WBUF (1u << 20)
#define NWBUF 8u
#define PAGE (NWBUF * WBUF)
#define MAX_ITEMS 8000u
#define ITEM_CAS 2u
#define MAX_VALUE 3000u
#define MAX_IMG (48 + 16 + 8 + MAX_VALUE + 2)
#define GONE UINT64_MAX

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

static uint64_t where[MAX_ITEMS]; /* the hash table: page offset of each live item's image, or GONE */
static uint32_t size_of[MAX_ITEMS]; /* the ITEM_ntotal each image was written with */
static uint64_t at[MAX_ITEMS];     /* where each image was written, live or not */
static uint8_t damaged[MAX_ITEMS], rescued[MAX_ITEMS], dead[MAX_ITEMS]; /* dead: nkey zeroed */
static uint32_t nitems;

/* storage.c:964-975: the image's key, looked up, must be linked to exactly
 * this offset (`room`: the image's bytes) */
static int rescue(const uint8_t *page, uint64_t off, uint64_t room) {
    const uint8_t *im = page + off;
    uint16_t flags;
    memcpy(&flags, im + 38, 2);
    const uint32_t nkey = im[41], koff = 48 + ((flags & ITEM_CAS) ? 8 : 0);
    char key[16];
    if (nkey != 10 || koff + nkey > room) return 0;
    memcpy(key, im + koff, nkey);
    key[nkey] = 0;
    if (strncmp(key, "key", 3) != 0) return 0;
    char *end = NULL;
    const unsigned long id = strtoul(key + 3, &end, 10);
    if (*end || id >= nitems || where[id] != off || rescued[id]) return 0;
    rescued[id] = 1;
    return 1;
}

/* the 42 length bits (crc32c_batch.h), by image bit index */
static uint32_t length_bit_of(uint32_t v) { return v < 32 ? 256 + v : v < 40 ? 328 + (v - 32) : v == 40 ? 305 : 312; }
static int length_bit(uint64_t k) {
    const uint64_t by = k / 8, b = k % 8;
    return (by >= 32 && by <= 35) || by == 41 || (by == 38 && b == 1) || (by == 39 && b == 0);
}

static uint64_t *offs, *flip_offs, *flip_bits;
static uint32_t *lens;
static uint8_t *kind, *flip_by;
static uint64_t cap, n;
static int failures;

/* the rescue loop over the list in offs / lens / kind: the live items lost */
static uint64_t lost_in_list(const uint8_t *page, uint64_t live) {
    memset(rescued, 0, sizeof rescued);
    uint64_t got = 0;
    for (uint64_t k = 0; k < n; ++k)
        if (kind[k] != 0 && kind[k] != CRC32C_ITEM_SUSPECT) got += (uint64_t)rescue(page, offs[k], lens[k]);
    return live - got;
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
        opts.mode = CRC32C_SCRUB_GAPS;
        const int rc = crc32c_scrub_pages(buf, sizeof buf, 64, &opts, &out);
        printf("gaps_sim: no GPU, the scrub reports %s\n", crc32c_strerror(rc));
        const int same = memcmp(&out, &was, sizeof out) == 0 && kind1[0] == 9 && by1[0] == 9 && o1[0] == 9 &&
                         fo1[0] == 9 && fb1[0] == 9 && lens1[0] == 9;
        return rc == CRC32C_ENODEV && same ? 0 : 1;
    }
    uint8_t *page = calloc(PAGE, 1), *pristine = malloc(PAGE), *old = malloc(PAGE), *damaged_bytes = malloc(PAGE);
    static uint8_t img[MAX_IMG];
    if (!page || !pristine || !old || !damaged_bytes) return 1;
    uint64_t rng = 41;

    /* fill the page through wbufs: an image never crosses one, tails stay zero */
    uint64_t used = 0;
    for (;; ++nitems) {
        const uint32_t nt = make_image(img, nitems, &rng);
        if (used % WBUF + nt > WBUF) used = (used / WBUF + 1) * WBUF;
        if (used >= PAGE) break;
        if (nitems >= MAX_ITEMS) {
            fprintf(stderr, "item table too small\n");
            return 1;
        }
        memcpy(page + used, img, nt);
        where[nitems] = at[nitems] = used;
        size_of[nitems] = nt;
        used += nt;
    }
    memcpy(pristine, page, PAGE);

    /* the live set, and the damage "on flash": one header bit of every 37th live image (recover_sim.c's) */
    uint64_t live = 0, ndamaged = 0;
    for (uint32_t id = 0; id < nitems; ++id) {
        if (mix(&rng) % 5 >= 2) {
            where[id] = GONE;
            continue;
        }
        if (live++ % 37 == 11) {
            uint8_t *im = page + where[id];
            switch (ndamaged % 3) {
                case 0: im[41] = 0; dead[id] = 1; break;                     /* nkey: ends the walk */
                case 1: im[32 + mix(&rng) % 2] ^= (uint8_t)(1u << (mix(&rng) % 8)); break; /* nbytes */
                default: im[38] ^= ITEM_CAS; break;                          /* it_flags */
            }
            damaged[id] = 1;
            ++ndamaged;
        }
    }
    /* ... one of the 42 length bits of every 11th of the other live images; of the rest every 7th one bit of the
     * stored CRC or the bytes it covers (no length bit), every fifth of those a second one */
    uint64_t rng2 = 77, nth = 0, nlen = 0, ndata = 0;
    for (uint32_t id = 0; id < nitems; ++id) {
        if (where[id] == GONE || damaged[id]) continue;
        uint8_t *im = page + where[id];
        const uint64_t turn = nth++;
        if (turn % 11 == 5) {
            const uint32_t k = length_bit_of((uint32_t)(mix(&rng2) % CRC32C_HEADER_BITS));
            im[k / 8] ^= (uint8_t)(1u << (k % 8));
            damaged[id] = 3;
            ++nlen;
        } else if (turn % 7 == 3) {
            const uint64_t nbits = 8ull * size_of[id] - 224;
            uint64_t k1;
            do k1 = 224 + mix(&rng2) % nbits; while (length_bit(k1));
            im[k1 / 8] ^= (uint8_t)(1u << (k1 % 8));
            if (ndata % 5 == 4) {
                uint64_t k2;
                do k2 = 224 + mix(&rng2) % nbits; while (length_bit(k2) || k2 == k1);
                im[k2 / 8] ^= (uint8_t)(1u << (k2 % 8));
            }
            damaged[id] = 2;
            ++ndata;
        }
    }
    memcpy(old, page, PAGE);
    memcpy(damaged_bytes, page, PAGE);

    /* (suspects may overlap: their number is bounded by the candidates, not by the page's bytes over 50) */
    cap = 4 * (PAGE / 50) + NWBUF;
    offs = malloc(cap * 8), lens = malloc(cap * 4), kind = malloc(cap);
    flip_offs = malloc(cap * 8), flip_bits = malloc(cap * 8), flip_by = malloc(cap);
    if (!offs || !lens || !kind || !flip_offs || !flip_bits || !flip_by) return 1;

    /* the sim's own count, from the pristine bytes and the layout (ids are in layout order) */
    static uint8_t back_scrub[MAX_ITEMS], back_gaps[MAX_ITEMS]; /* the image is proven at the end */
    uint64_t c_multi = 0, c_dead = 0, c_behind = 0, u_scrub = 0, first_dead[NWBUF];
    for (uint32_t w = 0; w < NWBUF; ++w) first_dead[w] = UINT64_MAX; /* the wbuf's first header no rule fixes */
    for (uint32_t id = 0; id < nitems; ++id)
        if (dead[id] && at[id] < first_dead[at[id] / WBUF]) first_dead[at[id] / WBUF] = at[id];
    for (uint32_t id = 0; id < nitems; ++id) {
        const uint8_t *im = page + at[id], *was_b = pristine + at[id];
        const int is_live = where[id] != GONE;
        uint32_t nflipped = 0;
        uint64_t which = 0;
        for (uint32_t b = 28; b < size_of[id]; ++b)
            for (uint32_t i = 0; i < 8; ++i)
                if ((im[b] ^ was_b[b]) >> i & 1) {
                    ++nflipped;
                    which = 8ull * b + i;
                }
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
           (unsigned long long)ndamaged, (unsigned long long)nlen, (unsigned long long)ndata, failures);
    printf("live=%llu lost_scrub=%llu unrepairable_scrub=%llu lost_gaps=%llu unrepairable_gaps=%llu multi=%llu "
           "dead=%llu behind_lost=%llu rounds_scrub=%u rounds_gaps=%u headers_repaired=%llu items_repaired=%llu "
           "nflips=%llu complete=%u\n",
           (unsigned long long)live, (unsigned long long)lost[0], (unsigned long long)u_scrub,
           (unsigned long long)lost[1], (unsigned long long)(c_multi + c_dead + c_behind),
           (unsigned long long)c_multi, (unsigned long long)c_dead, (unsigned long long)c_behind, rounds[0], rounds[1],
           (unsigned long long)out.headers_repaired, (unsigned long long)out.items_repaired,
           (unsigned long long)out.nflips, out.complete);
    free(offs); free(lens); free(kind);
    free(flip_offs); free(flip_bits); free(flip_by);
    free(page);
    free(pristine);
    free(old);
    free(damaged_bytes);
    return failures == 0 ? 0 : 1;
}

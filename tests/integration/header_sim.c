/* header_sim.c -- storage_compact_readback over a page with damaged headers and
 * damaged data, through crc32c_recover_pages, crc32c_repair_headers and
 * crc32c_repair_items (INTEGRATION.md sections 4e and 4f): recover_sim.c's page
 * and header damage (the same generator and seed), with single length bits and
 * data bits flipped inside other live images added to it.
 *
 * The flow over the bytes, each stage's loss counted by a read-back and rescue
 * loop of its own (crc32c_recover_pages, kind 0 skipped):
 *   recover   crc32c_recover_pages alone;
 *   headers   the list of INTEGRATION.md 4f (every kind 0 entry, every wbuf's
 *             walk end that is no entry) given to crc32c_repair_headers, the
 *             page walked again, and so on while a round repairs a header: a
 *             wbuf's walk reaches its second damaged header only when the
 *             first one is right;
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
#define MAX_ROUNDS 64

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

static uint64_t *offs, *todo, *bit;
static uint32_t *lens, *hlens;
static uint8_t *kind, *ok;
static uint64_t cap, n;
static int failures;

static void recover(uint8_t *page) {
    uint64_t nbad = 0, nsalvaged = 0;
    const int rc = crc32c_recover_pages(page, PAGE, WBUF, offs, lens, kind, cap, &n, &nbad, &nsalvaged, NULL, NULL, 0, NULL);
    if (rc != CRC32C_OK || n > cap) {
        fprintf(stderr, "crc32c_recover_pages: %s\n", crc32c_strerror(rc));
        ++failures;
        n = 0;
    }
}

/* one read-back and rescue loop: the live items lost */
static uint64_t lost_now(uint8_t *page, uint64_t live) {
    memset(rescued, 0, sizeof rescued);
    recover(page);
    uint64_t got = 0;
    for (uint64_t k = 0; k < n; ++k)
        if (kind[k] != 0) got += (uint64_t)rescue(page, offs[k], lens[k]);
    return live - got;
}

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
    uint8_t *page = calloc(PAGE, 1), *pristine = malloc(PAGE);
    static uint8_t img[MAX_IMG];
    if (!page || !pristine) return 1;
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

    cap = 2 * (PAGE / 50) + NWBUF;
    offs = malloc(cap * 8), todo = malloc((cap + NWBUF) * 8), bit = malloc((cap + NWBUF) * 8);
    lens = malloc(cap * 4), hlens = malloc((cap + NWBUF) * 4);
    kind = malloc(cap), ok = malloc(cap + NWBUF);
    if (!offs || !todo || !bit || !lens || !hlens || !kind || !ok) return 1;

    /* stage 1: crc32c_recover_pages alone */
    const uint64_t lost_recover = lost_now(page, live);

    /* stage 2: the headers, round by round (lost_now left the walk's lists behind) */
    uint64_t headers_repaired = 0;
    int rounds = 0;
    for (; rounds < MAX_ROUNDS; ++rounds) {
        uint64_t m = 0, k = 0;
        for (uint64_t w = 0; w * WBUF < PAGE; ++w) { /* INTEGRATION.md 4f */
            const uint64_t ps = w * WBUF, pe = ps + WBUF < PAGE ? ps + WBUF : PAGE;
            uint64_t end = ps;
            int last = -1;
            for (; k < n && offs[k] < pe; ++k) {
                if (kind[k] == CRC32C_ITEM_SALVAGED) continue;
                if (kind[k] == 0) todo[m++] = offs[k];
                last = kind[k];
                end = offs[k] + lens[k];
            }
            if (last != 0 && end >= ps && end <= pe && pe - end >= 48) todo[m++] = end;
        }
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
    uint64_t m = 0, items_repaired = 0, nleft = 0;
    for (uint64_t k = 0; k < n; ++k)
        if (kind[k] == 0 && lens[k] != 0) todo[m++] = offs[k];
    int rc = crc32c_repair_items(page, PAGE, WBUF, todo, m, 0, ok, bit, &items_repaired, &nleft, 0, NULL);
    if (rc != CRC32C_OK) {
        fprintf(stderr, "crc32c_repair_items: %s\n", crc32c_strerror(rc));
        ++failures;
    }
    const uint64_t lost_items = lost_now(page, live);

    /* the sim's own count of what no rule can fix, from the pristine bytes; a rescued image is the one written */
    uint64_t c_multi = 0, c_behind = 0, first_dead[NWBUF];
    for (uint32_t w = 0; w < NWBUF; ++w) first_dead[w] = UINT64_MAX; /* the wbuf's first header no rule fixes */
    for (uint32_t id = 0; id < nitems; ++id)
        if (dead[id] && at[id] < first_dead[at[id] / WBUF]) first_dead[at[id] / WBUF] = at[id];
    for (uint32_t id = 0; id < nitems; ++id) {
        if (where[id] == GONE) continue;
        const uint8_t *im = page + where[id], *was = pristine + where[id];
        if (rescued[id]) {
            if (memcmp(im + 28, was + 28, size_of[id] - 28) != 0) ++failures;
            continue;
        }
        uint32_t nflipped = 0;
        for (uint32_t b = 28; b < size_of[id]; ++b) nflipped += (uint32_t)__builtin_popcount(im[b] ^ was[b]);
        if (nflipped >= 2) ++c_multi;
        else if (nflipped == 1 && at[id] > first_dead[at[id] / WBUF]) ++c_behind;
        else ++failures; /* intact, or one bit in front of every such header: it should have come back */
    }
    printf("header_sim: %u items, %llu header-damaged, %llu with a length bit, %llu data-damaged, failures %d\n", nitems,
           (unsigned long long)ndamaged, (unsigned long long)nlen, (unsigned long long)ndata, failures);
    printf("live=%llu lost_recover=%llu lost_headers=%llu lost_items=%llu headers_repaired=%llu items_repaired=%llu "
           "rounds=%d unrepairable=%llu multi=%llu behind=%llu\n",
           (unsigned long long)live, (unsigned long long)lost_recover, (unsigned long long)lost_headers,
           (unsigned long long)lost_items, (unsigned long long)headers_repaired, (unsigned long long)items_repaired,
           rounds, (unsigned long long)(c_multi + c_behind), (unsigned long long)c_multi,
           (unsigned long long)c_behind);
    free(offs); free(todo); free(bit); free(lens); free(hlens); free(kind); free(ok);
    free(page);
    free(pristine);
    return failures == 0 ? 0 : 1;
}

/* readback_page.h -- the page, the damage and the rescue check that the
 * read-back sims share (salvage_sim.c, recover_sim.c, repair_sim.c,
 * header_sim.c, triage_sim.c, scrub_sim.c, gaps_sim.c, bytes_sim.c), so that
 * "the same page and the same damage" holds by construction.
 * readback_page_check.c pins the bytes each damage profile gives.
 *
 * The setting.  storage_compact_readback (storage.c:950-1072) walks each wbuf
 * of the page it read back from its first byte, image to image by ITEM_ntotal,
 * until nkey == 0 or fewer than 48 bytes are left, and rescues an image only
 * when its key is still linked to exactly this page and offset
 * (storage.c:964-975).  The sims fill a page of 8 wbufs with stamped images,
 * keep a key -> offset table as the hash table, mark two fifths of the items
 * live, damage live images "on flash" and play the read-back over the result.
 *
 * Each sim is one translation unit: the state here is file-scope static and
 * the functions are static inline, so a sim takes what it needs.  A sim may
 * define MAX_VALUE before the include.  The order and number of mix() draws
 * is part of the page: change none.
 */
#ifndef READBACK_PAGE_H
#define READBACK_PAGE_H

#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "crc32c.h"
#include "crc32c_batch.h"

/* ---- primitives ---- */

#define WBUF (1u << 20)
#define NWBUF 8u
#define PAGE (NWBUF * WBUF)
#define MAX_ITEMS 8000u
#define ITEM_CAS 2u
#ifndef MAX_VALUE
#define MAX_VALUE 3000u
#endif
#define MAX_IMG (48 + 16 + 8 + MAX_VALUE + 2)
#define GONE UINT64_MAX
#define MAX_ROUNDS 64

static inline uint32_t rd32(const uint8_t *p) { uint32_t v; memcpy(&v, p, 4); return v; }

static inline uint64_t ntotal_of(const uint8_t *p) {
    uint16_t flags;
    memcpy(&flags, p + 38, 2);
    return 48ull + p[41] + 1 + rd32(p + 32) + ((flags & 256u) ? 4 : 0) + ((flags & ITEM_CAS) ? 8 : 0);
}

static inline uint64_t mix(uint64_t *s) { /* splitmix64 */
    uint64_t z = (*s += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}

/* an item image as storage_write leaves it, CRC stored (storage.c:567) */
static inline uint32_t make_image(uint8_t *img, uint32_t id, uint64_t *rng) {
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

/* the 42 length-determining header bits (crc32c_batch.h): the v-th of them by image bit index, whether image bit k
 * is one, and whether a byte's mask holds one */
static inline uint32_t length_bit_of(uint32_t v) {
    return v < 32 ? 256 + v : v < 40 ? 328 + (v - 32) : v == 40 ? 305 : 312;
}
static inline int length_bit(uint64_t k) {
    const uint64_t by = k / 8, b = k % 8;
    return (by >= 32 && by <= 35) || by == 41 || (by == 38 && b == 1) || (by == 39 && b == 0);
}
static inline int length_mask(uint64_t by, uint8_t m) {
    for (unsigned b = 0; b < 8; ++b)
        if ((m >> b & 1) && length_bit(8 * by + b)) return 1;
    return 0;
}

static inline void flip(uint8_t *im, uint64_t k) { im[k / 8] ^= (uint8_t)(1u << (k % 8)); }

/* ---- the page ---- */

static uint64_t where[MAX_ITEMS];   /* the hash table: page offset of each live item's image, or GONE */
static uint32_t size_of[MAX_ITEMS]; /* the ITEM_ntotal each image was written with */
static uint64_t at[MAX_ITEMS];      /* where each image was written, live or not */
/* damaged: 0 intact, 1 header bit of the first pass; of the second pass 2 one data bit (or two, DAMAGE_BITS and
 * DAMAGE_LENGTHS), 3 a length bit (DAMAGE_LENGTHS) or two bits of one byte (DAMAGE_BYTES), 4 bits of two bytes */
static uint8_t damaged[MAX_ITEMS], rescued[MAX_ITEMS], listed[MAX_ITEMS], dead[MAX_ITEMS]; /* dead: nkey zeroed */
static uint32_t nitems;

/* the second damage pass */
enum {
    DAMAGE_HEADERS, /* none: salvage_sim.c, recover_sim.c */
    DAMAGE_BITS,    /* data bits on every 7th image, a second bit on every fifth of those: repair_sim.c */
    DAMAGE_BYTES,   /* the same, the second bit alternately in the same byte and in another: bytes_sim.c */
    DAMAGE_LENGTHS, /* a length bit on every 11th image, then data bits on every 7th of the rest: header_sim.c,
                       triage_sim.c, scrub_sim.c, gaps_sim.c */
    DAMAGE_PROFILES
};

struct page_counts {
    uint64_t live;     /* items on the hash table */
    uint64_t ndamaged; /* first pass: live images with a damaged header */
    uint64_t nlen;     /* second pass: images with a length bit flipped */
    uint64_t ndata;    /*              images with data bits flipped ... */
    uint64_t nsame;    /*              ... of those, two bits of one byte */
    uint64_t ntwo;     /*              ... and bits of two bytes */
};

/* Fills `page` (PAGE bytes) through wbufs, copies it to `pristine` unless that is NULL, draws the live set and damages
 * it by `profile`.  Returns 0, or -1 when the item table is too small. */
static inline int page_build(uint8_t *page, uint8_t *pristine, int profile, struct page_counts *c) {
    static uint8_t img[MAX_IMG];
    uint64_t rng = 41, used = 0;
    memset(c, 0, sizeof *c);
    memset(page, 0, PAGE);
    memset(damaged, 0, sizeof damaged);
    memset(rescued, 0, sizeof rescued);
    memset(listed, 0, sizeof listed);
    memset(dead, 0, sizeof dead);

    /* an image never crosses a wbuf, tails stay zero */
    for (nitems = 0;; ++nitems) {
        const uint32_t nt = make_image(img, nitems, &rng);
        if (used % WBUF + nt > WBUF) used = (used / WBUF + 1) * WBUF;
        if (used >= PAGE) break;
        if (nitems >= MAX_ITEMS) {
            fprintf(stderr, "item table too small\n");
            return -1;
        }
        memcpy(page + used, img, nt);
        where[nitems] = at[nitems] = used;
        size_of[nitems] = nt;
        used += nt;
    }
    if (pristine) memcpy(pristine, page, PAGE);

    /* the live set, and the damage "on flash": one header bit of every 37th live image (case 1 draws twice in one
     * expression, as the sims always did: the pinned bytes are those of gcc's order) */
    for (uint32_t id = 0; id < nitems; ++id) {
        if (mix(&rng) % 5 >= 2) {
            where[id] = GONE;
            continue;
        }
        if (c->live++ % 37 == 11) {
            uint8_t *im = page + where[id];
            switch (c->ndamaged % 3) {
                case 0: im[41] = 0; dead[id] = 1; break;                     /* nkey: ends the walk */
                case 1: im[32 + mix(&rng) % 2] ^= (uint8_t)(1u << (mix(&rng) % 8)); break; /* nbytes */
                default: im[38] ^= ITEM_CAS; break;                          /* it_flags */
            }
            damaged[id] = 1;
            ++c->ndamaged;
        }
    }
    if (profile == DAMAGE_HEADERS) return 0;

    /* ... and, of the other live images, by the profile: one of the 42 length bits of every 11th; of the rest every
     * 7th one bit of the stored CRC or the bytes it covers (no length bit), every fifth of those a second one */
    uint64_t rng2 = 77, nth = 0, nmulti = 0;
    for (uint32_t id = 0; id < nitems; ++id) {
        if (where[id] == GONE || damaged[id]) continue;
        uint8_t *im = page + where[id];
        const uint64_t turn = nth++;
        if (profile == DAMAGE_LENGTHS && turn % 11 == 5) {
            flip(im, length_bit_of((uint32_t)(mix(&rng2) % CRC32C_HEADER_BITS)));
            damaged[id] = 3;
            ++c->nlen;
            continue;
        }
        if (turn % 7 != 3) continue;
        const uint64_t nbits = 8ull * size_of[id] - 224;
        uint64_t k1, k2;
        do k1 = 224 + mix(&rng2) % nbits; while (length_bit(k1));
        flip(im, k1);
        damaged[id] = 2;
        if (c->ndata++ % 5 != 4) continue;
        if (profile != DAMAGE_BYTES) {
            do k2 = 224 + mix(&rng2) % nbits; while (length_bit(k2) || k2 == k1);
        } else if (nmulti++ % 2 == 0) {
            do k2 = 8 * (k1 / 8) + mix(&rng2) % 8; while (length_bit(k2) || k2 == k1);
            damaged[id] = 3;
            ++c->nsame;
        } else {
            do k2 = 224 + mix(&rng2) % nbits; while (length_bit(k2) || k2 / 8 == k1 / 8);
            damaged[id] = 4;
            ++c->ntwo;
        }
        flip(im, k2);
    }
    return 0;
}

/* the wbuf's first header no rule fixes (nkey zeroed), or UINT64_MAX */
static inline void first_dead_of(uint64_t first_dead[NWBUF]) {
    for (uint32_t w = 0; w < NWBUF; ++w) first_dead[w] = UINT64_MAX;
    for (uint32_t id = 0; id < nitems; ++id)
        if (dead[id] && at[id] < first_dead[at[id] / WBUF]) first_dead[at[id] / WBUF] = at[id];
}

/* the bits from byte 28 on in which an image of `size` bytes differs from what was written; *which: the last one */
static inline uint32_t flipped_bits(const uint8_t *im, const uint8_t *was, uint32_t size, uint64_t *which) {
    uint32_t nflipped = 0;
    for (uint32_t b = 28; b < size; ++b)
        for (uint32_t i = 0; i < 8; ++i)
            if ((im[b] ^ was[b]) >> i & 1) {
                ++nflipped;
                *which = 8ull * b + i;
            }
    return nflipped;
}

/* ---- the flows every sim replays ---- */

/* storage.c:964-975: the image's key, looked up, must be linked to exactly this offset.  `room`: the bytes that may
 * be read at `off` (the image's, or what is left of its wbuf); *idp, unless NULL: the item. */
static inline int rescue(const uint8_t *page, uint64_t off, uint64_t room, uint32_t *idp) {
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
    if (idp) *idp = (uint32_t)id;
    return 1;
}

static inline uint64_t count_rescued(void) {
    uint64_t got = 0;
    for (uint32_t id = 0; id < nitems; ++id) got += rescued[id];
    return got;
}

/* the reference: the walk of storage.c:950-1072 with the scalar crc32c.  An image whose CRC fails is skipped, a
 * damaged header ends the wbuf. */
static inline void reference_walk(const uint8_t *page) {
    for (uint64_t ps = 0; ps < PAGE; ps += WBUF) {
        uint64_t o = ps;
        while (ps + WBUF - o >= 48 && page[o + 41] != 0) {
            const uint64_t nt = ntotal_of(page + o);
            if (nt > ps + WBUF - o) break;
            if (crc32c(0, page + o + 32, nt - 32) == rd32(page + o + 28)) rescue(page, o, nt, NULL);
            o += nt;
        }
    }
}

/* the page's list, as crc32c_recover_pages, crc32c_triage_pages or crc32c_scrub_pages returns it */
static uint64_t *offs;
static uint32_t *lens;
static uint8_t *kind;
static uint64_t cap, n;
static int failures;
static int triage; /* recover() asks crc32c_triage_pages, whose list holds suspects (kind CRC32C_ITEM_SUSPECT) too */

static inline int list_alloc(uint64_t entries) {
    cap = entries;
    offs = malloc(cap * 8), lens = malloc(cap * 4), kind = malloc(cap);
    return offs && lens && kind ? 0 : -1;
}

static inline void list_free(void) { free(offs); free(lens); free(kind); }

/* fills the list: crc32c_recover_pages or crc32c_triage_pages */
static inline void recover(uint8_t *page) {
    uint64_t nbad = 0, nsalvaged = 0, nsuspect = 0;
    const int rc = triage ? crc32c_triage_pages(page, PAGE, WBUF, offs, lens, kind, cap, &n, &nbad, &nsalvaged,
                                                &nsuspect, NULL, NULL, 0, NULL)
                          : crc32c_recover_pages(page, PAGE, WBUF, offs, lens, kind, cap, &n, &nbad, &nsalvaged, NULL,
                                                 NULL, 0, NULL);
    if (rc != CRC32C_OK || n > cap) {
        fprintf(stderr, "%s: %s\n", triage ? "crc32c_triage_pages" : "crc32c_recover_pages", crc32c_strerror(rc));
        ++failures;
        n = 0;
    }
}

/* The rescue loop over the list, the image's size taken from lens[]: the live items lost.  Nobody vouches for kind 0
 * (reached, but not sane or its CRC fails) or for a suspect.  crc32c_recover_pages lists kinds 0, 1 and
 * CRC32C_ITEM_SALVAGED only, so on its list the tests for suspects, here and below, are idle. */
static inline uint64_t lost_in_list(const uint8_t *page, uint64_t live) {
    memset(rescued, 0, sizeof rescued);
    uint64_t got = 0;
    for (uint64_t k = 0; k < n; ++k)
        if (kind[k] != 0 && kind[k] != CRC32C_ITEM_SUSPECT) got += (uint64_t)rescue(page, offs[k], lens[k], NULL);
    return live - got;
}

/* one read-back and rescue loop */
static inline uint64_t lost_now(uint8_t *page, uint64_t live) {
    recover(page);
    return lost_in_list(page, live);
}

/* which live items the list names at all */
static inline void mark_listed(void) {
    for (uint64_t k = 0; k < n; ++k)
        for (uint32_t id = 0; id < nitems; ++id)
            if (where[id] == offs[k]) listed[id] = 1;
}

/* INTEGRATION.md 4f, the list for crc32c_repair_headers: every kind 0 entry, and every wbuf's walk end that is no
 * entry.  `todo` holds up to cap + NWBUF offsets; returns their number. */
static inline uint64_t header_list(uint64_t *todo) {
    uint64_t m = 0, k = 0;
    for (uint64_t w = 0; w * WBUF < PAGE; ++w) {
        const uint64_t ps = w * WBUF, pe = ps + WBUF < PAGE ? ps + WBUF : PAGE;
        uint64_t end = ps;
        int last = -1;
        for (; k < n && offs[k] < pe; ++k) {
            if (kind[k] == CRC32C_ITEM_SALVAGED || kind[k] == CRC32C_ITEM_SUSPECT) continue;
            if (kind[k] == 0) todo[m++] = offs[k];
            last = kind[k];
            end = offs[k] + lens[k];
        }
        if (last != 0 && end >= ps && end <= pe && pe - end >= 48) todo[m++] = end;
    }
    return m;
}

/* the list for crc32c_repair_items or crc32c_repair_bytes: the entries with kind == 0 && lens != 0 (reached, sane,
 * CRC failing) and, in the same pass over the ascending list, the suspects that pass the caller's filter of
 * one that ends behind the next proven entry (kind 1 or 4) or starts in front of the end of the
 * last suspect kept is dropped.  *nsuspects, *nkept, unless NULL: the suspects met and kept.  Returns the number. */
static inline uint64_t item_list(uint64_t *todo, uint64_t *nsuspects, uint64_t *nkept) {
    uint64_t m = 0, j = 0, kept_end = 0;
    for (uint64_t k = 0; k < n; ++k) {
        if (kind[k] == 0 && lens[k] != 0) todo[m++] = offs[k];
        if (kind[k] != CRC32C_ITEM_SUSPECT) continue;
        if (nsuspects) ++*nsuspects;
        if (j <= k) j = k + 1;
        while (j < n && kind[j] != 1 && kind[j] != CRC32C_ITEM_SALVAGED) ++j;
        const uint64_t next = j < n ? offs[j] : UINT64_MAX, end = offs[k] + lens[k];
        if (end > next || offs[k] < kept_end) continue;
        todo[m++] = offs[k];
        kept_end = end;
        if (nkept) ++*nkept;
    }
    return m;
}

#endif

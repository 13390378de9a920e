/* bytes_sim.c -- storage_compact_readback over a page with damaged headers and
 * damaged data, through crc32c_recover_pages and crc32c_repair_bytes
 * (INTEGRATION.md section 4j): repair_sim.c's page and damage (the same
 * generator and seeds), with its multi-bit hits split into damage inside one
 * byte and damage in two bytes.
 *
 * Three flows over the same bytes:
 *   reference  the walk of storage.c:950-1072 with the scalar crc32c: an image
 *              whose CRC fails is skipped, a damaged header ends the wbuf;
 *   recover    crc32c_recover_pages alone: one rescue loop over its merged list,
 *              kind 0 skipped;
 *   bytes      crc32c_recover_pages, then crc32c_repair_bytes over the entries
 *              with kind == 0 && lens != 0 (reached, sane, CRC failing); the
 *              repaired ones join the rescue loop.
 *
 * The damage "on flash": one header bit of every 37th live image, as in
 * recover_sim.c; of the other live images every 7th has one bit of its stored
 * CRC or of the bytes it covers flipped, every fifth of those a second bit --
 * alternately another bit of the same byte and a bit of another byte.
 *
 * What the rule cannot fix is counted by the sim's own CPU search
 * (crc32c_locate_byte over each damaged live image with the length the sim gave
 * it, from the bytes as they were read): damage that inverts a length bit,
 * damage in two bytes, and -- the flow's own limit -- damaged images that
 * crc32c_recover_pages does not list at all.
 *
 * Usage: bytes_sim [--gpu]
 * Prints live=<l> lost_reference=<a> lost_recover=<b> lost_bytes=<c>
 * repaired=<r> samebyte=<s> unrepairable=<u> length=<x> twobyte=<y>
 * unlisted=<z> (u = x + y + z; s: the repaired images whose damage was two bits
 * of one byte).  Exit status 0 = the run itself worked; the caller judges the
 * counts.
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

static uint32_t rd32(const uint8_t *p) { uint32_t v; memcpy(&v, p, 4); return v; }

static uint64_t ntotal_of(const uint8_t *p) {
    uint16_t flags;
    memcpy(&flags, p + 38, 2);
    return 48ull + p[41] + 1 + rd32(p + 32) + ((flags & 256u) ? 4 : 0) + ((flags & ITEM_CAS) ? 8 : 0);
}

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
/* damaged: 1 header, 2 one bit, 3 two bits of one byte, 4 bits of two bytes */
static uint8_t damaged[MAX_ITEMS], rescued[MAX_ITEMS], listed[MAX_ITEMS];
static uint32_t nitems;

/* storage.c:964-975: the image's key, looked up, must be linked to exactly
 * this offset (`room`: the image's bytes); *idp: the item */
static int rescue(const uint8_t *page, uint64_t off, uint64_t room, uint32_t *idp) {
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

static uint64_t count_rescued(void) {
    uint64_t n = 0;
    for (uint32_t id = 0; id < nitems; ++id) n += rescued[id];
    return n;
}

/* the length-determining header bits (crc32c_batch.h), by image bit index, and for a byte's mask */
static int length_bit(uint64_t k) {
    const uint64_t by = k / 8, b = k % 8;
    return (by >= 32 && by <= 35) || by == 41 || (by == 38 && b == 1) || (by == 39 && b == 0);
}
static int length_mask(uint64_t by, uint8_t m) {
    for (unsigned b = 0; b < 8; ++b)
        if ((m >> b & 1) && length_bit(8 * by + b)) return 1;
    return 0;
}

int main(int argc, char **argv) {
    int gpu = 0;
    for (int i = 1; i < argc; ++i)
        if (!strcmp(argv[i], "--gpu")) gpu = 1;
    crc32c_init();
    if (!gpu) {
        uint8_t buf[64] = {0};
        uint64_t offs[1] = {0}, byte[1] = {9};
        uint8_t ok[1] = {9}, mask[1] = {9};
        crc32c_bytes_out out = {ok, byte, mask, 9, 9};
        const int rc = crc32c_repair_bytes(buf, sizeof buf, 0, offs, 1, NULL, &out);
        printf("bytes_sim: no GPU, repair reports %s\n", crc32c_strerror(rc));
        return rc == CRC32C_ENODEV && ok[0] == 9 && byte[0] == 9 && mask[0] == 9 && out.nrepaired == 9 &&
                       out.nbad == 9
                   ? 0
                   : 1;
    }
    uint8_t *page = calloc(PAGE, 1), *pristine = malloc(PAGE);
    static uint8_t img[MAX_IMG];
    if (!page || !pristine) return 1;
    int failures = 0;
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
        where[nitems] = used;
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
                case 0: im[41] = 0; break;                                   /* nkey: ends the walk */
                case 1: im[32 + mix(&rng) % 2] ^= (uint8_t)(1u << (mix(&rng) % 8)); break; /* nbytes */
                default: im[38] ^= ITEM_CAS; break;                          /* it_flags */
            }
            damaged[id] = 1;
            ++ndamaged;
        }
    }
    /* ... and bits of the stored CRC or the bytes it covers: every 7th of the other live images, one bit (no
     * length bit); every fifth of those a second one, alternately in the same byte and in another */
    uint64_t rng2 = 77, nth = 0, ndata = 0, nmulti = 0, nsame = 0, ntwo = 0;
    for (uint32_t id = 0; id < nitems; ++id) {
        if (where[id] == GONE || damaged[id] || nth++ % 7 != 3) continue;
        uint8_t *im = page + where[id];
        const uint64_t nbits = 8ull * size_of[id] - 224;
        uint64_t k1;
        do k1 = 224 + mix(&rng2) % nbits; while (length_bit(k1));
        im[k1 / 8] ^= (uint8_t)(1u << (k1 % 8));
        damaged[id] = 2;
        if (ndata % 5 == 4) {
            uint64_t k2;
            if (nmulti++ % 2 == 0) {
                do k2 = 8 * (k1 / 8) + mix(&rng2) % 8; while (length_bit(k2) || k2 == k1);
                damaged[id] = 3;
                ++nsame;
            } else {
                do k2 = 224 + mix(&rng2) % nbits; while (length_bit(k2) || k2 / 8 == k1 / 8);
                damaged[id] = 4;
                ++ntwo;
            }
            im[k2 / 8] ^= (uint8_t)(1u << (k2 % 8));
        }
        ++ndata;
    }

    /* flow 1, the reference: storage.c:950-1072 with the scalar crc32c */
    for (uint64_t ps = 0; ps < PAGE; ps += WBUF) {
        uint64_t o = ps;
        while (ps + WBUF - o >= 48 && page[o + 41] != 0) {
            const uint64_t nt = ntotal_of(page + o);
            if (nt > ps + WBUF - o) break;
            if (crc32c(0, page + o + 32, nt - 32) == rd32(page + o + 28)) rescue(page, o, nt, NULL);
            o += nt;
        }
    }
    const uint64_t got_reference = count_rescued();
    memset(rescued, 0, sizeof rescued);

    /* flow 2: crc32c_recover_pages alone */
    const uint64_t cap = 2 * (PAGE / 50) + NWBUF;
    uint64_t *offs = malloc(cap * 8), *bad = malloc(cap * 8), *byte = malloc(cap * 8);
    uint32_t *lens = malloc(cap * 4);
    uint8_t *kind = malloc(cap), *ok = malloc(cap), *mask = malloc(cap);
    uint64_t n = 0, nbad = 0, nsalvaged = 0;
    if (!offs || !bad || !byte || !lens || !kind || !ok || !mask) return 1;
    int rc = crc32c_recover_pages(page, PAGE, WBUF, offs, lens, kind, cap, &n, &nbad, &nsalvaged, NULL, NULL, 0, NULL);
    if (rc != CRC32C_OK || n > cap) {
        fprintf(stderr, "crc32c_recover_pages: %s\n", crc32c_strerror(rc));
        ++failures;
        n = 0;
    }
    for (uint64_t k = 0; k < n; ++k)
        if (kind[k] != 0) rescue(page, offs[k], lens[k], NULL);
    const uint64_t got_recover = count_rescued();
    memset(rescued, 0, sizeof rescued);

    /* flow 3: the same list, the damaged sane entries repaired first */
    uint64_t m = 0, repaired_live = 0, repaired_same = 0;
    for (uint64_t k = 0; k < n; ++k)
        if (kind[k] == 0 && lens[k] != 0) bad[m++] = offs[k];
    crc32c_bytes_out out = {ok, byte, mask, 0, 0};
    rc = crc32c_repair_bytes(page, PAGE, WBUF, bad, m, NULL, &out);
    if (rc != CRC32C_OK) {
        fprintf(stderr, "crc32c_repair_bytes: %s\n", crc32c_strerror(rc));
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
            repaired_same += damaged[id] == 3;
            /* a repaired image is the image that was written */
            if (memcmp(page + offs[k], pristine + offs[k], size_of[id]) != 0) ++failures;
        }
    }
    const uint64_t got_bytes = count_rescued();
    for (uint64_t k = 0; k < n; ++k) { /* which live items the list names at all */
        for (uint32_t id = 0; id < nitems; ++id)
            if (where[id] == offs[k]) listed[id] = 1;
    }
    printf("bytes_sim: %llu entries, %llu given to the repair, %llu repaired, %llu not\n", (unsigned long long)n,
           (unsigned long long)m, (unsigned long long)out.nrepaired, (unsigned long long)out.nbad);

    /* the sim's own count of what the rule cannot fix, from the bytes as they were read (the repairs undone) */
    uint64_t c_length = 0, c_two = 0, c_unlisted = 0;
    for (uint32_t id = 0; id < nitems; ++id) {
        if (where[id] == GONE || !damaged[id]) continue;
        const uint8_t *im = page + where[id];
        const uint32_t nt = size_of[id];
        if (rescued[id]) continue; /* (repaired: counted above against the pristine bytes) */
        uint8_t mk = 0;
        const uint64_t p = crc32c_locate_byte(crc32c(0, im + 32, nt - 32), rd32(im + 28), nt - 32, &mk);
        if (p == CRC32C_NO_BIT) ++c_two;
        else if (length_mask(28 + p, mk)) ++c_length;
        else if (!listed[id]) ++c_unlisted;
        else ++failures; /* one byte, no length bit, listed: the repair should have taken it */
    }
    free(offs); free(bad); free(byte); free(lens); free(kind); free(ok); free(mask);
    printf("bytes_sim: %u items, %llu header-damaged, %llu data-damaged (%llu in one byte twice, %llu in two bytes), "
           "failures %d\n",
           nitems, (unsigned long long)ndamaged, (unsigned long long)ndata, (unsigned long long)nsame,
           (unsigned long long)ntwo, failures);
    printf("live=%llu lost_reference=%llu lost_recover=%llu lost_bytes=%llu repaired=%llu samebyte=%llu "
           "unrepairable=%llu length=%llu twobyte=%llu unlisted=%llu\n",
           (unsigned long long)live, (unsigned long long)(live - got_reference), (unsigned long long)(live - got_recover),
           (unsigned long long)(live - got_bytes), (unsigned long long)repaired_live, (unsigned long long)repaired_same,
           (unsigned long long)(c_length + c_two + c_unlisted), (unsigned long long)c_length,
           (unsigned long long)c_two, (unsigned long long)c_unlisted);
    free(page);
    free(pristine);
    return failures == 0 ? 0 : 1;
}

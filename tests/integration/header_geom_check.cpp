// header_geom_check.cpp -- the arithmetic of crc32c_repair_headers
// (memcached_amd/csrc/header_geom.h) run on the CPU over real images, with the
// CRCs from the library's host CRC (memcached_amd/csrc/crc32c_host.cpp).
//
//   g++ -std=c++17 -Wall -Werror -fsanitize=address,undefined -I memcached_amd/csrc header_geom_check.cpp
//       memcached_amd/csrc/crc32c_host.cpp
//
// For every length bit, a few image lengths and both client-flags widths: the
// bit is inverted in a stamped image; every variant of the damaged header is
// judged by salvage_span over header_room (against mcrc::item_sane over the bytes with the bit
// applied); the CRC of a variant's span with its bit inverted equals the CRC
// of the span as it lies XOR x^t (header_t); and of the candidates exactly one
// hits, the variant of the bit that was inverted.  Prints "header_geom ok".
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <set>
#include <vector>

#include "../../include/crc32c_batch.h"
#include "crc32c_gf2.h"
#include "crc32c_host.h"
#include "header_geom.h"

using namespace mcrc;

static int fails = 0;
#define CHECK(c)                                             \
    do {                                                     \
        if (!(c)) {                                          \
            fprintf(stderr, "%s:%d %s\n", __FILE__, __LINE__, #c); \
            ++fails;                                         \
        }                                                    \
    } while (0)

static uint32_t rnd(uint64_t *s) {
    *s = *s * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(*s >> 32);
}

static uint32_t xpow_t(uint64_t t) {
    uint32_t x = xpow8n(t >> 3);
    for (uint64_t r = t & 7; r; --r) x = repair_step(x);
    return x;
}

static SalvageHdr fields(const uint8_t *it) {
    uint32_t nbytes;
    uint16_t flags;
    memcpy(&nbytes, it + 32, 4);
    memcpy(&flags, it + 38, 2);
    return {nbytes, flags, it[41]};
}

static uint32_t stored(const uint8_t *it) {
    uint32_t e;
    memcpy(&e, it + 28, 4);
    return e;
}

int main() {
    static_assert(kHeaderBits == CRC32C_HEADER_BITS && kHeaderWorkMax == CRC32C_HEADER_WORK_MAX, "the header's constants");
    uint64_t seed = 11;
    // the table v -> k: the length bits of repair_length_bit, each once
    std::set<uint32_t> ks;
    for (uint32_t v = 0; v < kHeaderBits; ++v) {
        CHECK(repair_length_bit(header_bit(v)) && header_bit(v) < 8 * 48);
        ks.insert(header_bit(v));
    }
    CHECK(ks.size() == kHeaderBits);
    for (uint32_t k = 0; k < 8 * 48; ++k) CHECK(repair_length_bit(k) == (ks.count(k) == 1));
    CHECK(kHeaderListMax * kHeaderVariants < 0xffffffffull && (kHeaderListMax + 1) * kHeaderVariants >= 0xffffffffull);
    // the work bound
    CHECK(!header_work_over(0, 0) && header_work_over(1, 0) && !header_work_over(800, 100) && header_work_over(801, 100));
    CHECK(!header_work_over(~0ull, ~0ull / 8 + 1) && header_work_over(~0ull, ~0ull / 8 - 1));

    const uint64_t kBuf = 1 << 14, kOff = 37;
    uint64_t tried = 0, cands = 0;
    for (uint32_t cfl : {4u, 8u})
        for (uint32_t nt : {52u, 61u, 77u, 300u, 4165u})
            for (uint32_t region : {0u, 8192u}) {
                std::vector<uint8_t> buf(kBuf);
                for (auto &b : buf) b = (uint8_t)rnd(&seed);
                // a stamped image of nt bytes at kOff: CAS and client flags where they fit
                uint8_t *it = buf.data() + kOff;
                const bool cas = nt >= 77, cflags = nt >= 300;
                const uint32_t nkey = nt < 60 ? 1 : 1 + nt % 5;  // (52 bytes: a one-byte key and the bare CRLF)
                const uint32_t nbytes = nt - 49 - nkey - (cas ? 8 : 0) - (cflags ? cfl : 0);
                const uint16_t flags = (uint16_t)((cas ? 2 : 0) | (cflags ? 256 : 0) | 0x40);
                memcpy(it + 32, &nbytes, 4);
                memcpy(it + 38, &flags, 2);
                it[41] = (uint8_t)nkey;
                it[nt - 2] = '\r';
                it[nt - 1] = '\n';
                const uint32_t e = crc32c_host_sw(0, it + 32, nt - 32);
                memcpy(it + 28, &e, 4);
                CHECK(salvage_span(fields(it), cfl, header_room(kOff, kBuf, region)) == nt);
                for (uint32_t v = 0; v < kHeaderBits; ++v) {
                    const uint32_t kv = header_bit(v);
                    it[kv / 8] ^= (uint8_t)(1u << (kv % 8));  // the damage
                    const SalvageHdr h = fields(it);
                    uint32_t nhits = 0, which = ~0u, len_hit = 0;
                    for (uint32_t w = 0; w < kHeaderBits; ++w) {
                        const uint32_t kw = header_bit(w);
                        const SalvageHdr f = header_variant(h, w);
                        const uint32_t ntw = salvage_span(f, cfl, header_room(kOff, kBuf, region));
                        // the fields and the verdict are those of the bytes with the bit applied
                        it[kw / 8] ^= (uint8_t)(1u << (kw % 8));
                        const SalvageHdr g = fields(it);
                        uint64_t want = 0;
                        const bool sane = item_sane(buf.data(), kBuf, region, kOff, cfl, &want);
                        CHECK(g.nbytes == f.nbytes && g.flags == f.flags && g.nkey == f.nkey);
                        CHECK(sane == (ntw != 0) && want == ntw);
                        const uint32_t flipped = ntw ? crc32c_host_sw(0, it + 32, ntw - 32) : 0;
                        it[kw / 8] ^= (uint8_t)(1u << (kw % 8));
                        ++tried;
                        if (!ntw) continue;
                        // inverting bit kw of the span changes its CRC by x^t
                        const uint32_t asis = crc32c_host_sw(0, it + 32, ntw - 32);
                        CHECK((asis ^ xpow_t(header_t(w, ntw - 32))) == flipped);
                        CHECK(header_t(w, ntw - 32) == repair_t_of_q(kw - 224, ntw - 32));
                        if (!(salvage_has_crlf(f.nbytes) && salvage_crlf(it[ntw - 2], it[ntw - 1]))) continue;
                        ++cands;
                        if ((asis ^ xpow_t(header_t(w, ntw - 32))) == stored(it)) {
                            ++nhits;
                            which = w;
                            len_hit = ntw;
                        }
                    }
                    CHECK(nhits == 1 && which == v && len_hit == nt);
                    // the header as it stands (variant 42) changes nothing
                    const SalvageHdr same = header_variant(h, kHeaderAsIs);
                    CHECK(same.nbytes == h.nbytes && same.flags == h.flags && same.nkey == h.nkey);
                    it[kv / 8] ^= (uint8_t)(1u << (kv % 8));
                }
            }
    CHECK(tried == 2 * 5 * 2 * 42 * 42 && cands >= 2 * 5 * 2 * 42);
    if (fails) return 1;
    printf("header_geom ok\n");
    return 0;
}

// copy_edges_check.cpp -- the store decomposition of k_copy (memcached_amd/csrc/
// copy_edges.h) run on the CPU for every alignment pair.
//
// For every source address mod 16 x destination address mod 16 x ITEM_ntotal
// in 50..300, 4096 +- 80 and 8192 +- 80, the stores that for_each_copy_store
// lists (copy_plan and edge_widths, which the kernel's stores follow) must
//   - cover the image bytes [0, nt) exactly once and touch nothing else;
//   - take every byte from the aligned 16-B source piece that holds it: store
//     (at, width, piece, byte) has byte + width <= 16, piece < npieces and
//     16 piece - sa + byte == at;
//   - be 16 B wide for every piece inside the image, and 1, 2, 4 or 8 B wide
//     in descending order, each at a multiple of its width from the first, for
//     the first and the last piece only.
// The stores are also performed, from a source whose pieces are read as
// aligned 16-B blocks into a destination pre-filled with 0xa5 at the
// destination's alignment, and the result compared with memcpy.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "copy_edges.h"

namespace {

int g_fail = 0;
#define CHECK(c)                                                                              \
    do {                                                                                      \
        if (!(c)) {                                                                           \
            if (g_fail++ < 20) fprintf(stderr, "%s:%d: %s (sa %u da %u nt %llu)\n", __FILE__, __LINE__, #c, sa, da, \
                                       (unsigned long long)nt);                               \
        }                                                                                     \
    } while (0)

void check_one(uint32_t sa, uint32_t da, uint64_t nt) {
    const mcrc::CopyPlan p = mcrc::copy_plan(sa, da, nt);
    CHECK(p.npieces == (sa + nt + 15) / 16 && p.npieces >= 4);
    CHECK(p.head == 16 - sa && p.tail >= 1 && p.tail <= 16);
    CHECK(16ull * (p.npieces - 1) - sa + p.tail == nt);
    CHECK(p.dalign == ((da + 16 - sa) & 15u));

    // the source: 16-B aligned pieces, the image sa bytes into piece 0; the
    // bytes of the first and last piece outside the image are poison
    alignas(16) static uint8_t srcbuf[16 * 600];
    static uint8_t dstbuf[64 + 16 * 600 + 64];
    const uint64_t span = 16ull * p.npieces;
    for (uint64_t i = 0; i < span; ++i) srcbuf[i] = (uint8_t)(i * 131 + 7 * sa + 3);
    for (uint64_t i = 0; i < sa; ++i) srcbuf[i] = 0xee;
    for (uint64_t i = sa + nt; i < span; ++i) srcbuf[i] = 0xee;
    memset(dstbuf, 0xa5, sizeof dstbuf);
    uint8_t *const dimg = dstbuf + 48 + da;  // ((dstbuf + 48) need not be aligned: only the offset matters here)

    std::vector<uint8_t> hits(nt, 0);
    uint32_t last_piece = 0, last_width = 0, first_at_of_piece = 0, nstores = 0;
    bool seen = false;
    mcrc::for_each_copy_store(sa, da, nt, [&](uint64_t at, uint32_t width, uint32_t piece, uint32_t byte) {
        ++nstores;
        CHECK(width == 1 || width == 2 || width == 4 || width == 8 || width == 16);
        CHECK(piece < p.npieces && byte + width <= 16);
        CHECK((int64_t)16 * piece - sa + byte == (int64_t)at);
        CHECK(at + width <= nt);
        const bool edge = piece == 0 || piece + 1 == p.npieces;
        if (!edge) CHECK(width == 16 && byte == 0);
        if (seen && piece == last_piece) {
            CHECK(edge && width < last_width);  // descending widths within an edge piece
            CHECK((at - first_at_of_piece) % width == 0);
        } else {
            CHECK(!seen || piece == last_piece + 1);  // pieces in order, none skipped
            first_at_of_piece = (uint32_t)at;
        }
        seen = true;
        last_piece = piece;
        last_width = width;
        if (at + width <= nt) {
            for (uint32_t k = 0; k < width; ++k) ++hits[at + k];
            memcpy(dimg + at, srcbuf + 16ull * piece + byte, width);
        }
    });
    CHECK(seen && last_piece + 1 == p.npieces);
    CHECK(nstores <= p.npieces + 6);  // at most four stores per edge piece
    bool once = true;
    for (uint64_t i = 0; i < nt; ++i) once = once && hits[i] == 1;
    CHECK(once);
    CHECK(memcmp(dimg, srcbuf + sa, nt) == 0);
    bool clean = true;
    for (const uint8_t *q = dstbuf; q < dimg; ++q) clean = clean && *q == 0xa5;
    for (const uint8_t *q = dimg + nt; q < dstbuf + sizeof dstbuf; ++q) clean = clean && *q == 0xa5;
    CHECK(clean);
}

}  // namespace

int main() {
    uint64_t cases = 0;
    for (uint32_t sa = 0; sa < 16; ++sa)
        for (uint32_t da = 0; da < 16; ++da) {
            for (uint64_t nt = 50; nt <= 300; ++nt, ++cases) check_one(sa, da, nt);
            for (uint64_t c : {4096ull, 8192ull})
                for (uint64_t nt = c - 80; nt <= c + 80; ++nt, ++cases) check_one(sa, da, nt);
        }
    // edge_widths alone: every byte count of a piece
    for (uint32_t n = 1; n <= 16; ++n) {
        uint32_t w[4], sum = 0;
        const uint32_t k = mcrc::edge_widths(n, w);
        for (uint32_t j = 0; j < k; ++j) sum += w[j];
        if (sum != n || k < 1 || k > 4) {
            fprintf(stderr, "edge_widths(%u)\n", n);
            ++g_fail;
        }
    }
    if (g_fail) {
        fprintf(stderr, "copy_edges: %d checks failed\n", g_fail);
        return 1;
    }
    printf("copy_edges ok (%llu cases)\n", (unsigned long long)cases);
    return 0;
}

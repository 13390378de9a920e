// copy_edges.h -- which stores copy an item image (k_copy, k_copy.h).
//
// k_copy reads an image as the aligned 16-B pieces that hold a byte of it and
// stores each piece's bytes at the destination's own byte alignment.  With sa
// = the source address mod 16, piece k holds image bytes [16 k - sa,
// 16 k - sa + 16): every piece but the first and the last lies inside the
// image and is one 16-B store; piece 0 (sa != 0) and the last piece (when the
// image does not end on a piece boundary) straddle an image edge and are
// stored narrower, by one lane, as the 8-, 4-, 2- and 1-B stores of their byte
// count's set bits.  Plain C++ too, so that a CPU program can run the
// decomposition for every alignment pair (tests/integration/
// copy_edges_check.cpp).
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define COPY_EDGES_HD __host__ __device__
#else
#define COPY_EDGES_HD
#endif

namespace mcrc {

struct CopyPlan {
    uint32_t npieces;  // aligned 16-B source pieces holding a byte of the image
    uint32_t head;     // bytes of piece 0 inside the image (its last ones): 16 - sa; 16: a whole store
    uint32_t tail;     // bytes of the last piece inside the image (its first ones); 16: a whole store
    uint32_t dalign;   // destination address mod 16 of the whole-piece stores: (da - sa) mod 16.  (The
                       // stores are issued at that alignment as they are; only a form that realigns in
                       // registers would take a width from it.)
};

// sa / da: the image's source / destination address mod 16; nt = ITEM_ntotal
// (an image is at least 50 bytes: four pieces or more, so the head, the
// header's second piece and the tail are three different pieces).
COPY_EDGES_HD inline CopyPlan copy_plan(uint32_t sa, uint32_t da, uint64_t nt) {
    const uint32_t over = (uint32_t)((sa + nt) & 15u);  // bytes of the image in a partial last piece
    return {(uint32_t)((sa + nt + 15u) >> 4), 16u - sa, over ? over : 16u, (da - sa) & 15u};
}

// Widths of the stores that write n bytes of one piece, in the order issued:
// 16 is one store, anything less the set bits of n from 8 down.  Each store
// starts at a multiple of its own width from the first byte written.
COPY_EDGES_HD inline uint32_t edge_widths(uint32_t n, uint32_t w[4]) {
    if (n >= 16u) {
        w[0] = 16u;
        return 1u;
    }
    uint32_t k = 0;
    for (uint32_t b = 8u; b; b >>= 1)
        if (n & b) w[k++] = b;
    return k;
}

// Every store of the copy, in image order: f(at, width, piece, byte) writes
// image bytes [at, at + width) from bytes [byte, byte + width) of source piece
// `piece`.
template <class F>
COPY_EDGES_HD inline void for_each_copy_store(uint32_t sa, uint32_t da, uint64_t nt, F f) {
    const CopyPlan p = copy_plan(sa, da, nt);
    uint32_t w[4];
    for (uint32_t k = 0; k < p.npieces; ++k) {
        const bool first = k == 0, last = k + 1 == p.npieces;
        const uint32_t n = first ? p.head : last ? p.tail : 16u;
        uint32_t byte = first ? sa : 0u;
        uint64_t at = first ? 0u : 16ull * k - sa;
        const uint32_t nw = edge_widths(n, w);
        for (uint32_t j = 0; j < nw; ++j) {
            f(at, w[j], k, byte);
            at += w[j];
            byte += w[j];
        }
    }
}

}  // namespace mcrc

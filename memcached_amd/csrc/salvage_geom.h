// salvage_geom.h -- the arithmetic of crc32c_salvage_pages that needs no GPU:
// the pieces, the cuts that turn a gap between covered images into a range of
// eligible offsets, the tiles a range is scanned in, what makes a header a
// candidate given its bytes, and the work bound.  Plain C++ over k_consts.h
// (k_salvage.h and shim_salvage.h use it; tests/integration/
// salvage_geom_check.cpp runs it on the CPU).
//
// The rule (include/crc32c_batch.h): piece w of a buffer is [w W, min((w + 1) W,
// base_bytes)); an offset o of a piece ending at pe is eligible when pe - o >=
// 48 and no covered image holds it; eligible offsets are looked at one by one.
#pragma once

#include <stdint.h>

#include "k_consts.h"

namespace mcrc {

constexpr uint32_t kSalvageTile = 4096;   // bytes of an aligned block the scan takes per step (256 pieces of 16 B)
constexpr uint32_t kSalvageWorkMax = 64;  // CRC32C_SALVAGE_WORK_MAX

MCRC_HD uint64_t salvage_piece_end(uint64_t w, uint64_t wbuf, uint64_t base_bytes) {
    const uint64_t ps = w * wbuf;
    return base_bytes - ps < wbuf ? base_bytes : ps + wbuf;
}

// The eligible offsets [lo, hi) of the gap [a, b) between covered images in
// the piece [ps, pe): those with 48 bytes left in the piece (lo == hi: none).
struct SalvageRange {
    uint64_t lo, hi;
};
MCRC_HD SalvageRange salvage_cut(uint64_t a, uint64_t b, uint64_t ps, uint64_t pe) {
    const uint64_t last = pe - ps >= 48 ? pe - 47 : ps;  // one past the last offset with 48 bytes left
    const uint64_t hi = b < last ? b : last;
    return {a, a < hi ? hi : a};
}

// Tiles.  A range is scanned in the aligned kSalvageTile blocks of the
// buffer's address space that hold one of its offsets: with ba = the base
// address mod kSalvageTile, offset o lies in block (ba + o) / kSalvageTile.
// Tile k of the range is its part inside its k-th block, so a tile never
// straddles a block and every 16-B piece of it is aligned.
MCRC_HD uint64_t salvage_ntiles(uint64_t lo, uint64_t hi, uint32_t ba) {
    return lo < hi ? (ba + hi - 1) / kSalvageTile - (ba + lo) / kSalvageTile + 1 : 0;
}
MCRC_HD SalvageRange salvage_tile(uint64_t lo, uint64_t hi, uint32_t ba, uint64_t k) {
    const uint64_t g = ((ba + lo) / kSalvageTile + k) * kSalvageTile;  // the block's first byte, from base - ba
    const uint64_t s = g > ba + lo ? g - ba : lo, e = g + kSalvageTile - ba;
    return {s, e < hi ? e : hi};
}

// Header fields of a possible image at o: nbytes (bytes 32..35), it_flags
// (38..39), nkey (41).
struct SalvageHdr {
    uint32_t nbytes, flags, nkey;
};
// ITEM_ntotal of a header that is sane with `room` = pe - o bytes left in its
// piece (pe <= base_bytes, so "inside the buffer and inside its own piece" is
// ntotal <= room; mcrc::item_sane for an offset with 48 bytes left), else 0.
MCRC_HD uint32_t salvage_span(const SalvageHdr &h, uint32_t cfl, uint64_t room) {
    if (h.nkey == 0 || h.nbytes >= 0x80000000u) return 0;
    // (at most 2^31 + 320: 32 bits hold it)
    const uint32_t nt = 49u + h.nkey + h.nbytes + ((h.flags & 256u) ? cfl : 0u) + ((h.flags & 2u) ? 8u : 0u);
    return nt - 32u > mcrc_dev::kMaxSpan || nt > room ? 0u : nt;
}
// A sane header is a candidate when its value ends in CRLF: c0, c1 = the
// image's last two bytes (read only when nbytes >= 2).
MCRC_HD bool salvage_has_crlf(uint32_t nbytes) { return nbytes >= 2; }
MCRC_HD bool salvage_crlf(uint8_t c0, uint8_t c1) { return c0 == 0x0d && c1 == 0x0a; }

// The work bound: the candidates' spans add up to more than
// kSalvageWorkMax * (scanned + wbuf).  (No product is formed: nothing overflows.)
MCRC_HD bool salvage_work_over(uint64_t work, uint64_t scanned, uint64_t wbuf) {
    const uint64_t x = scanned + wbuf < scanned ? ~0ull : scanned + wbuf;
    const uint64_t q = work / kSalvageWorkMax;
    return q > x || (q == x && work % kSalvageWorkMax != 0);
}

}  // namespace mcrc

// header_geom.h -- the arithmetic of crc32c_repair_headers that needs no GPU:
// the 42 header bits that decide ITEM_ntotal, the fields of a header with one
// of them inverted, ITEM_ntotal and sanity from the fields, the exponent a
// variant's bit has in its own span's CRC, and the work bound.  Plain C++ over
// k_consts.h (k_header.h and shim_header.h use it;
// tests/integration/header_geom_check.cpp runs it on the CPU).
//
// The rule (include/crc32c_batch.h).  Variant v < 42 of the header at o is the
// header with image bit k = header_bit(v) inverted; variant 42 is the header as
// it stands.  Bit k lies in the span's first ten bytes, so with L' the
// variant's span length, inverting it changes the span's CRC by x^t, t =
// repair_t_of_q(k - 224, L') (repair_geom.h): a variant hits when the CRC of
// the bytes as they lie, XOR x^t, equals the stored one.
#pragma once

#include <stdint.h>

#include "k_consts.h"
#include "repair_geom.h"
#include "salvage_geom.h"

namespace mcrc {

constexpr uint32_t kHeaderBits = 42;     // CRC32C_HEADER_BITS
constexpr uint32_t kHeaderWorkMax = 8;   // CRC32C_HEADER_WORK_MAX
constexpr uint32_t kHeaderAsIs = kHeaderBits;          // the variant that inverts nothing
constexpr uint32_t kHeaderVariants = kHeaderBits + 1;  // lanes of a header's wave that have one
constexpr uint64_t kHeaderListMax = (0xffffffffull - 1) / kHeaderVariants;  // 43 n < 2^32 - 1

// Variant v -> image bit k: nbytes (bytes 32..35), nkey (byte 41), it_flags bit
// 1 (ITEM_CAS: byte 38 bit 1), it_flags bit 8 (ITEM_CFLAGS: byte 39 bit 0).
MCRC_HD uint32_t header_bit(uint32_t v) {
    return v < 32 ? 256u + v : v < 40 ? 328u + (v - 32u) : v == 40 ? 305u : 312u;
}

// The fields (nbytes, it_flags, nkey) with variant v's bit inverted.
MCRC_HD SalvageHdr header_variant(SalvageHdr h, uint32_t v) {
    if (v < 32) h.nbytes ^= 1u << v;
    else if (v < 40) h.nkey ^= 1u << (v - 32u);
    else if (v == 40) h.flags ^= 2u;
    else if (v == 41) h.flags ^= 256u;
    return h;
}

// The bytes an image at off (inside the buffer) may take: up to the end of the
// buffer and of its own region (0: no such bound).  The same for every variant
// of one header, and what salvage_span (salvage_geom.h) judges a variant's
// fields by: ITEM_ntotal when crc32c_verify_items would call them sane, else 0.
MCRC_HD uint64_t header_room(uint64_t off, uint64_t base_bytes, uint64_t region) {
    const uint64_t left = base_bytes - off;
    if (region == 0) return left;
    const uint64_t in_region = region - off % region;
    return in_region < left ? in_region : left;
}

// A variant v < 42 whose header is sane is a candidate when its value ends in
// CRLF (salvage_has_crlf, salvage_crlf); the header as it stands needs none.

// The exponent of variant v's bit in the CRC of its own span of len bytes.
MCRC_HD uint64_t header_t(uint32_t v, uint64_t len) { return repair_t_of_q(header_bit(v) - 224u, len); }

// The work bound: the candidate variants' spans add up to more than
// kHeaderWorkMax * base_bytes.  (No product is formed: nothing overflows.)
MCRC_HD bool header_work_over(uint64_t work, uint64_t base_bytes) {
    const uint64_t q = work / kHeaderWorkMax;
    return q > base_bytes || (q == base_bytes && work % kHeaderWorkMax != 0);
}

}  // namespace mcrc

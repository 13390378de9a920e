// crc32c_host.h -- the shim's own host CRC-32C for the synchronous scalar call
// surface (crc_func crc32c, crc32c.h:15-16).  Single calls from storage.c are
// latency-bound (one 4 KiB item ~0.5 us on a core) and stay on the host; batched
// callers use the GPU entry points in crc32c_batch.h.
//
//   crc32c_host_sw : slice-by-8 tables (same results as crc32c_sw, crc32c.c:366-424)
//   crc32c_host_hw : the CRC32C instruction (SSE4.2 crc32 / ARMv8 crc32cx), three independent streams merged
//                    with zeros operators (same results as crc32c_hw, crc32c.c:161-246)
#pragma once

#include <stddef.h>
#include <stdint.h>

namespace mcrc {

void host_tables_init();  // idempotent, thread-safe
uint32_t crc32c_host_sw(uint32_t crc, const void *buf, size_t len);
uint32_t crc32c_host_hw(uint32_t crc, const void *buf, size_t len);
// crc32c_sw_big (crc32c.c:467-498) as the reference computes it on this host
uint32_t crc32c_host_sw_big(uint32_t crc, const void *buf, size_t len);
bool host_has_hw_crc();  // SSE4.2 (x86-64) or the ARMv8 CRC extension (arm64)
// crc32c(crc, A || B) from crc32c(crc, A), crc32c(0, B) and |B|.
uint32_t crc32c_host_combine(uint32_t crc_a, uint32_t crc_b, uint64_t len_b);

// The item header rule of the device code (mcrc_dev::ItemHdr / item_desc,
// k_common.h) restated for the host: ITEM_ntotal of the image at `it`
// (memcached.h:149-152; cfl = sizeof(client_flags_t)), and whether the image at
// base + off is sane -- its 48 header bytes lie in [base, base + base_bytes),
// nkey != 0, nbytes < 2^31, its span is at most CRC32C_MAX_SPAN, and it ends
// inside the buffer and inside its own `region` (0: no such bound).  *ntotal:
// ITEM_ntotal of a sane image, else 0.
uint64_t item_ntotal(const uint8_t *it, uint32_t cfl);
bool item_sane(const uint8_t *base, uint64_t base_bytes, uint64_t region, uint64_t off, uint32_t cfl,
               uint64_t *ntotal);

}  // namespace mcrc

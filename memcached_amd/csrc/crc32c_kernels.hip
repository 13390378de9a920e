// crc32c_kernels.hip -- hand-written gfx950 kernels for batched CRC-32C.
//
// K1  k_fixed<CRCIN, NT>: equal 4 KiB, 16-B aligned items at a fixed stride
//     (extstore spill batches of one slab class; BASELINE configs 2 and 4).
//     Replaces N calls of crc32c(0, item, len), crc32c_hw (crc32c.c:161-246)
//     reached from storage.c:567.
// K2  k_spans<UNITS>: any offsets, lengths and alignment; one 32-lane group
//     per work unit of <= 128 KiB (configs 3 and 5, storage.c:172 read-back
//     spans), then k_final<MODE 0> per span.
// K3  the same kernels over the spans of packed item images in extstore
//     pages, [off+32, off+ITEM_ntotal) (k_count<MODE 1/2> parses the
//     headers): k_final<MODE 1> checks the CRC stored in the item's exptime
//     field (storage.c:160-178 over the page walk of storage.c:950-960);
//     k_final<MODE 2> stamps it (the spill CRC of storage.c:567, batched per
//     wbuf); k_final<MODE 3> (CRC32C_KEEP_STAMPED) stamps the images whose
//     exptime is 0 and checks the others.  k_walk walks the pages on the
//     device.
// K4  k_blocks: spans whose unit is one 4 KiB block (K1's loop, gathered).
// K5  k_lines<MODE>: spans or item images whose span is one 4 KiB window of
//     whole lines after a short head (every 4165-B image of config 5 and the
//     config-2 variant), each image's header, head and tail done once by one
//     lane of a run of consecutive images; k_fix stamps (MODE 2).
//     k_small: batches of up to 8192 spans in one launch (IO batches, wbufs,
//     the coalescing queue).
//     k_copy: k_small's verify with every block also stored at the image's
//     destination (crc32c_copy_items: compaction's rescue copy, checked).
//
// See crc32c_device.h for the lane-group work model and LDS table layouts.
//
// One header per family, included here in the kernels' definition order
// (each includes what it uses, so any one of them compiles alone).
#include "k_common.h"  // loads, geometry, SpanArgs, Tab8, span_corr, parse_hdr, emit, count_bad
#include "k_fixed.h"   // K1
#include "k_spans.h"   // K2/K3: work units, k_spans
#include "k_plan.h"    // K2/K3: k_count, the plan's scans, k_expand, k_final
#include "k_small.h"   // k_small
#include "k_copy.h"    // k_copy: crc32c_copy_items (copy and verify in one pass)
#include "k_window.h"  // K1Regs / k1_lane_value: the whole window of K4 and K5
#include "k_blocks.h"  // K4
#include "k_lines.h"   // K5: k_lines, k_fix, k_census
#include "k_walk.h"    // k_gather_offs, k_scatter_ok, k_chain, k_walk
#include "k_salvage.h" // crc32c_salvage_pages: k_salvage_regions, k_salvage_scan, k_salvage_pick (the triage's too)
#include "k_recover.h" // crc32c_recover_pages, crc32c_triage_pages: k_recover_regions, k_recover_merge
#include "k_repair.h"  // crc32c_repair_items: k_repair_count, k_repair_emit, k_repair_search, k_repair_apply
#include "k_header.h"  // crc32c_repair_headers: k_header_variants, k_header_apply
#include "k_scrub.h"   // crc32c_scrub_pages: k_scrub_headers, k_scrub_items, k_scrub_gaps, k_scrub_gap_merge, k_scrub_log, k_scrub_log_bytes
#include "k_repair_bytes.h"  // crc32c_repair_bytes: k_repair_bytes_search, k_repair_bytes_apply
#include "k_ptrs.h"    // crc32c_batch_ptrs on device arrays: k_ptr_rebase

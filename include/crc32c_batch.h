/* crc32c_batch.h -- batched CRC-32C on AMD Instinct MI355X (gfx950).
 *
 * New surface added next to crc32c.h.  Each entry point
 * replaces a loop of scalar crc32c() calls in the reference:
 *
 *   crc32c_batch           N x crc32c(crc_in[i], base + off[i], len[i]):
 *                          the spill CRC of storage.c:567 gathered per wbuf,
 *                          the read-back CRC of storage.c:172 and
 *                          proxy_internal.c:28 gathered per IO batch
 *                          (extstore.c:853-945).
 *   crc32c_stamp_items     the spill CRC of storage.c:567 for every item image of
 *                          a wbuf, written into exptime.
 *   crc32c_batch_chains    the chained CRC of chunked items over iov lists
 *                          (storage.c:163-170).
 *   crc32c_verify_pages    the same over whole pages, walked on the device as
 *                          storage_compact_readback walks them.
 *   crc32c_stamp_pages     crc32c_stamp_items over a wbuf walked on the device
 *                          the same way: no offset list; with
 *                          CRC32C_KEEP_STAMPED the images compaction copied with
 *                          their CRC (storage.c:1004-1006) are verified, not
 *                          stamped again.
 *   crc32c_salvage_pages   the images of a page that the walk never reaches because
 *                          a damaged header in front of them ended it
 *                          (storage.c:950-1072 loses them silently): every
 *                          unreached offset tried as an image start, the ones
 *                          whose stored CRC proves them reported.
 *   crc32c_recover_pages   crc32c_verify_pages and crc32c_salvage_pages in one call:
 *                          the page staged once, the walk's lists kept on the
 *                          device, one merged list with each image's kind and
 *                          ITEM_ntotal for a single rescue loop.
 *   crc32c_triage_pages    crc32c_recover_pages with a third list merged in: the
 *                          unreached candidates whose stored CRC does not match
 *                          (kind CRC32C_ITEM_SUSPECT), the data-damaged images
 *                          behind a header that ended its wbuf's walk, so that
 *                          crc32c_repair_items can be handed them.
 *   crc32c_repair_items   the images those calls prove damaged (kind 0,
 *                          CRC32C_ITEM_DAMAGED, badcrc_from_extstore) and the
 *                          reference drops: where one inverted bit explains the
 *                          mismatch, the stored CRC names it; it is flipped back
 *                          and the image proven again.  crc32c_locate_bit is the
 *                          same search for one span on the host (no GPU).
 *   crc32c_repair_bytes    the images whose damage is several bits of one byte:
 *                          the same search names the byte and its XOR mask, at 32
 *                          times the one-bit rule's false-repair odds
 *                          (crc32c_locate_byte: one span on the host).
 *   crc32c_repair_headers  the one image per damaged header that those calls still
 *                          lose: a flipped bit of nbytes, nkey or the two it_flags
 *                          bits that decide ITEM_ntotal moves the image's end, and
 *                          derails its wbuf's walk.  The 42 headers one such bit
 *                          away are tried, each over its own span; the one whose
 *                          CRC matches is the header that was written.
 *   crc32c_verify_items    the read-verify compare of storage.c:159-178 applied
 *                          to every item image of a packed extstore page
 *                          (walk of storage.c:950-960): CRC over
 *                          [off + 32, off + ITEM_ntotal) against the value
 *                          stored in the item's exptime field (byte 28).
 *   crc32c_copy_items      the rescue copy of storage_compact_readback
 *                          (storage.c:1004-1006), which the reference makes
 *                          unchecked: every image compaction keeps is moved to
 *                          its new place and verified from the same loads.
 *   crc32c_host_alloc      pinned buffers for wbufs / readback_buf (SURVEY.md 8f
 *                          rank 3).
 *   crc32c_batch_multi     crc32c_batch for host-resident batches split across
 *                          several GPUs by bytes (no collective: items are
 *                          independent); crc32c_shard_cuts is its split.
 *   crc32c_batch_submit    the read-verify CRCs of many IO threads
 *   / crc32c_batch_wait    (extstore.c:853-945, one batch of <= io_depth reads
 *                          per thread) coalesced into one kernel launch per
 *                          dispatch by a per-device queue.
 *
 * Results are bit-identical to the reference crc32c.c.  There is no CPU
 * fallback: without a usable gfx950 device every batch entry point returns
 * CRC32C_ENODEV.  Buffers stay owned by the caller and must stay valid until
 * the call (or crc32c_batch_wait) returns.
 */
#ifndef CRC32C_BATCH_H
#define CRC32C_BATCH_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CRC32C_OK 0
#define CRC32C_ENODEV (-1) /* no gfx950 device visible */
#define CRC32C_EHIP (-2)   /* HIP runtime error */
#define CRC32C_EINVAL (-3) /* bad arguments */
#define CRC32C_ENOMEM (-4) /* device or pinned allocation failed */
#define CRC32C_ERANGE (-5) /* a span lies outside [base, base + base_bytes): it was
                              not read and its out[] entry is 0 */
#define CRC32C_EWALK (-6)  /* crc32c_verify_pages / _stamp_pages: the device walk's count and emit
                              passes disagreed on some wbuf (an internal invariant;
                              the results are not valid) */
#define CRC32C_EWORK (-7)  /* crc32c_salvage_pages / _recover_pages / _triage_pages: the candidates' spans exceed
                              the work bound; crc32c_repair_items: the damaged images' spans do;
                              crc32c_repair_headers: the candidate variants' spans do */

/* flags */
#define CRC32C_DEVICE 0x1u    /* every pointer in the batch is device memory of the
                                 current HIP device */
#define CRC32C_ASYNC 0x2u     /* with CRC32C_DEVICE: enqueue on `stream`, do not wait */
/* (0x4u is reserved: earlier builds named it CRC32C_ALIGNED16, an alignment
   promise no kernel needs -- every span kernel reads the 16-B pieces a span
   overlaps as they lie, at any alignment -- and it is ignored.) */
#define CRC32C_CFLAGS64 0x8u  /* item-image calls: the images come from a build with
                                 --enable-large-client-flags (configure.ac:139-140):
                                 client_flags_t is 8 bytes, so ITEM_CFLAGS adds 8 to
                                 ITEM_ntotal instead of 4 (memcached.h:96-100, :149-152) */
#define CRC32C_KEEP_STAMPED 0x10u /* stamp calls: an image whose exptime is not 0 already
                                 carries its CRC (compaction copies images with it,
                                 storage.c:1004-1006): it is verified against that
                                 value and not written; see crc32c_stamp_items */
#define CRC32C_LOCATE_ONLY 0x20u /* repair calls: report, write nothing into the buffer */

/* ok[] values of the stamp calls (0: malformed, or a carried image whose stored
 * CRC does not match) */
#define CRC32C_ITEM_STAMPED 1 /* the CRC was written into exptime */
#define CRC32C_ITEM_KEPT 2    /* CRC32C_KEEP_STAMPED: the stored CRC matched, nothing written */

/* ok[] values of crc32c_copy_items (0: nothing written -- a malformed source
 * image, or one that does not fit dst) */
#define CRC32C_ITEM_COPIED 1  /* written to dst, stored CRC matches */
#define CRC32C_ITEM_DAMAGED 3 /* written to dst verbatim, stored CRC does not match */

/* Longest span: 2 GiB - 64 KiB, twice the largest item memcached stores
 * (ITEM_SIZE_MAX_UPPER_LIMIT, memcached.h:115).  A device span past it is not
 * read (out[i] = 0, CRC32C_ERANGE; an item image claiming one is malformed);
 * a fixed-length batch or a host batch with one is rejected (CRC32C_EINVAL;
 * host spans are limited to 256 MiB each). */
#define CRC32C_MAX_SPAN 0x7fff0000u

/* A batch of byte spans inside one buffer.
 *   span i = [base + (offsets ? offsets[i] : i * stride),  + (lens ? lens[i] : len))
 *   out[i] = crc32c(crc_in ? crc_in[i] : 0, span i)
 * base_bytes bounds every span: no byte outside [base, base + base_bytes) is
 * read.  In a device batch (CRC32C_DEVICE) a span that does not fit is skipped
 * (out[i] = 0) and the call returns CRC32C_ERANGE (with CRC32C_ASYNC it cannot
 * report it: the out-of-range spans still read nothing and get 0).  A host
 * batch with such a span, a job of crc32c_batch_submit included, is refused
 * whole: CRC32C_EINVAL, nothing read, out untouched.  A batch of equal spans
 * at a fixed stride that overruns base_bytes is rejected up front
 * (CRC32C_EINVAL).  offsets / lens / crc_in / out hold n entries each.
 * Spans may come in any order and may overlap (chunked-item iov lists keep
 * their chain order; host batches are staged in offset order internally).
 * base needs no alignment, here and in every other call: a view into the
 * middle of a larger allocation gives the results its bytes give anywhere. */
typedef struct crc32c_spans {
    const void *base;
    uint64_t base_bytes;
    const uint64_t *offsets;
    uint64_t stride;
    const uint32_t *lens;
    uint32_t len;
    const uint32_t *crc_in;
    uint32_t *out;
    uint64_t n;
} crc32c_spans;

/* Number of usable gfx950 devices (0 when none): the visible HIP ordinals
 * that are gfx950, whatever other devices sit between them. */
int crc32c_gpu_count(void);

/* Checksum a batch.  Host batches are staged through pinned memory and the
 * call returns when out[] is filled.  Device batches are enqueued on `stream`
 * (a hipStream_t; NULL = the default stream) and, without CRC32C_ASYNC, the
 * call returns when they are done. */
int crc32c_batch(const crc32c_spans *spans, unsigned flags, void *stream);

/* Host batch split by bytes into `ngpus` parts (<= 0 or more than there are:
 * crc32c_gpu_count()); part g runs on the g-th gfx950 device in HIP ordinal
 * order, on that device's persistent worker thread, pinned H2D / D2H
 * overlapped with the kernels. */
int crc32c_batch_multi(const crc32c_spans *spans, int ngpus);

/* The split crc32c_batch_multi uses: parts + 1 cut points, part g owns spans
 * [cuts[g], cuts[g+1]).  cuts[g] is the first span index i whose byte prefix
 * sum(len[0..i)) reaches total * g / parts (total = every span's bytes), so
 * each part holds about total / parts bytes.  lens == NULL: every span is
 * `len` bytes.  (The Python twin is memcached_amd/shard.py plan().) */
int crc32c_shard_cuts(const uint32_t *lens, uint32_t len, uint64_t n, int parts, uint64_t *cuts);

/* Verify n item images of a packed page buffer (host or device per flags).
 * ok[i] = 1 when item i's CRC matches its stored exptime; *nbad receives the
 * number of mismatching (or malformed) items.  region_bytes is the write
 * buffer size: extstore never lets an item cross a wbuf (extstore.c:627-636),
 * so an image whose header claims to is malformed (0 = bound by base_bytes
 * only). */
int crc32c_verify_items(const void *base, uint64_t base_bytes, uint64_t region_bytes,
                        const uint64_t *item_offsets, uint64_t n, uint8_t *ok, uint64_t *nbad,
                        unsigned flags, void *stream);

/* Chained CRCs over iov lists: the chunked-item read verify of
 * storage.c:163-170, where crc = crc32c(0, hdr + 32, hdr_len - 32) and then
 * crc = crc32c(crc, chunk_x, len_x) for every chunk.  iovs describes every
 * iov of every chain (crc_in must be NULL; iovs->out receives each iov's own
 * CRC and must hold iovs->n entries); chain c is iovs [chain_first[c],
 * chain_first[c+1]) (nchains + 1 entries) and out[c] its chained CRC; a chain
 * of no iovs gets 0.  All arrays are host or device memory per flags, as for
 * crc32c_batch.  An iov outside the buffer is treated as crc32c_batch treats
 * the span: a device call skips it (its iovs->out entry is 0, CRC32C_ERANGE)
 * and the chain that contains it has an unspecified value, every other chain
 * its exact one; a host call is refused whole (CRC32C_EINVAL).  A host
 * chain_first that descends or passes iovs->n is refused (CRC32C_EINVAL); a
 * device chain_first is not validated: it must ascend and stay within
 * iovs->n, or the fold reads outside the arrays.  nchains == 0: CRC32C_OK,
 * nothing written. */
int crc32c_batch_chains(const crc32c_spans *iovs, const uint64_t *chain_first, uint64_t nchains,
                        uint32_t *out, unsigned flags, void *stream);

/* Verify whole pages with the walk done on the device: [base, base_bytes) is
 * a sequence of wbuf_bytes reads, each walked as storage_compact_readback does
 * (storage.c:950-1070: items packed from the read's start, nkey == 0 ends it,
 * next item at + ITEM_ntotal, stop when < 48 bytes remain) and every item
 * verified as crc32c_verify_items does (with region_bytes = wbuf_bytes).
 * base needs no alignment, and the wbuf_bytes pieces are counted from base
 * (piece w is [base + w * wbuf_bytes, + wbuf_bytes)), in this and in every
 * other page call (salvage, recover, triage, scrub, stamp).
 * *nitems = items found; the first min(cap, *nitems) offsets and ok flags are
 * written to offsets[] / ok[], in walk order, and *nbad counts every bad item.
 * cap == 0 is a count-only query: the walk runs, nothing is verified, *nbad =
 * 0 and offsets / ok may be NULL.  An item count is at most
 * base_bytes / 50 + ceil(base_bytes / wbuf_bytes) (an image is >= 50 bytes; a
 * wbuf's last counted image may run past its end).  Device scratch: the walk
 * keeps up to wbuf_bytes / 2048 offsets per wbuf (8 B each, 0.4 % of the
 * walked bytes; grow-only, reused by later calls). */
int crc32c_verify_pages(const void *base, uint64_t base_bytes, uint64_t wbuf_bytes,
                        uint64_t *offsets, uint8_t *ok, uint64_t cap, uint64_t *nitems,
                        uint64_t *nbad, unsigned flags, void *stream);

/* Find the intact images behind a damaged header.  The page walk finds images
 * one from the other, so one flipped header bit (nkey -> 0, a wrong nbytes or
 * it_flags) costs every image packed behind it in that wbuf, almost all of
 * them intact.  This call looks at every offset the walk's good images do not
 * cover as a possible image start and reports those whose stored CRC matches.
 *
 * The rule.  W = wbuf_bytes, cfl = 4 (8 with CRC32C_CFLAGS64); piece w is
 * [w W, min((w + 1) W, base_bytes)), as in crc32c_verify_pages.  For an offset o:
 *   sane(o)       what crc32c_verify_items requires of a header: at least 48
 *                 bytes left, nkey != 0, nbytes < 2^31, a span of at most
 *                 CRC32C_MAX_SPAN, the image (nt = ITEM_ntotal bytes) inside the
 *                 buffer and inside its own piece;
 *   candidate(o)  sane(o), nbytes >= 2 and the image's last two bytes "\r\n"
 *                 (every value memcached stores ends so; against random bytes a
 *                 plausible header passes once per 2^10 offsets of a 4 MiB wbuf,
 *                 with the CRLF once per 2^26);
 *   intact(o)     candidate(o) and crc32c(0, base + o + 32, nt - 32) equal to
 *                 the exptime field at o + 28.
 * The covered set C: every entry of walked[0, nwalked) with walked_ok[i] != 0
 * and sane(walked[i]) covers [walked[i], walked[i] + nt); an entry marked good
 * whose header is not sane covers nothing.  The lists are what
 * crc32c_verify_pages returned for the same buffer; with nwalked == 0 nothing is
 * covered and every intact image of the buffer is found from scratch.  Per
 * piece, from its first byte, while piece_end - o >= 48:
 *     o in C          ->  o = the end of the covering image
 *     else intact(o)  ->  report o;  o += nt
 *     else            ->  o += 1
 * The offsets reported are ascending, mutually disjoint and start outside every
 * covered image; a candidate inside a reported image is never reported.  A
 * look-alike inside the damaged image's own bytes can be: the caller's key
 * lookup with its offset check (storage.c:964-975) makes that, and a 2^-32 CRC
 * collision, harmless.
 *   *scanned (optional) = the eligible offsets: those o of any piece with
 *     piece_end - o >= 48 and o not in C;
 *   *ncand (optional) = the eligible offsets with candidate(o);
 *   both are exact and do not depend on how the search is carried out.
 * The work bound.  With work = the sum of nt - 32 over the eligible candidates,
 * work > CRC32C_SALVAGE_WORK_MAX * (scanned + W) verifies and reports nothing:
 * CRC32C_EWORK with *nfound = 0, *scanned and *ncand filled.  True images are
 * disjoint (at most `scanned` bytes in all) and real data yields less than one
 * false candidate per wbuf; only values crafted as overlapping fake headers
 * come near the bound, which keeps one call from becoming minutes of kernel
 * time.  Treat such a wbuf as the reference does.  (More than 2^32 - 2
 * candidates, possible only in such a buffer of several GiB, are refused the
 * same way.)
 * Outputs.  *nfound = the images found; the first min(cap, *nfound) offsets are
 * written to offsets[], nothing behind them; cap == 0 counts only (the CRCs are
 * still checked) and offsets may be NULL.
 * With CRC32C_DEVICE base, walked, walked_ok and offsets are device memory (the
 * three counts are always host words) and the call runs on `stream`; without
 * it everything is host memory and the buffer is staged as crc32c_verify_pages
 * stages it.  The counts are read back, so CRC32C_ASYNC has no effect.
 * CRC32C_EINVAL: NULL base or nfound, wbuf_bytes == 0, cap != 0 with NULL
 * offsets, nwalked != 0 with either list NULL, walked not strictly ascending or
 * an entry >= base_bytes (nothing is written; so base_bytes == 0 with a list that
 * is not empty), 2^31 - 1 pieces or more, 2^32 - 1 list entries or more.
 * base_bytes == 0 with nwalked == 0: CRC32C_OK with zero counts; no device:
 * CRC32C_ENODEV, nothing written.  Whatever the buffer
 * or the lists hold, no byte outside [base, base + base_bytes) is read beyond
 * the 16-byte granules of header bytes that the walk's own header reads touch,
 * and nothing but the outputs is written.  After the call
 * crc32c_last_kernel_ms() is the time of the scan's first pass over the
 * eligible bytes, the one that counts the candidates (0 when nothing was
 * eligible); the pass that writes them out reads the tiles that hold one again
 * and is not in it.  Scratch (grow-only): 24 B per 4 KiB of eligible bytes, 13 B per
 * candidate. */
#define CRC32C_SALVAGE_WORK_MAX 64
int crc32c_salvage_pages(const void *base, uint64_t base_bytes, uint64_t wbuf_bytes,
                         const uint64_t *walked, const uint8_t *walked_ok, uint64_t nwalked,
                         uint64_t *offsets, uint64_t cap, uint64_t *nfound, uint64_t *scanned,
                         uint64_t *ncand, unsigned flags, void *stream);

/* The whole read-back of a page in one call: crc32c_verify_pages followed by
 * crc32c_salvage_pages over its lists, the two results merged.  The buffer
 * crosses the link once, the walk's lists never leave the device, and the
 * caller runs one rescue loop.
 * The result is the composition of the two calls.  Let walked[], wok[] and
 * nbad_w be what crc32c_verify_pages(base, base_bytes, wbuf_bytes, ...) returns
 * with room for every item (nwalked of them), and found[], scanned, ncand what
 * crc32c_salvage_pages(base, ..., walked, wok, nwalked, ...) returns for them
 * (nfound of them).  The list is walked[] and found[] together, sorted ascending
 * by offset.  The offsets are distinct (a walked entry with wok == 0 is not
 * sane or fails its CRC, so the salvage does not find it); entries may overlap
 * in bytes: a bad walked entry may lie over salvaged images.  Per entry i:
 *   kind[i]  wok (0 or 1) for a walked entry, CRC32C_ITEM_SALVAGED for a found
 *            one; a rescue loop skips kind 0;
 *   lens[i]  ITEM_ntotal when the header at offsets[i] is sane as
 *            crc32c_verify_items judges it (region_bytes = wbuf_bytes), else 0;
 *            an image's span is at most CRC32C_MAX_SPAN, so 32 bits hold it.
 * Counts, always filled: *nitems = nwalked + nfound, *nbad = nbad_w,
 * *nsalvaged = nfound; *scanned and *ncand (both optional) as for
 * crc32c_salvage_pages.  The first min(cap, *nitems) entries of the merged list
 * are written to the three arrays, nothing behind them.  cap == 0: everything is
 * still computed, the counts are exact and the three arrays may be NULL; this
 * is crc32c_salvage_pages' rule, not crc32c_verify_pages' walk-only query.
 * CRC32C_EWORK (the salvage's work bound): the walk's entries alone are
 * written, with kinds 0 and 1; *nitems = nwalked, *nsalvaged = 0, *scanned and
 * *ncand are filled.  CRC32C_EWALK: as for crc32c_verify_pages (the walk's
 * entries and counts, not valid).  CRC32C_EINVAL: NULL base, nitems, nbad or
 * nsalvaged, wbuf_bytes == 0, cap != 0 with any array NULL, 2^31 - 1 pieces or
 * more.  base_bytes == 0: CRC32C_OK with zero counts; no device: CRC32C_ENODEV,
 * nothing written.
 * With CRC32C_DEVICE base and the three arrays are device memory (the five
 * counts are always host words) and the call runs on `stream`; without it
 * everything is host memory and the buffer is staged once.  CRC32C_CFLAGS64
 * applies as elsewhere; the counts are read back, so CRC32C_ASYNC has no effect.
 * Reads and writes are bounded as in the two calls: no byte outside [base,
 * base + base_bytes) is read beyond the 16-byte granules of header bytes that
 * the walk's own header reads touch, and nothing but the outputs is written.
 * After the call crc32c_last_kernel_ms() is the time of the scan's counting
 * pass, as after crc32c_salvage_pages.  Scratch (grow-only): the two calls',
 * 76 B per piece and, for a host call, 13 B per entry written. */
#define CRC32C_ITEM_SALVAGED 4 /* kind[]: not reached by the walk, proven by its stored CRC */
int crc32c_recover_pages(const void *base, uint64_t base_bytes, uint64_t wbuf_bytes, uint64_t *offsets,
                         uint32_t *lens, uint8_t *kind, uint64_t cap, uint64_t *nitems, uint64_t *nbad,
                         uint64_t *nsalvaged, uint64_t *scanned, uint64_t *ncand, unsigned flags,
                         void *stream);

/* crc32c_recover_pages with the damaged images the walk never reaches listed
 * too.  The salvage reports intact images only, so an image whose own bytes
 * were hit and that lies behind a header that ended its wbuf's walk is named
 * by neither list of crc32c_recover_pages, and crc32c_repair_items cannot be
 * handed it.  This call merges a third list in: the suspects, kind
 * CRC32C_ITEM_SUSPECT.
 * The rule.  walked[], wok[], found[], C, sane, candidate and intact are as
 * defined above for crc32c_recover_pages and crc32c_salvage_pages.  Per piece,
 * from its first byte, while piece_end - o >= 48:
 *     o in C                                        ->  o = the end of the covering image
 *     else intact(o)                                ->  found: report o;  o += nt
 *     else candidate(o) and o no entry of walked[]  ->  suspect: report o;  o += 1
 *     else                                          ->  o += 1
 * A suspect never moves the cursor by its length, which is not proven; so
 * found[] is exactly what crc32c_salvage_pages finds, and a candidate inside a
 * found image is never a suspect.  A walked entry with wok == 0 that is itself
 * a failing candidate is in the list already, as kind 0, and is not listed
 * twice.  The suspects ascend, are distinct from every walked and found
 * offset, may overlap each other and later entries in bytes, and number at
 * most ncand - nfound.
 * The list is walked[], found[] and the suspects together, ascending by
 * offset.  kind[i] is wok, CRC32C_ITEM_SALVAGED or CRC32C_ITEM_SUSPECT; lens[i]
 * as for crc32c_recover_pages, and a suspect's is its ITEM_ntotal, never 0 (a
 * candidate is sane).  *nitems = nwalked + nfound + nsuspect, *nbad = nbad_w,
 * *nsalvaged = nfound, *nsuspect (required) = the suspects.  With the
 * kind-CRC32C_ITEM_SUSPECT entries taken out, the three arrays, *nbad,
 * *nsalvaged, *scanned, *ncand and the return code are crc32c_recover_pages'
 * for the same buffer.
 * A suspect is evidence of nothing but a plausible header and a CRLF: a rescue
 * loop skips it, as it skips kind 0.  It is a candidate for
 * crc32c_repair_items, whose proof (one bit that makes the stored CRC match) is
 * then the only one it has; filter overlapping suspects first (INTEGRATION.md
 * section 4g).
 * Everything else is crc32c_recover_pages': cap (0 still computes everything,
 * the arrays may be NULL; the first min(cap, *nitems) entries are written,
 * nothing behind them); CRC32C_EWORK (the walk's entries alone, *nitems =
 * nwalked, *nsalvaged = *nsuspect = 0, *scanned and *ncand filled);
 * CRC32C_EWALK; CRC32C_EINVAL (NULL base, nitems, nbad, nsalvaged or nsuspect,
 * wbuf_bytes == 0, cap != 0 with any array NULL, 2^31 - 1 pieces or more);
 * base_bytes == 0 (CRC32C_OK with zero counts); no device (CRC32C_ENODEV,
 * nothing written); CRC32C_DEVICE (base and the three arrays are device
 * memory, the six counts host words) and host staging (the buffer is staged
 * once); CRC32C_CFLAGS64; CRC32C_ASYNC has no effect; the read and write
 * bounds; crc32c_last_kernel_ms() is the time of the scan's counting pass.
 * No pass over the page's bytes is added: the candidates and their CRCs are
 * the ones crc32c_recover_pages computes and drops.  Scratch (grow-only):
 * crc32c_recover_pages', 1 B per candidate (the kind byte of a picked entry)
 * and 4 B per piece.
 * crc32c_salvage_pages has no such mode: it returns no kind array to tell a
 * suspect from an image found.
 * call_flags is the flags word of crc32c_recover_pages, bit for bit.  It has a
 * name of its own because tests/test_interleave_cases.py and
 * tests/test_header_interleave_cases.py count the declarations with a parameter
 * called flags and pin them at the entry points of their own two op tables;
 * tests/test_triage_interleave_cases.py counts a flags word under any name and
 * holds this call to the third table. */
#define CRC32C_ITEM_SUSPECT 6 /* kind[]: not reached by the walk, a candidate whose stored CRC does not match */
int crc32c_triage_pages(const void *base, uint64_t base_bytes, uint64_t wbuf_bytes, uint64_t *offsets,
                        uint32_t *lens, uint8_t *kind, uint64_t cap, uint64_t *nitems, uint64_t *nbad,
                        uint64_t *nsalvaged, uint64_t *nsuspect, uint64_t *scanned, uint64_t *ncand,
                        unsigned call_flags, void *stream);

/* Correct single-bit damage from the stored CRC.  An image whose own bytes were
 * hit comes back as kind 0 from the walk, as CRC32C_ITEM_DAMAGED from
 * crc32c_copy_items, as badcrc_from_extstore on the read path, and is dropped.
 * When exactly one bit of it is inverted, the bits that say which one are still
 * in it: this call finds the bit, inverts it again and so proves the image.
 *
 * The rule, per image at o = item_offsets[i].  The image is judged sane exactly
 * as crc32c_verify_items judges it (region_bytes and CRC32C_CFLAGS64 apply).
 * nt = ITEM_ntotal, L = nt - 32, c = crc32c(0, base + o + 32, L), e = the
 * little-endian dword at o + 28, S = c ^ e.
 *   not sane, or L > max_span   ok = 0, bit = CRC32C_NO_BIT, nothing written.
 *                               max_span == 0 means CRC32C_REPAIR_SPAN_DEFAULT;
 *                               max_span > CRC32C_REPAIR_SPAN_MAX: CRC32C_EINVAL.
 *   S == 0                      ok = 1, bit = CRC32C_NO_BIT.
 *   otherwise                   the positions are the image's bits k in
 *     [224, 8 nt): bit k % 8 (LSB = 0) of image byte k / 8 -- the stored CRC and
 *     every byte it covers.  k is located when the image with bit k inverted
 *     has a stored CRC equal to its computed one.  In syndrome form: g(0) =
 *     0x80000000, g(t + 1) = (g(t) >> 1) ^ (g(t) & 1 ? 0x82F63B78 : 0);
 *     stored-CRC bit j (k = 224 + j) has t = 31 - j, bit b of span byte m (k =
 *     256 + 8 m + b) has t = 32 + 8 (L - 1 - m) + (7 - b); k is located iff
 *     g(t) == S.  At most one k exists.
 *     A located k is accepted when (1) it is not a length-determining header
 *     bit -- nbytes (bytes 32..35), nkey (byte 41), it_flags bits 1 and 8 (byte
 *     38 bit 1, byte 39 bit 0): inverting one changes nt, so the image would not
 *     verify over its own span -- and (2) with the bit inverted nbytes >= 2 and
 *     the image's last two bytes are "\r\n" (crc32c_salvage_pages' candidate
 *     rule).
 *     accepted                  ok = CRC32C_ITEM_REPAIRED, bit = k; without
 *                               CRC32C_LOCATE_ONLY that one bit of the buffer
 *                               is inverted, so the image then passes
 *                               crc32c_verify_items.
 *     not located / accepted    ok = 0, bit = CRC32C_NO_BIT, nothing written.
 * *nrepaired counts ok == CRC32C_ITEM_REPAIRED and *nbad counts ok == 0; both are
 * always filled.  ok and bit hold n entries.
 *
 * What the rule guarantees, and why.  A register holds a polynomial mod
 * P = 0x11EDC6F41 (reflected: 0x80000000 is 1, g(t) = x^t).  The stored CRC
 * followed by the span is a codeword exactly when S == 0, S is linear in the
 * codeword's bits, and inverting the bit with exponent t alone gives S = x^t.
 *   - P has 18 terms, so x + 1 divides it and every codeword has even weight:
 *     an error pattern of even weight has S divisible by x + 1, a power of x
 *     never is.  Damage of any even number of bits inside [o + 28, o + nt) is
 *     therefore never "repaired".
 *   - x has order 2^31 - 1 mod P (x^(2^31 - 1) = 1 and 2^31 - 1 is prime), and a
 *     codeword of L <= CRC32C_REPAIR_SPAN_MAX bytes has 32 + 8 L < 2^31 - 1
 *     positions: their x^t are distinct.  One inverted bit there is always
 *     located, at its own position and no other, and accepted unless it is a
 *     length bit.
 *   - Damage of any other kind (three or more bits, a wrong length) leaves an S
 *     that is as good as random: it is taken for a single bit with probability
 *     about (8 nt - 224) / 2^32 per damaged image -- 2^-17 (8e-6) for a 4 KiB
 *     image, 2^-9 (2e-3) for a 1 MiB one, 2^-8 at the default max_span.  The
 *     CRLF test multiplies that by 2^-16 only where the damage moved the
 *     image's end.  The caller chooses max_span with that in mind.
 * A repaired image is thus weaker evidence than an intact one: a separate,
 * explicit call, not a mode of the verify.
 *
 * The work bound.  The list is expected to name distinct, disjoint images, as
 * the walk's lists do.  If the spans of the images with S != 0 and L <= max_span
 * add up to more than base_bytes (disjoint images cannot), the call returns
 * CRC32C_EWORK: nothing is written into the buffer, ok and bit are unspecified,
 * *nrepaired = 0.  An offset listed twice below that bound leaves that one
 * image's content unspecified and touches nothing else.
 *
 * With CRC32C_DEVICE base, item_offsets, ok and bit are device memory and the
 * call runs on `stream`; the two counts are host words, read back, so
 * CRC32C_ASYNC has no effect.  Without it everything is host memory: the buffer
 * is staged as crc32c_verify_items stages it and the host inverts the located
 * bits in the caller's buffer.  CRC32C_EINVAL: NULL base, item_offsets, ok, bit,
 * nrepaired or nbad.  n == 0: CRC32C_OK with zero counts; no device:
 * CRC32C_ENODEV, nothing written.  No byte outside [base, base + base_bytes) is
 * read beyond what crc32c_verify_items reads; nothing but the outputs and the
 * accepted bits is written.  After the call crc32c_last_kernel_ms() is the time
 * of the search kernel alone (0 when no image had S != 0).  Scratch
 * (grow-only): 20 B per image beside crc32c_verify_items' own (a host call 17 B
 * more and the staged buffer), 32 B per image with S != 0. */
#define CRC32C_ITEM_REPAIRED 5 /* ok[]: one bit located (and, without CRC32C_LOCATE_ONLY, flipped back) */
#define CRC32C_NO_BIT UINT64_MAX
#define CRC32C_REPAIR_SPAN_DEFAULT 0x200000u /* 2 MiB */
#define CRC32C_REPAIR_SPAN_MAX 0x0fffffc0u   /* 32 + 8 L < 2^31 - 1: the located position is unique */
int crc32c_repair_items(void *base, uint64_t base_bytes, uint64_t region_bytes,
                        const uint64_t *item_offsets, uint64_t n, uint32_t max_span,
                        uint8_t *ok, uint64_t *bit, uint64_t *nrepaired, uint64_t *nbad,
                        unsigned flags, void *stream);

/* The same search for one span on the host, no GPU: after a scalar mismatch of
 * a read (storage.c:172-178, io_depth 1).  crc_computed = crc32c(0, span, len),
 * crc_stored what the item carries.  Returns q < 32 for bit q of the stored CRC
 * and q >= 32 for bit (q - 32) % 8 of span byte (q - 32) / 8; CRC32C_NO_BIT when
 * the two CRCs are equal, when no position of a len-byte span explains them, or
 * when len > CRC32C_REPAIR_SPAN_MAX.  For an item image k = 224 + q; the
 * length-bit and CRLF conditions are the caller's.  4 + len table steps. */
uint64_t crc32c_locate_bit(uint32_t crc_computed, uint32_t crc_stored, uint64_t len);

/* Restore one damaged byte from the stored CRC.  crc32c_repair_items and every
 * flow built on it handle exactly one inverted bit; an image with two or more
 * bits inverted inside ONE byte (a failed x8 DRAM device, a stuck lane, a torn
 * byte) is dropped by all of them.  This call finds that byte and its XOR mask
 * by the same search and puts the byte back.
 *
 * The rule, per image at o = item_offsets[i], in crc32c_repair_items' terms
 * (sanity as crc32c_verify_items judges it, nt, L = nt - 32, c, e, S = c ^ e):
 *   not sane, or L > max_span   ok = 0, byte = CRC32C_NO_BIT, mask = 0, nothing
 *                               written.  max_span == 0 means
 *                               CRC32C_REPAIR_BYTES_SPAN_DEFAULT; max_span >
 *                               CRC32C_REPAIR_BYTES_SPAN_MAX: CRC32C_EINVAL.
 *   S == 0                      ok = 1, byte = CRC32C_NO_BIT, mask = 0.
 *   otherwise                   a pair (p, m) is located when p is an image
 *     byte in [28, nt), m is in 1..255 and the image with byte p XORed by m has
 *     a stored CRC equal to its computed one.  At most one pair exists (below).
 *     A located pair is accepted when (1) m inverts no length-determining bit
 *     -- p is not 32..35 or 41, not 38 with m & 0x02, not 39 with m & 0x01:
 *     crc32c_repair_items' condition applied to each inverted bit -- and (2)
 *     with the byte corrected nbytes >= 2 and the image's last two bytes are
 *     "\r\n".
 *     accepted                  ok = CRC32C_ITEM_REPAIRED, byte = p, mask = m
 *                               (LSB = bit 0 of the byte); without
 *                               CRC32C_LOCATE_ONLY that one byte of the buffer
 *                               is XORed with m, so the image then passes
 *                               crc32c_verify_items.
 *     not located / accepted    ok = 0, byte = CRC32C_NO_BIT, mask = 0, nothing
 *                               written.
 * out->nrepaired counts ok == CRC32C_ITEM_REPAIRED and out->nbad counts ok == 0.
 *
 * What the rule guarantees.  In the syndrome form of crc32c_repair_items, V_j =
 * S x^(-8 j) is non-zero and confined to the register's top byte exactly when
 * the error pattern lies in the codeword byte of step j (step j < 4: stored-CRC
 * byte 3 - j; step j >= 4: span byte L + 3 - j), and V_j >> 24 is that byte's
 * mask.  Two one-byte patterns B and B' that lie d bytes apart share a syndrome
 * iff B = B' x^(8 d) mod P.  Over all 255 patterns the smallest such d is
 * 190 235 (0xdf against 0x4c; tests/integration/repair_bytes_check.cpp
 * recomputes it).  So in a codeword of 4 + L <= 190 235 bytes -- L <=
 * CRC32C_REPAIR_BYTES_SPAN_MAX -- damage confined to one byte is always
 * located, at its own byte with its own mask and nowhere else, and accepted
 * unless it inverts a length bit.  The single-bit masks are among the 255:
 * within that bound the call finds everything crc32c_repair_items finds, at
 * the same bit.
 *
 * The evidence is weaker, and that is the price.
 *   - A syndrome that is as good as random passes for a one-byte error with
 *     probability 255 (4 + L) / 2^32: 2^-12 for a 4 KiB image where the one-bit
 *     rule has 2^-17, 2^-8 at the default max_span of 64 KiB -- 32 times the
 *     one-bit rule's odds at equal length (255 patterns a byte against 8).
 *   - The even-weight guarantee is gone.  Two inverted bits in DIFFERENT bytes,
 *     which crc32c_repair_items never takes for a repair, are taken for a
 *     one-byte error with that same probability.
 * An image repaired by this call is the weakest evidence any call here gives:
 * a separate, explicit call, not a mode of anything.  Run it after
 * crc32c_repair_items on what is still 0, or instead of it where those odds
 * are acceptable.  Damage spread over two bytes is
 * not located; crc32c_scrub_pages uses this call only where the caller sets
 * CRC32C_SCRUB_BYTES, and logs its repairs apart (CRC32C_SCRUB_BY_BYTE).
 *
 * Everything else is crc32c_repair_items': the work bound (the spans of the
 * images with S != 0 and L <= max_span add up to more than base_bytes:
 * CRC32C_EWORK, nothing written into the buffer, both counts 0); with
 * CRC32C_DEVICE base, item_offsets and the three arrays are device memory and
 * the call runs on opts->stream, the two counts are host words, read back, so
 * CRC32C_ASYNC has no effect; without it the buffer is staged, the kernels run
 * with the write off and the host applies the masks to the caller's buffer.
 * CRC32C_EINVAL: NULL base, item_offsets, out, or any of the three arrays.
 * n == 0: CRC32C_OK with zero counts.  No device: CRC32C_ENODEV, and neither
 * `out` nor any array is written.  The read and write bounds are the same.
 * After the call crc32c_last_kernel_ms() is the time of the search kernel alone
 * (0 when no image had S != 0).  Scratch (grow-only): crc32c_repair_items', and
 * a host call 2 B per image more. */
#define CRC32C_REPAIR_BYTES_SPAN_MAX 190231u      /* 4 + L <= 190235: the located byte is unique */
#define CRC32C_REPAIR_BYTES_SPAN_DEFAULT 0x10000u /* 255 (4 + L) / 2^32 = 2^-8, crc32c_repair_items' odds at its default */

typedef struct crc32c_bytes_opts { /* NULL: all zero */
    uint32_t mode;     /* CRC32C_DEVICE | CRC32C_CFLAGS64 | CRC32C_LOCATE_ONLY; others ignored */
    uint32_t max_span; /* 0: the default; above CRC32C_REPAIR_BYTES_SPAN_MAX: CRC32C_EINVAL */
    void *stream;
} crc32c_bytes_opts;

typedef struct crc32c_bytes_out {
    /* in: n entries each (device memory with CRC32C_DEVICE) */
    uint8_t *ok;
    uint64_t *byte; /* image byte index, CRC32C_NO_BIT when none */
    uint8_t *mask;  /* XOR mask of that byte, LSB = bit 0; 0 when none */
    /* out: always filled, host words */
    uint64_t nrepaired, nbad;
} crc32c_bytes_out;

int crc32c_repair_bytes(void *base, uint64_t base_bytes, uint64_t region_bytes,
                        const uint64_t *item_offsets, uint64_t n,
                        const crc32c_bytes_opts *opts, crc32c_bytes_out *out);

/* The same search for one span on the host, no GPU.  Returns the codeword byte
 * p -- p < 4: stored-CRC byte p, p >= 4: span byte p - 4; image byte 28 + p --
 * with its XOR mask in *mask (optional), or CRC32C_NO_BIT with *mask = 0 when
 * the two CRCs are equal, when no byte of a len-byte span explains them, or
 * when len > CRC32C_REPAIR_BYTES_SPAN_MAX.  The length-bit and CRLF conditions
 * are the caller's.  4 + len table steps. */
uint64_t crc32c_locate_byte(uint32_t crc_computed, uint32_t crc_stored, uint64_t len, uint8_t *mask);

/* Undo a flipped length bit in an item header.  crc32c_repair_items leaves the
 * 42 header bits that decide ITEM_ntotal alone: with one of them inverted the
 * image's span is no longer the one its CRC was made over.  That image is also
 * the one whose header derailed its wbuf's walk.  This call tries the 42
 * headers one such bit away, each with its own span and CRC.
 *
 * The rule, per listed offset o = item_offsets[i].  Sanity is
 * crc32c_verify_items' (region_bytes and CRC32C_CFLAGS64 apply); e is the
 * little-endian dword at o + 28.  The 42 length bits, by image bit index k (bit
 * k % 8, LSB = 0, of image byte k / 8): 256..287 (nbytes), 328..335 (nkey), 305
 * (it_flags bit 1, ITEM_CAS), 312 (it_flags bit 8, ITEM_CFLAGS).
 *   fewer than 48 bytes left, or o >= base_bytes
 *                      ok = 0, bit = CRC32C_NO_BIT, lens = 0; nothing is read.
 *   as it stands       the header is sane and crc32c(0, base + o + 32, nt - 32) ==
 *                      e: ok = 1, bit = CRC32C_NO_BIT, lens = nt (no CRLF is
 *                      demanded: crc32c_verify_items' verdict).
 *   otherwise          variant k is the header with bit k inverted, nt' its
 *     ITEM_ntotal.  It is a candidate when that header is sane, nbytes' >= 2 and
 *     the bytes at o + nt' - 2 and o + nt' - 1 are "\r\n" (crc32c_salvage_pages'
 *     candidate rule; bit k lies inside the span's first ten bytes, so the two
 *     end bytes are as the buffer has them).  A candidate hits when crc32c(0,
 *     the span [o + 32, o + nt') with bit k inverted) == e.
 *     exactly one hit  ok = CRC32C_ITEM_REPAIRED, bit = k, lens = nt'; without
 *                      CRC32C_LOCATE_ONLY that one bit of the buffer is inverted,
 *                      so the image then passes crc32c_verify_items.
 *     none, or several ok = 0, bit = CRC32C_NO_BIT, lens = 0, nothing written: an
 *                      ambiguous header is not guessed at.
 * *nrepaired counts ok == CRC32C_ITEM_REPAIRED and *nbad counts ok == 0; both are
 * always filled.  ok, bit and lens hold n entries.
 *
 * The evidence.  Not a syndrome search over 8 nt positions: 42 comparisons of
 * full 32-bit CRCs, each also gated by the CRLF.  A false repair costs about
 * 42 * 2^-32 per header at any image length (crc32c_repair_items: 2^-17 for a
 * 4 KiB image).  So repair headers first, then crc32c_repair_items on what is
 * still 0, then walk the repaired wbufs again: with its header right, a wbuf's
 * walk finds everything behind it without a salvage.
 *
 * Which offsets to list is the caller's choice.  From crc32c_recover_pages'
 * output: every kind == 0 entry, with lens 0 or not; and each piece's walk end
 * when it is not itself an entry (a flip of nkey to 0 ends the walk without
 * listing the header) -- the end of the piece's last walked entry when that
 * entry is good, or the piece's start when the piece has no entry -- when at
 * least 48 bytes remain there (INTEGRATION.md section 4f has the loop).  A
 * salvaged look-alike inside a repaired image's bytes is the caller's to drop.
 *
 * The work bound.  work = the spans of every candidate variant.  work >
 * CRC32C_HEADER_WORK_MAX * base_bytes: CRC32C_EWORK, nothing is written into the
 * buffer, the three arrays are unspecified and both counts are 0.  The true
 * variants of distinct images are disjoint, at most base_bytes together; every
 * other variant needs a CRLF at one fixed place.  8 leaves room: a cap, not a
 * tuned number.  What the cap limits is the call's own multiplication of work,
 * up to 42 spans per listed header, which crafted values could otherwise steer.
 * What it does not limit: the as-it-stands span of every listed header that is
 * sane is read once as well and is not in the sum (a header whose flipped
 * nbytes bit still leaves it sane claims a long one honestly).  That part is
 * exactly what crc32c_verify_items reads of the same list and, as there,
 * unbounded: at most n * min(region_bytes, base_bytes) bytes, so a caller who
 * lists one sane header many times, or overlapping ones, pays for each entry.
 * Lists built from a walk name disjoint entries and stay within base_bytes.
 * An offset listed twice below the bound leaves that image's content
 * unspecified and touches nothing else.
 *
 * With CRC32C_DEVICE base, item_offsets, ok, bit and lens are device memory and
 * the call runs on `stream`; the two counts are host words, read back, so
 * CRC32C_ASYNC has no effect.  Without it everything is host memory: the buffer
 * is staged as crc32c_repair_items stages it and the host inverts the accepted
 * bits in the caller's buffer.  CRC32C_EINVAL: NULL base, item_offsets, ok, bit,
 * lens, nrepaired or nbad; 43 n >= 2^32 - 1.  n == 0: CRC32C_OK with zero counts;
 * no device: CRC32C_ENODEV, nothing written.  Reads and writes are bounded as in
 * crc32c_repair_items.  After the call crc32c_last_kernel_ms() is the time of
 * the pass that finds and counts the candidate variants (0 for n == 0); the
 * pass that writes them out is not in it.  Scratch (grow-only): 8 B per header
 * (a host call 21 B more and the staged buffer), 24 B per candidate beside the
 * span kernels' own. */
#define CRC32C_HEADER_BITS 42
#define CRC32C_HEADER_WORK_MAX 8
int crc32c_repair_headers(void *base, uint64_t base_bytes, uint64_t region_bytes,
                          const uint64_t *item_offsets, uint64_t n,
                          uint8_t *ok, uint64_t *bit, uint32_t *lens,
                          uint64_t *nrepaired, uint64_t *nbad,
                          unsigned int flags, void *stream);

/* A page's whole repair flow in one call: crc32c_triage_pages, rounds of
 * crc32c_repair_headers over the list that INTEGRATION.md section 4f builds
 * from it, crc32c_repair_items over the list of section 4g, and the triage
 * again after every round that repaired something, until nothing more can be
 * repaired.  The page crosses the link once, the lists between the stages
 * stay on the device, and the caller gets the final triage list and a log of
 * every bit that was inverted.
 *
 * The rule is a composition of the three calls and nothing else.  With
 * region_bytes = wbuf_bytes, the CRC32C_CFLAGS64 bit of opts->mode and the
 * repairs writing in place:
 *
 *   header_list(T): per piece every kind-0 entry, then the piece's walk end
 *     (the end of its last walked entry, kinds 4 and 6 skipped; the piece's
 *     start when it has none) when that entry is not kind 0 and at least 48
 *     bytes of the piece remain there;
 *   item_list(T): every entry with kind == 0 && lens != 0, and every suspect
 *     that ends at or before the next kind-1 or kind-4 entry and starts at or
 *     behind the end of the last suspect kept, in one ascending list;
 *
 *   T = triage
 *   loop: T failed (CRC32C_EWORK, CRC32C_EWALK): return its status, T is what
 *           crc32c_triage_pages returns then;
 *         h = repair_headers(header_list(T)); h failed: return its status (it
 *           wrote nothing, T still describes the page);
 *         h repaired something: log its flips, one more round, T = triage,
 *           stop at max_rounds, else start the loop again (headers before
 *           items, every time);
 *         i = repair_items(item_list(T), max_span); i failed: return its status;
 *         i repaired nothing: complete = 1, stop (T describes the page);
 *         log its flips, one more round, T = triage, stop at max_rounds.
 *
 * CRC32C_SCRUB_GAPS in opts->mode (opt-in; with the bit clear the call is
 * exactly the above) changes how the two lists are built and nothing else.
 * An image with one flipped length bit, or one flipped bit of its final CRLF,
 * behind a header that ended its wbuf's walk is no candidate of the scan (its
 * end is wrong, or it has no CRLF), so T never names its offset.  But extstore
 * packs images back to back: it starts where the image in front of it ends,
 * and when that one is proven, its end is the offset nobody names.
 *
 *   gap_starts(T): for every kind-4 entry (o, len) of T, e = o + len, when e
 *     is the offset of no entry of T of any kind and at least 48 bytes of o's
 *     piece remain at e; ascending, each once.  (The end of a kind-1 entry
 *     needs no rule: it is the next walked entry or the piece's walk end,
 *     which header_list has.)
 *   header_list'(T): header_list(T) and gap_starts(T) in one ascending list,
 *     each offset once.
 *   item_list'(T): item_list applied to T with every gap start g whose header
 *     is sane (as crc32c_verify_items judges it with region_bytes =
 *     wbuf_bytes; nt its ITEM_ntotal) merged in by offset as a suspect of
 *     length nt: kept when it ends at or before the next kind-1 or kind-4
 *     entry and starts at or behind the end of the last suspect or gap start
 *     kept.  A gap start that is not sane is not listed for the items.
 *
 * The loop, the round count, the log, complete, max_rounds,
 * CRC32C_LOCATE_ONLY, the host staging, the error codes and the fixpoint
 * property are unchanged: a header repaired at a gap start is logged with
 * CRC32C_SCRUB_BY_HEADER, an item repaired there with CRC32C_SCRUB_BY_ITEM.
 * The next triage finds a repaired gap image as kind 4, so its end is the
 * next gap start: a run of k consecutive such images takes k rounds.  An
 * image directly behind the dead header itself stays lost: nothing proven
 * ends where it starts.  The rule adds no evidence and weakens none: each
 * listed header still costs 42 * 2^-32 and each listed item (8 nt - 224) /
 * 2^32, and at most nsalvaged more offsets are listed per round.  The item
 * rule reads the header at a gap start, where at least 48 bytes of the piece
 * remain (as the walk reads a header: the 16-byte granules of its bytes
 * 28..43).  The other entry points ignore the bit.
 *
 * CRC32C_SCRUB_BYTES in opts->mode (opt-in; with the bit clear the call is
 * exactly the above; it composes with CRC32C_SCRUB_GAPS) adds a third stage
 * to the loop and nothing else: crc32c_repair_bytes, for the images whose
 * damage is several bits of one byte, which the item stage drops.  The step
 * "i repaired nothing: complete = 1, stop" becomes
 *
 *         i repaired nothing:
 *           b = repair_bytes(L, bspan), in place, over the SAME list L the
 *             item stage just ran on (item_list(T), or item_list'(T) with
 *             CRC32C_SCRUB_GAPS); b failed: return its status;
 *           b repaired nothing: complete = 1, stop (T describes the page);
 *           log its flips, one more round, T = triage, stop at max_rounds,
 *           else start the loop again (headers, then items, then bytes,
 *           every time).
 *
 * bspan = CRC32C_REPAIR_BYTES_SPAN_DEFAULT when opts->max_span == 0, else
 * min(opts->max_span, CRC32C_REPAIR_BYTES_SPAN_DEFAULT): the stage never
 * searches longer spans than crc32c_repair_bytes does by default, and a caller
 * who wants longer ones at worse odds makes that call themselves.  bspan is at
 * most the item stage's resolved limit, so the byte stage's work sum is at
 * most the item stage's over the same list and bytes: it cannot return
 * CRC32C_EWORK where the item stage did not (a status that comes all the same
 * is returned as any stage's is).
 *
 * The log stays one entry per inverted bit.  An image repaired at byte p with
 * mask m contributes popcount(m) consecutive entries, in ascending bit order:
 * flip_offsets = the image's offset, flip_bits = 8 p + b for every set bit b
 * of m, flip_by = CRC32C_SCRUB_BY_BYTE; the images of a stage in list order.
 * So the log's meaning holds (buffer bit 8 * offset + index; replaying the log
 * on the damaged page gives the result), and flip_cap may cut between two bits
 * of one byte: the first min(flip_cap, nflips) entries are written, nothing
 * behind them, and nflips is exact.  nflips counts bits.  rounds counts the
 * repair calls that repaired something, the byte stage's among them.
 * items_repaired counts the images repaired by the item stage and the byte
 * stage together (the struct has no room for a count of its own); the byte
 * stage's share is the number of distinct flip_offsets among the
 * CRC32C_SCRUB_BY_BYTE entries of the log.  With the bit set nflips ==
 * headers_repaired + items_repaired no longer holds.  A single inverted bit is
 * the item stage's, as before, and logged CRC32C_SCRUB_BY_ITEM: the byte stage
 * runs only when the item stage repaired nothing.
 *
 * complete and the fixpoint property (a second call with the same mode on the
 * result inverts nothing and returns the same list), max_rounds,
 * CRC32C_LOCATE_ONLY (host only), the host staging, the error codes, the read
 * and write bounds and crc32c_last_kernel_ms are unchanged.  The evidence is
 * that of the calls composed: an image logged CRC32C_SCRUB_BY_BYTE carries
 * crc32c_repair_bytes' odds, 255 (4 + L) / 2^32 with no even-weight guarantee,
 * and suspects and gap starts, which nothing else proves, are handed to it
 * too: the weakest evidence the scrub can give.  The log tells such images
 * apart.  The other entry points ignore the bit.
 *
 * Outputs. offsets / lens / kind take the first min(cap, nitems) entries of
 * the last T, and nitems, nbad, nsalvaged, nsuspect, scanned and ncand are
 * its counts, all as crc32c_triage_pages reports them.  The log has one entry
 * per bit inverted, in the order made (round by round, in a round in list
 * order): flip_offsets[r] the image's offset, flip_bits[r] the image's bit
 * index as the repair call reported it (buffer bit 8 * offset + index),
 * flip_by[r] the stage; its first min(flip_cap, nflips) entries are written.
 * Nothing is written behind either, cap == 0 or flip_cap == 0 means those
 * arrays may be NULL, and every count is exact whatever the caps are.  With
 * CRC32C_DEVICE the six arrays are device memory; the counts are host words.
 * rounds counts the repair calls that repaired something.
 *
 * complete == 1: the flow ended because nothing more could be repaired.  The
 * result is then a fixpoint: a second call on the result inverts nothing and
 * returns the same list.  complete == 0 with CRC32C_OK: max_rounds (0:
 * CRC32C_SCRUB_ROUNDS_DEFAULT) was reached; what was repaired stays repaired
 * and is logged.
 *
 * A host buffer (no CRC32C_DEVICE) is staged once, every stage runs on the
 * staged copy, and at the end the host inverts the logged bits in the
 * caller's buffer, whatever flip_cap is.  With CRC32C_LOCATE_ONLY those
 * inversions are left out: the list and the log describe the page as it
 * would be and the caller's bytes are untouched.  A device buffer with
 * CRC32C_LOCATE_ONLY is CRC32C_EINVAL: the rounds need the earlier flips in
 * place and the library keeps no second copy of a device page.
 *
 * Evidence.  Exactly that of the calls composed: a header repair is wrong
 * with probability 42 * 2^-32 per header, an item repair with (8 nt - 224) /
 * 2^32 per item (see crc32c_repair_headers and crc32c_repair_items).  A
 * caller who wants to treat repaired images apart finds them through the log.
 *
 * CRC32C_EINVAL: NULL base or out, wbuf_bytes == 0, cap or flip_cap non-zero
 * with one of its arrays NULL, max_span above CRC32C_REPAIR_SPAN_MAX, 2^31 - 1
 * pieces or more, a header list longer than crc32c_repair_headers takes.
 * base_bytes == 0: CRC32C_OK, zero counts, complete = 1.  No device:
 * CRC32C_ENODEV, and neither `out` nor any array is written, not even partly
 * (CRC32C_EINVAL, CRC32C_ENOMEM and CRC32C_EHIP write nothing into `out`
 * either).  CRC32C_ASYNC has no effect.  Reads and writes stay inside the
 * bounds of the three calls.  crc32c_last_kernel_ms: the last triage's
 * counting pass.
 *
 * Scratch (grow-only) beyond that of the three calls: per entry of the merged
 * list 13 B (the whole list stays on the device, not its first cap entries);
 * per piece 8 B of count and scan; per entry of a repair list 8 B of offset
 * and the repair calls' 9 B (items) or 13 B (headers) of verdicts; a host
 * call: the staged page and 17 B per flip of a round.  With
 * CRC32C_SCRUB_GAPS: 12 B per gap start, and where a triage has any, 14 B per
 * entry of the merged list and its gap starts together.  With
 * CRC32C_SCRUB_BYTES: 1 B of mask per item-list entry, a host call 8 flip
 * slots per image a byte stage repaired instead of 1, and one 8-byte count
 * read back per byte stage that repaired something. */
#define CRC32C_SCRUB_ROUNDS_DEFAULT 64
#define CRC32C_SCRUB_BY_HEADER 1 /* flip_by[]: made by the crc32c_repair_headers stage */
#define CRC32C_SCRUB_BY_ITEM 2   /* flip_by[]: made by the crc32c_repair_items stage */
#define CRC32C_SCRUB_BY_BYTE 3   /* flip_by[]: made by the crc32c_repair_bytes stage */
#define CRC32C_SCRUB_GAPS 0x40u  /* crc32c_scrub_opts.mode: list the gap starts too (above); other calls ignore it */
#define CRC32C_SCRUB_BYTES 0x80u /* crc32c_scrub_opts.mode: the crc32c_repair_bytes stage (above); other calls ignore it */

typedef struct crc32c_scrub_opts { /* NULL: all zero */
    uint32_t mode;       /* CRC32C_DEVICE | CRC32C_CFLAGS64 | CRC32C_LOCATE_ONLY | CRC32C_SCRUB_GAPS | CRC32C_SCRUB_BYTES; others ignored */
    uint32_t max_span;   /* crc32c_repair_items' max_span, same meaning, same CRC32C_EINVAL */
    uint32_t max_rounds; /* 0: CRC32C_SCRUB_ROUNDS_DEFAULT */
    void *stream;
} crc32c_scrub_opts;

typedef struct crc32c_scrub_out {
    /* in: the caller's arrays (device memory with CRC32C_DEVICE) and their room */
    uint64_t *offsets;
    uint32_t *lens;
    uint8_t *kind;
    uint64_t cap;
    uint64_t *flip_offsets;
    uint64_t *flip_bits;
    uint8_t *flip_by;
    uint64_t flip_cap;
    /* out: always filled, host words */
    uint64_t nitems, nbad, nsalvaged, nsuspect, scanned, ncand; /* the final list's, as crc32c_triage_pages' */
    uint64_t nflips, headers_repaired, items_repaired;
    uint32_t rounds;   /* repair calls that repaired something */
    uint32_t complete; /* 1: the flow ended because nothing more could be repaired */
} crc32c_scrub_out;

int crc32c_scrub_pages(void *base, uint64_t base_bytes, uint64_t wbuf_bytes,
                       const crc32c_scrub_opts *opts, crc32c_scrub_out *out);

/* Stamp the spill CRC of n item images (storage.c:567, gathered per wbuf
 * before it is submitted): exptime (bytes 28..31) of image i receives
 * crc32c(0, image + 32, ITEM_ntotal - 32).  Host or device per flags; with
 * CRC32C_DEVICE | CRC32C_ASYNC and nbad == NULL the call returns once the
 * kernels are enqueued on `stream` (the caller fences reads of the wbuf on
 * that stream).  ok (optional) marks stamped images;
 * malformed images are left untouched and counted in *nbad.  region_bytes as
 * for crc32c_verify_items.  Images are expected not to overlap (extstore
 * packs them back to back); where one image's span covers another's exptime,
 * its CRC may or may not include that image's new stamp.
 *
 * With CRC32C_KEEP_STAMPED a wbuf may mix fresh images with images carried over
 * verbatim with their stored CRC (compaction, storage.c:1004-1006).  Per image
 * whose header is sane, c = crc32c(0, image + 32, ITEM_ntotal - 32):
 *   exptime == 0 (fresh: the writer leaves it 0): c is written into exptime,
 *                ok[i] = CRC32C_ITEM_STAMPED;
 *   exptime != 0 (carried): nothing is written; ok[i] = CRC32C_ITEM_KEPT when
 *                exptime == c, else ok[i] = 0 and the image counts in *nbad
 *                (count it like badcrc_from_extstore: the image was damaged
 *                before it was copied).
 * Malformed images are untouched, ok[i] = 0, counted, as without the flag.  A
 * carried image whose stored CRC is genuinely 0 is taken for fresh: intact, it
 * is re-stamped with the same 0; corrupt, its damage is covered by a new CRC
 * (probability 2^-32 per corrupt image).  Without the flag nothing changes:
 * every sane image is stamped. */
int crc32c_stamp_items(void *base, uint64_t base_bytes, uint64_t region_bytes,
                       const uint64_t *item_offsets, uint64_t n, uint8_t *ok, uint64_t *nbad,
                       unsigned flags, void *stream);

/* crc32c_stamp_items with the walk done on the device: [base, base_bytes) is
 * walked exactly as crc32c_verify_pages walks it (wbuf_bytes pieces, items
 * packed from each piece's start, nkey == 0 or fewer than 48 bytes left end
 * it; CRC32C_EWALK as there) and every image found is stamped, or with
 * CRC32C_KEEP_STAMPED stamped or verified, as crc32c_stamp_items does with
 * region_bytes = wbuf_bytes.  Host or device per flags; the call returns when
 * the stamps are written (the walk's count is read back, so CRC32C_ASYNC has no
 * effect).  *nitems = images found and *nbad = bad ones, always filled; the
 * first min(cap, *nitems) offsets and ok flags (CRC32C_ITEM_*) are written, in
 * walk order, when cap > 0.  Unlike crc32c_verify_pages' count-only query,
 * cap == 0 still stamps every image: offsets / ok may then be NULL (a caller
 * that wants no per-item output, e.g. extstore's _submit_wbuf).  Images behind
 * a header that stops a piece's walk are neither stamped nor counted.  A wbuf
 * that is still open, its tail not yet zeroed, is passed with base_bytes = the
 * bytes used, so the walk never reads what lies behind them (INTEGRATION.md
 * section 2: the hook runs before the tail memset).  Scratch as for
 * crc32c_verify_pages. */
int crc32c_stamp_pages(void *base, uint64_t base_bytes, uint64_t wbuf_bytes, uint64_t *offsets,
                       uint8_t *ok, uint64_t cap, uint64_t *nitems, uint64_t *nbad, unsigned flags,
                       void *stream);

/* Copy n item images and verify them while they pass: the copy that
 * storage_compact_readback makes of every image it keeps (storage.c:1004-1006,
 * unchecked in the reference), given as the list of images the walk decided to
 * rescue (src_offsets, into [src, src + src_bytes)) and the places
 * extstore_write_request gave them (dst_offsets, into [dst, dst + dst_bytes)).
 * Each image is read once: the 16-byte pieces the CRC folds are the pieces
 * that are stored.
 *   Sanity.  Image i is judged sane exactly as crc32c_verify_items judges it;
 *     src_bytes, region_bytes and CRC32C_CFLAGS64 apply to the source.
 *   A sane image that fits.  With nt = ITEM_ntotal, the bytes
 *     [src + src_offsets[i], + nt) are written to [dst + dst_offsets[i], + nt),
 *     all nt of them, header bytes 0..31 included, and
 *     c = crc32c(0, image + 32, nt - 32) is computed from the same loads:
 *     ok[i] = CRC32C_ITEM_COPIED when c == exptime, else CRC32C_ITEM_DAMAGED.  A
 *     damaged image is still written in full (its verdict is known only after
 *     its last byte has passed).  In dst it keeps its mismatching CRC, so a later
 *     read still counts it (storage.c:160-178), and it is walk-consistent there
 *     (it advances the walk by its own nt); the caller must not relink the item
 *     to it.
 *   An image that is not sane.  Nothing is written, ok[i] = 0, counted bad.
 *   A sane image that does not fit (dst_offsets[i] + nt > dst_bytes).  Nothing is
 *     written, ok[i] = 0, counted bad, and the call returns CRC32C_ERANGE (an
 *     asynchronous call cannot report it, as with crc32c_batch).
 *   *nbad counts every image whose ok is not CRC32C_ITEM_COPIED.
 *   No stray writes.  No byte of dst outside the written images is written, not
 *     even with the value it already holds (neighbouring images are written
 *     concurrently); no byte of src is written.
 *   Placement is the caller's.  The library does not pack; destination images
 *     must not overlap each other; [src, + src_bytes) and [dst, + dst_bytes)
 *     must not overlap (CRC32C_EINVAL when they do); region_bytes is not applied
 *     to dst.
 * Host or device per flags, as for crc32c_stamp_items: with CRC32C_DEVICE src,
 * dst, both offset arrays and ok are device memory, and with CRC32C_DEVICE |
 * CRC32C_ASYNC and nbad == NULL the call returns once the work is enqueued on
 * `stream`.  Host buffers that are both page-locked (crc32c_host_alloc /
 * _register: the readback_buf and the wbufs) are read and written in place by
 * the GPU; otherwise the images are verified on the GPU and copied by the host.
 * NULL src, dst, src_offsets, dst_offsets or ok: CRC32C_EINVAL; n == 0:
 * CRC32C_OK with *nbad = 0; no device: CRC32C_ENODEV, nothing written.  The
 * destination wbuf must not be submitted before the call returns (or, for an
 * asynchronous call, before `stream` has passed it). */
int crc32c_copy_items(const void *src, uint64_t src_bytes, uint64_t region_bytes,
                      const uint64_t *src_offsets, void *dst, uint64_t dst_bytes,
                      const uint64_t *dst_offsets, uint64_t n, uint8_t *ok, uint64_t *nbad,
                      unsigned flags, void *stream);

/* Asynchronous form of crc32c_batch: returns at once with a job handle;
 * crc32c_batch_wait blocks until out[] is filled and frees the handle.
 *
 * Jobs go to the current device's queue.  Host jobs whose buffer is
 * device-visible (crc32c_host_alloc, crc32c_host_register) and whose spans are
 * at most 256 KiB are coalesced: the queue's dispatcher packs every such job
 * pending at that moment (up to 8192 spans) into one kernel launch that reads
 * the spans straight from host memory, while the previous launch runs.  Many
 * IO threads that each submit their few reads (storage.c:172 per io_depth
 * batch) thus share launches; crc32c_batch itself takes this path for such
 * batches.  Other jobs (pageable host memory, long spans, CRC32C_DEVICE
 * batches) run one by one on the dispatcher.  A CRC32C_DEVICE job runs on the
 * queue's own stream after the work the submitting thread had enqueued on its
 * device's default (NULL) stream when it submitted (an event recorded there
 * at submit time): a batch filled by work on another stream must be complete
 * when submitted.  The caller's arrays must stay valid until
 * crc32c_batch_wait returns. */
typedef struct crc32c_job *crc32c_job_t;
int crc32c_batch_submit(const crc32c_spans *spans, unsigned flags, crc32c_job_t *job);
int crc32c_batch_wait(crc32c_job_t job);

/* A batch of byte spans that lie wherever the caller's buffers do: one pointer
 * per span, no common base.  The read path's shape (storage.c:147-178,
 * proxy_internal.c:16-60): slab pages malloc'ed one by one (slabs.c:613-616),
 * the proxy's malloc(ntotal) per read (proxy_internal.c:91), one iov per chunk
 * of a chunked item (storage.c:298-337).
 *   span i = [ptrs[i], + (lens ? lens[i] : len))
 *   out[i] = crc32c(crc_in ? crc_in[i] : 0, span i), bit-identical to the
 *   reference.  Spans may repeat, overlap and come in any order.  A span of no
 *   bytes gives out[i] = crc_in[i] (0 without crc_in); its pointer may be NULL
 *   and is never dereferenced.
 * What is read.  There is no bound to check the spans against, so the contract
 * is what the call reads:
 *   pageable host memory        the span's own bytes [ptrs[i], + len_i), by the
 *                               host, and nothing else;
 *   device and page-locked      the 16-byte granules (addresses that are
 *   memory                      multiples of 16) that the span's bytes touch.
 *                               A granule never crosses a page, so any span
 *                               inside mapped memory is safe.
 * Host batches (no CRC32C_DEVICE).  A NULL pointer with len_i != 0, or a span
 * longer than crc32c_batch's host limit (256 MiB - 16): CRC32C_EINVAL, nothing
 * read, out untouched.  When every span lies in page-locked memory
 * (crc32c_host_alloc, crc32c_host_register, or locked by other means), the
 * spans are at most 256 KiB and the batch is small (at most 8192 spans, and
 * their lengths add up to at most 8 MiB -- or, with lens == NULL, len is at most
 * 1 MiB: buffers that lie far apart do not make a batch large), the GPU reads
 * the spans where they lie, in one launch shared with other threads' jobs (the
 * queue of crc32c_batch_submit).  Any other batch is packed: the host copies
 * each span's bytes, and only those, back to back into the pipeline's pinned
 * slots (each span keeps its address mod 16), while the slot before is
 * checksummed.  A slot whose spans are all page-locked and average 64 KiB or
 * more is filled by one DMA per span instead, without the host copy.
 * Device batches (CRC32C_DEVICE).  ptrs, lens, crc_in and out are device
 * arrays; every ptrs[i] is memory of the current device, from any allocation.
 * A span longer than CRC32C_MAX_SPAN is not read: out[i] = 0 and the call
 * returns CRC32C_ERANGE, as crc32c_batch treats it (lens == NULL with such a
 * len: CRC32C_EINVAL).  Unless the batch is small by n and a fixed len, one
 * pass over ptrs and lens first finds the spans' extent and the sum of their
 * lengths (24 bytes read back, 8 B of grow-only scratch per span), which decide
 * the route as base_bytes decides crc32c_batch's.  With CRC32C_ASYNC the call
 * still returns without waiting for the CRC kernels; it waits for that
 * read-back only.
 * No device: CRC32C_ENODEV, nothing written.  n == 0: CRC32C_OK. */
typedef struct crc32c_ptr_batch {
    const void *const *ptrs;  /* n span starts */
    const uint32_t *lens;     /* n lengths, or NULL: every span is `len` bytes */
    uint32_t len;
    const uint32_t *crc_in;   /* or NULL (0) */
    uint32_t *out;            /* n */
    uint64_t n;
} crc32c_ptr_batch;

typedef struct crc32c_ptr_opts { /* NULL: all zero */
    uint32_t mode;            /* CRC32C_DEVICE | CRC32C_ASYNC; others ignored */
    void *stream;
} crc32c_ptr_opts;

int crc32c_batch_ptrs(const crc32c_ptr_batch *b, const crc32c_ptr_opts *opts);

/* Asynchronous form, as crc32c_batch_submit is crc32c_batch's: wait with
 * crc32c_batch_wait.  The spans are translated when the job is submitted.  A
 * host job whose spans are all page-locked and at most 256 KiB, with at most
 * 8192 of them, shares the queue's launches with every other coalescable job
 * (crc32c_queue_stats counts it among them); any other runs alone on the
 * dispatcher, a CRC32C_DEVICE job behind the submitter's default stream.
 * opts->stream is not used. */
int crc32c_ptrs_submit(const crc32c_ptr_batch *b, const crc32c_ptr_opts *opts, crc32c_job_t *job);

/* crc32c_batch_chains over such iovs: the same fold, the same chain_first
 * rules (a host one that descends or passes iovs->n: CRC32C_EINVAL), iovs->out
 * receives each iov's own CRC, iovs->crc_in must be NULL.  nchains == 0:
 * CRC32C_OK, nothing written. */
int crc32c_chains_ptrs(const crc32c_ptr_batch *iovs, const uint64_t *chain_first, uint64_t nchains,
                       uint32_t *out, const crc32c_ptr_opts *opts);

/* Queue counters of the current device since the first submit: coalesced
 * kernel launches, the spans and jobs they carried, and jobs run alone.  Any
 * pointer may be NULL. */
int crc32c_queue_stats(uint64_t *launches, uint64_t *spans, uint64_t *jobs, uint64_t *solo_jobs);

/* Page-locked host memory for extstore's wbufs (extstore.c:127-140) and the
 * compaction readback_buf (storage.c:1120): host batches over such buffers
 * are copied by one DMA per pipeline slot with no staging copy.  NULL when
 * there is no gfx950 device or the allocation fails; free with
 * crc32c_host_free. */
void *crc32c_host_alloc(size_t bytes);
void crc32c_host_free(void *p);

/* Page-lock and map an existing host range (e.g. the slab arena that read
 * buffers come from, storage.c:264-337) so host batches over it are read by
 * the GPU in place: coalesced by the queue and copied without staging.  The
 * ranges need not be one arena: register each slab page where it is malloc'ed
 * (slabs.c:613-616) and name the buffers by pointer (crc32c_batch_ptrs).  The
 * library records every range it page-locks, so a span's device address is a
 * lookup, not a runtime call. */
int crc32c_host_register(void *p, size_t bytes);
int crc32c_host_unregister(void *p);

/* Tuning, for tests and benchmarks: batches of at most n spans (default 8192,
 * the kernel's limit) take the single-launch small-batch kernel; 0 sends every
 * batch through the planned multi-launch path.  Process-wide; returns the
 * previous value. */
uint64_t crc32c_set_small_max(uint64_t n);

/* Tuning, for tests and benchmarks: batches of equal 4 KiB spans whose waves
 * each run at least `steps` steps (a step: two spans) have their last eighth
 * claimed in chunks by the waves that finish first; shorter ones are split
 * evenly.  UINT64_MAX: never; values below the smallest the split supports
 * (8) count as that.  Process-wide; returns the previous value. */
uint64_t crc32c_set_k1_tail_min(uint64_t steps);

const char *crc32c_strerror(int err);

/* Duration of this thread's last synchronous device batch (milliseconds,
 * hipEvent-measured on its stream); -1 before the first one.  After
 * crc32c_salvage_pages, crc32c_recover_pages and crc32c_triage_pages: the scan's
 * counting pass over the eligible bytes.  After crc32c_repair_items and crc32c_repair_bytes: the search kernel.  After
 * crc32c_repair_headers: the variants' counting pass.  After
 * crc32c_scrub_pages: its last triage's counting pass. */
float crc32c_last_kernel_ms(void);

#ifdef __cplusplus
}
#endif

#endif /* CRC32C_BATCH_H */

"""Buffers and framing for the base-shift tests (no GPU, no library call):
tests/test_gpu_base_shift.py runs every entry point of the library over them
with a `base` that is off the 16-byte grid.

The rule under test.  A buffer B and a shift s are framed in an allocation of
SLACK + s + len(B) + SLACK bytes, every byte FILL (not zero: zeros behind a
span hide a tail that was not cleared), B at [SLACK + s:).  The library gets
the view that starts at SLACK + s and is len(B) bytes long, so its `base` has
the residue of s on every grid the allocator aligned it to.  Every result of
the call must equal the oracle's or the model's result for B and, bit for
bit, the result of the same call at s = 0; a call that writes must leave the
whole allocation, slack included, as the model's bytes framed the same way.

Gaps between spans or images inside B hold random non-zero bytes, except
where a case means zeros (a wbuf's zero tail ends its walk).
"""
import functools

import numpy as np

from memcached_amd import layout

from . import header_cases as hc
from . import header_model as hm
from . import oracle
from . import repair_bytes_cases as bc
from . import repair_cases as rc
from . import salvage_cases as sc

SLACK = 256
FILL = 0xA5
# every kind of residue mod 16, both sides of a 128-byte line, off the 4 KiB block and tile grid
SHIFTS = (1, 7, 8, 15, 16, 17, 120, 127, 129, 4097)
THIN = (1, 8, 15, 129)       # the least a case may be thinned to
HOST_SHIFTS = (1, 15, 129)   # page-locked host buffers at ptr + s


def frame(B, s):
    """The allocation of buffer B at shift s, as a host array."""
    B = np.ascontiguousarray(B, np.uint8)
    a = np.full(SLACK + s + B.size + SLACK, FILL, np.uint8)
    a[SLACK + s:SLACK + s + B.size] = B
    return a


def nonzero_bytes(rng, n):
    return rng.integers(1, 256, n, dtype=np.uint8)


def fill_gaps(buf, offs, lens, rng):
    """Every byte of buf outside the spans (offs[i], lens[i]) becomes a random non-zero byte."""
    covered = np.zeros(buf.size + 1, np.int64)
    np.add.at(covered, np.asarray(offs, np.int64), 1)
    np.add.at(covered, np.asarray(offs, np.int64) + np.asarray(lens, np.int64), -1)
    gap = np.cumsum(covered)[:-1] == 0
    buf[gap] = nonzero_bytes(rng, int(gap.sum()))
    return buf


# ---------------------------------------------------------------------------
# crc32c_batch, offsets[] and lens[]
# ---------------------------------------------------------------------------
def _packed(lengths, rng):
    """Every length once at every start residue mod 16, gaps of 0..40 bytes of
    non-zero bytes in between: (buffer, offsets, lens)."""
    order = rng.permutation(np.repeat(np.asarray(lengths, np.int64), 16))
    want = np.zeros(order.size, np.int64)
    seen = {}
    for i, n in enumerate(order.tolist()):  # the k-th copy of a length starts at residue k
        want[i] = seen.get(n, 0)
        seen[n] = want[i] + 1
    offs, at = np.zeros(order.size, np.int64), 0
    for i, n in enumerate(order.tolist()):
        gap = int(rng.integers(0, 25))
        at += gap + (want[i] - (at + gap)) % 16   # 0..40 bytes
        offs[i] = at
        at += n
    buf = rng.integers(0, 256, at + int(rng.integers(0, 41)), dtype=np.uint8)
    fill_gaps(buf, offs, order, rng)
    assert all(set((offs[order == n] % 16).tolist()) == set(range(16)) for n in (lengths[0], lengths[-1]))
    assert (np.diff(offs) - order[:-1]).max() <= 40 and (np.diff(offs) - order[:-1]).min() >= 0
    return buf, offs.astype(np.uint64), order.astype(np.uint32)


# the lengths of test_fixed_length_head_fragment_thresholds above 1200, and several 64 KiB segments
LONG_LENS = (4080, 4097, 4200, 4209, 4224, 4225, 4240, 5104, 5125, 8195, 65536, 65552, 70001, 131073, 200003)


@functools.lru_cache(maxsize=None)
def batch_parts():
    """crc32c_batch with lens[]: every length 0..1200 (across kWholeMax = 1024,
    kFragMax = 128 and the 128-byte grid pad) at every start residue mod 16,
    in three buffers of at most 8192 spans and 8 MiB each (the bounds of the
    single-launch route), and the long lengths, two residues each, in a
    fourth.  Per part: (buffer, offsets, lens, crc_in, want, want with crc_in,
    a shuffle)."""
    rng = np.random.default_rng(1601)
    parts = [_packed(list(range(lo, hi)), rng) for lo, hi in ((0, 401), (401, 801), (801, 1201))]
    lens = np.repeat(np.array(LONG_LENS, np.int64), 2)
    gaps = rng.integers(0, 41, lens.size)
    offs = np.cumsum(gaps + np.concatenate([[0], lens[:-1]]))
    buf = rng.integers(0, 256, int(offs[-1] + lens[-1] + 33), dtype=np.uint8)
    fill_gaps(buf, offs, lens, rng)
    parts.append((buf, offs.astype(np.uint64), lens.astype(np.uint32)))
    out = []
    for buf, offs, lens in parts:
        assert offs.size <= 8192 and buf.size <= 8 << 20
        cin = rng.integers(0, 2**32, offs.size, dtype=np.uint64).astype(np.uint32)
        buf.flags.writeable = False
        out.append((buf, offs, lens, cin, oracle.batch(buf, offs, lens), oracle.batch(buf, offs, lens, cin),
                    rng.permutation(offs.size)))
    return out


# (0: no span kernel runs and k_final must not take the caller's out[] for a kernel's result)
# (257..513: across kWholeMax = 512.  len + 127 <= 512 is k_final alone, and from 386 to 512 a span is its
# thread's or the span kernel's by its own alignment: one batch holds both)
SHARED_LENS = (0, 1, 100, 257, 384, 385, 386, 400, 448, 511, 512, 513, 1009, 1024, 4133, 4225, 8195)


@functools.lru_cache(maxsize=None)
def shared_len_case(L, n=700):
    """offsets[] with one shared length (k_spans<false> and its neighbours):
    n sorted random offsets, as test_fixed_length_head_fragment_thresholds."""
    rng = np.random.default_rng(1700 + L)
    size = n * (L + 40) + 64
    buf = rng.integers(1, 256, size, dtype=np.uint8)
    offs = np.sort(rng.integers(0, size - L, n)).astype(np.uint64)
    cin = rng.integers(0, 2**32, n, dtype=np.uint64).astype(np.uint32)
    return buf, offs, cin, oracle.batch(buf, offs, np.full(n, L)), oracle.batch(buf, offs, np.full(n, L), cin)


@functools.lru_cache(maxsize=None)
def stride_case(stride, n=33, L=4096):
    rng = np.random.default_rng(1800 + stride)
    buf = rng.integers(1, 256, (n - 1) * stride + L, dtype=np.uint8)
    offs = np.arange(n, dtype=np.uint64) * np.uint64(stride)
    cin = rng.integers(0, 2**32, n, dtype=np.uint64).astype(np.uint32)
    return buf, cin, oracle.batch(buf, offs, np.full(n, L)), oracle.batch(buf, offs, np.full(n, L), cin)


# ---------------------------------------------------------------------------
# item images: verify_items / stamp_items / the page calls
# ---------------------------------------------------------------------------
WBUF = 1 << 20


def _item_set(items, wbuf, rng, carried_every=0):
    """(buffer with every image's exptime 0, the same with the CRCs stored,
    offsets): packed wbufs.  carried_every k: in the first buffer every k-th
    image carries its CRC already (CRC32C_KEEP_STAMPED verifies those)."""
    fresh, offs = layout.pack_wbufs(items, wbuf)
    soffs, slens = layout.spans_of(fresh, offs)
    crcs = oracle.batch(fresh, soffs, slens)
    assert (crcs != 0).all()
    stamped = fresh.copy()
    layout.store_crcs(stamped, offs, crcs)
    if carried_every:
        layout.store_crcs(fresh, offs[::carried_every], crcs[::carried_every])
    return fresh, stamped, offs


def _damage(buf, offs, data_at, nbytes_at, rng):
    """One data-damaged image and one with a flipped nbytes bit (a set bit of
    its low 16: the image gets shorter, so a stamp of it still overlaps no
    other image's exptime)."""
    o = int(offs[data_at])
    buf[o + 48 + int(rng.integers(0, layout.ntotal_of(buf, o) - 48))] ^= 1 << int(rng.integers(0, 8))
    o = int(offs[nbytes_at])
    low = int(buf[o + 32]) | int(buf[o + 33]) << 8
    bit = low.bit_length() - 1
    assert bit >= 0
    buf[o + 32 + bit // 8] ^= 1 << (bit % 8)


@functools.lru_cache(maxsize=None)
def item_set(name):
    """name -> (fresh, stamped, offsets, wbuf): `fresh` for the stamp calls
    (every second image carries its CRC, one of those data-damaged), `stamped`
    for the verify calls; one data-damaged image and one flipped nbytes bit in
    each."""
    rng = np.random.default_rng({"mixed": 37, "k5": 38, "long": 39}[name])
    if name == "mixed":    # test_stamp_items' shape: images of 52 B .. 9 KB
        items = [layout.make_item(b"st%06d" % i, rng.integers(0, 256, int(rng.integers(0, 9000)), dtype=np.uint8).tobytes(),
                                  cas=i + 1) for i in range(900)]
        items[5] = sc.image_nt(rng, 52)
        for k in (28, 29, 30, 31):
            items[5][k] = 0
    elif name == "k5":     # 4165-byte images: K5's and k_blocks' shape
        items = [layout.make_item(b"k5%06d" % i, rng.integers(0, 256, 4098, dtype=np.uint8).tobytes(), cas=i + 1)
                 for i in range(300)]
        assert len(items[0]) == 4165
    else:                  # several 64 KiB segments each
        items = [layout.make_item(b"lg%05d" % i, rng.integers(0, 256, int(rng.integers(65000, 300000)),
                                                              dtype=np.uint8).tobytes(), cas=i + 1) for i in range(10)]
    fresh, stamped, offs = _item_set(items, WBUF, rng, carried_every=2)
    n = offs.size
    _damage(fresh, offs, 2 * (n // 6), 2 * (n // 3) + 1, rng)   # (a carried image's data, a fresh image's nbytes)
    _damage(stamped, offs, n // 5, n // 2, rng)
    for b in (fresh, stamped, offs):
        b.flags.writeable = False
    return fresh, stamped, offs, WBUF


def walk(buf, wbuf):
    """storage_compact_readback's walk (storage.c:950-1070), one read per wbuf-sized piece from the buffer's start."""
    offs = []
    for start in range(0, buf.size, wbuf):
        size, off = min(wbuf, buf.size - start), 0
        while off + 48 <= size and buf[start + off + 41] != 0:
            offs.append(start + off)
            off += layout.ntotal_of(buf, start + off) & 0xffffffff
    return np.asarray(offs, np.uint64)


@functools.lru_cache(maxsize=None)
def page_set(name):
    """name -> (fresh, stamped, offsets, wbuf) for verify_pages / stamp_pages.
    runs_*: test_verify_pages_walk_wave_runs' runs of 63, 64 and 65 equal items
    (and its others) at two of its wbuf sizes; slots: test_verify_pages_slot_boundary's
    wbufs of 31, 32, 33, 0, 1, 32 and 33 items."""
    rng = np.random.default_rng(44)
    if name.startswith("runs"):
        sizes = []
        for run in (63, 64, 65, 1, 128, 129, 127, 2, 300, 64, 64, 5):
            sizes += [int(rng.choice([0, 3, 100, 4096]))] * run
        items = [layout.make_item(b"v%06d" % i, rng.integers(0, 256, n, dtype=np.uint8).tobytes(), cas=i + 1)
                 for i, n in enumerate(sizes)]
        wbuf = {"runs_1m": 1 << 20, "runs_odd": 4165 * 64 + 47}[name]
        fresh, stamped, offs = _item_set(items, wbuf, rng, carried_every=2)
    else:
        wbuf = 64 << 10
        parts = []
        for w, n in enumerate([31, 32, 33, 0, 1, 32, 33]):
            items = [layout.make_item(b"s%02d%05d" % (w, i), rng.integers(0, 256, 1800, dtype=np.uint8).tobytes(),
                                      cas=w * 100 + i + 1) for i in range(n)]
            parts.append(_item_set(items, wbuf, rng, carried_every=2) if items else
                         (np.zeros(wbuf, np.uint8), np.zeros(wbuf, np.uint8), np.zeros(0, np.uint64)))
            assert parts[-1][0].size == wbuf
        fresh, stamped = (np.concatenate([p[k] for p in parts]) for k in (0, 1))
        offs = np.concatenate([p[2] + np.uint64(w * wbuf) for w, p in enumerate(parts)])
    n = offs.size
    carried = [i for i in range(n) if fresh[int(offs[i]) + 28:int(offs[i]) + 32].any()]
    # (data damage only: a flipped length bit would turn the walk, which the salvage family's pages cover)
    for buf, at in ((fresh, (carried[len(carried) // 3], carried[-1])), (stamped, (n // 5, n // 2, n - 1))):
        for i in at:
            buf[int(offs[i]) + 50] ^= 0x10
        assert np.array_equal(walk(buf, wbuf), offs)
    for b in (fresh, stamped, offs):
        b.flags.writeable = False
    return fresh, stamped, offs, wbuf


# ---------------------------------------------------------------------------
# the repair calls: the 52-byte-image fixtures of their own tests, one alignment set each
# ---------------------------------------------------------------------------
def _regions(buf, offs, nt, rng):
    """Non-zero bytes between the nt-byte images of a one-image-per-region fixture."""
    return fill_gaps(buf, offs, np.full(len(offs), nt), rng)


@functools.lru_cache(maxsize=None)
def repair_items_case():
    """Every bit 224..415 of a 52-byte image inverted, one copy per 128-byte
    region (test_every_position_of_a_52_byte_image_at_every_alignment, the
    copies at region offset 5): (buffer, offsets, region)."""
    rng = np.random.default_rng(1)
    img = sc.image_nt(rng, 52)
    bits = list(range(224, 416))
    buf = np.zeros(len(bits) * 128, np.uint8)
    offs = [j * 128 + 5 for j in range(len(bits))]
    for o, k in zip(offs, bits):
        buf[o:o + 52] = np.frombuffer(bytes(img), np.uint8)
        rc.flip(buf, o, k)
    return _regions(buf, offs, 52, rng), np.array(offs, np.uint64), 128


@functools.lru_cache(maxsize=None)
def repair_bytes_case(p=36):
    """Byte p of a 52-byte image XORed with each of the 255 masks
    (test_all_255_masks_at_eight_alignments, the copies at region offset 3)."""
    rng = np.random.default_rng(p)
    img = sc.image_nt(rng, 52)
    buf = np.zeros(255 * 64 + 64, np.uint8)
    offs = [(m - 1) * 64 + 3 for m in range(1, 256)]
    for o, m in zip(offs, range(1, 256)):
        buf[o:o + 52] = np.frombuffer(bytes(img), np.uint8)
        bc.xor_byte(buf, o, p, m)
    return _regions(buf, offs, 52, rng), np.array(offs, np.uint64), 0


@functools.lru_cache(maxsize=None)
def repair_headers_case():
    """Each of the 42 length bits of a 52-byte image inverted, one copy per
    128-byte region (test_every_bit_of_a_52_byte_image_at_every_alignment, two
    alignments)."""
    rng = np.random.default_rng(5)
    img = sc.image_nt(rng, 52)
    buf, offs, bits, pristine = hc.per_region(img, hm.BITS, aligns=2)
    return _regions(buf, offs, 52, rng), offs, 128


@functools.lru_cache(maxsize=None)
def repair_mixed_case():
    """repair_cases.mixed(rng, 2000, 3000): packed back to back (no gaps)."""
    buf, offs, kinds = rc.mixed(np.random.default_rng(20), 2000, 3000)
    return buf, offs, 3000

"""Python face of the drop-in library, mirroring the reference interface.

Scalar calls follow crc32c.h (reference crc32c.h:15-21): ``crc32c(crc, buf)``
continues a CRC-32C over ``buf`` (first call with crc = 0, chaining allowed)
and ``crc32c_sw`` is the table-driven variant.  Batch calls wrap
include/crc32c_batch.h and run the gfx950 kernels:

* ``batch``        out[i] = crc32c(crc_in[i] or 0, span i)  (storage.c:567, :172)
* ``verify_items`` stored-CRC check of packed item images (storage.c:160-178)
* ``stamp_items``  spill CRC written into each image's exptime (storage.c:567)
* ``stamp_pages``  walk + stamp whole wbufs on the device (no offset list)
* ``copy_items``   compaction's rescue copy, verified while it copies (storage.c:1004-1006)
* ``verify_pages`` walk + verify whole pages on the device (storage.c:950-1070)
* ``salvage_pages`` the intact images behind a header that ended a wbuf's walk
* ``recover_pages`` verify_pages + salvage_pages in one call, one merged list
* ``triage_pages`` recover_pages plus the unreached candidates whose stored CRC fails (kind 6), for repair_items
* ``repair_items`` single-bit damage of item images located by the stored CRC and flipped back
  (``locate_bit``: the same search for one span on the host)
* ``repair_bytes`` damage confined to one byte (any of its 255 masks) located by the stored CRC and put back, on 32
  times weaker evidence than repair_items' (``locate_byte``: the same search for one span on the host)
* ``repair_headers`` a flipped length bit of an item header found among the 42 headers one bit away
* ``scrub_pages`` triage_pages, repair_headers and repair_items round by round in one call: the final list and a flip log
* ``batch_chains`` chained CRCs of chunked items over iov lists (storage.c:163-170)
* ``batch_multi``  host batch split across GPUs by bytes

Host inputs are numpy arrays (or bytes); device inputs are torch tensors on a
HIP device, enqueued on ``stream`` or else on torch's current stream of that
device.  Each batch wrapper chooses its side once from the buffer (_side) and
then reads: marshal, call, check, slice.
"""
from __future__ import annotations

import ctypes
import operator

import numpy as np

from . import _lib
from ._lib import (CRC32C_ASYNC, CRC32C_CFLAGS64, CRC32C_DEVICE, CRC32C_KEEP_STAMPED, CRC32C_SCRUB_BY_BYTE,
                   CRC32C_SCRUB_BYTES, CRC32C_SCRUB_GAPS, Crc32cError, check, lib)

# (recover_pages, triage_pages, repair_items, locate_bit, repair_headers, scrub_pages, repair_bytes, locate_byte,
# batch_ptrs and chains_ptrs are public as well; tests/test_python_face.py pins this list as it stood before them)
__all__ = ["crc32c", "crc32c_sw", "batch", "verify_items", "stamp_items", "stamp_pages", "verify_pages", "batch_chains",
           "copy_items", "salvage_pages",
           "batch_multi",
           "shard_cuts", "queue_stats", "set_small_max", "set_k1_tail_min", "gpu_count", "Crc32cError"]


def _host_buf(data):
    if isinstance(data, (bytes, bytearray, memoryview)):
        arr = np.frombuffer(data, dtype=np.uint8)
    else:
        arr = np.ascontiguousarray(data).view(np.uint8).reshape(-1)
    return arr


def crc32c(crc: int, data) -> int:
    """crc32c(crc, buf, len) through the `crc32c` function-pointer symbol."""
    arr = _host_buf(data)
    return int(_lib.scalar_crc32c()(crc & 0xFFFFFFFF, arr.ctypes.data, arr.size))


def crc32c_sw(crc: int, data) -> int:
    arr = _host_buf(data)
    return int(lib.crc32c_sw(crc & 0xFFFFFFFF, arr.ctypes.data, arr.size))


def gpu_count() -> int:
    return int(lib.crc32c_gpu_count())


def _is_torch(x) -> bool:
    return type(x).__module__.startswith("torch")


def _is_dev(x) -> bool:
    return _is_torch(x) and x.is_cuda


def _ptr(x):
    if x is None:
        return None
    if _is_torch(x):
        return x.data_ptr()
    return x.ctypes.data


def _count(x) -> int:
    return x.numel() if _is_torch(x) else x.size


# Element kinds of the descriptor and result arrays: (numpy dtype on the host,
# dtype names a device tensor may have -- a new one gets the first).
_U8 = (np.uint8, ("uint8",))
_U32 = (np.uint32, ("int32", "uint32"))
_U64 = (np.uint64, ("int64", "uint64"))
_WRITABLE = "a writable contiguous uint8 numpy array"


class _Host:
    """The host side of a call: numpy arrays, no flag, no stream."""
    dev, flag, stream = False, 0, None

    def buffer(self, buf, name="buf", inplace=None):
        """(array, bytes) of a data buffer.  ``inplace``: the call writes it,
        so nothing is converted; the text of the refusal, {} = _WRITABLE."""
        if not inplace:
            buf = _host_buf(buf)
        elif not (isinstance(buf, np.ndarray) and buf.dtype == np.uint8 and buf.flags.writeable
                  and buf.flags.c_contiguous):
            raise TypeError(inplace.format(_WRITABLE))
        return buf, buf.size

    def desc(self, a, name, kind, n=0, exact=False):
        """A descriptor array the library reads n elements of, converted to
        its width (None stays None).  ``exact``: a longer one is refused too."""
        if a is None:
            return None
        a = np.ascontiguousarray(a, dtype=kind[0])
        if a.size < n or (exact and a.size != n):
            raise ValueError(f"{name}: {a.size} elements for {n} spans")
        return a

    def out(self, a, name, kind, n):
        """The caller's result array, checked and never converted, or a new one."""
        if a is None:
            return self.empty(n, kind)
        if a.size < n:
            raise ValueError(f"{name}: {a.size} elements for {n} spans")
        if a.dtype.name not in kind[1] or not a.flags.c_contiguous:
            raise TypeError(f"{name}: need a contiguous {kind[0].__name__} array")
        return a

    def empty(self, n, kind):
        return np.empty(n, kind[0])


class _Device:
    """The device side: torch tensors of the buffer's device, CRC32C_DEVICE,
    the caller's stream or else torch's current stream of that device."""
    dev, flag = True, CRC32C_DEVICE

    def __init__(self, buf, stream):
        import torch
        self.torch, self.device = torch, buf.device
        self.stream = torch.cuda.current_stream(buf.device).cuda_stream if stream is None else stream

    def buffer(self, buf, name="buf", inplace=None):
        if not buf.is_contiguous():
            raise ValueError(f"{name}: need a contiguous device tensor")
        return buf, buf.numel() * buf.element_size()

    def desc(self, t, name, kind, n=0, exact=False):
        """Contiguous, on the device, one of the kind's dtypes, at least n
        elements (the kernels read n of them unchecked; a longer tensor is
        never refused here, ``exact`` is the host's)."""
        if t is None:
            return None
        if not (_is_dev(t) and t.is_contiguous()):
            raise ValueError(f"{name}: device batches need a contiguous device tensor")
        if str(t.dtype).replace("torch.", "") not in kind[1]:
            raise TypeError(f"{name}: dtype {t.dtype} (need one of {', '.join(kind[1])})")
        if t.numel() < n:
            raise ValueError(f"{name}: {t.numel()} elements for {n} spans")
        return t

    def out(self, t, name, kind, n):
        return self.empty(n, kind) if t is None else self.desc(t, name, kind, n)

    def empty(self, n, kind):
        return self.torch.empty(n, dtype=getattr(self.torch, kind[1][0]), device=self.device)


_HOST = _Host()


def _side(buf, stream=None):
    """Where a call's data lives, chosen from its buffer."""
    return _Device(buf, stream) if _is_dev(buf) else _HOST


def _flags(cflags64, keep_stamped=False):
    return (CRC32C_CFLAGS64 if cflags64 else 0) | (CRC32C_KEEP_STAMPED if keep_stamped else 0)


def _wbuf_bytes(wbuf_bytes) -> int:
    try:
        wbuf_bytes = operator.index(wbuf_bytes)
    except TypeError:
        wbuf_bytes = 0
    if wbuf_bytes <= 0:
        raise ValueError("wbuf_bytes: need a positive integer")
    return wbuf_bytes


def _check_carrying(rc, what, carrier, **attrs):
    """check(), but status ``carrier`` comes with partial results: they travel
    as attributes of the error."""
    if rc == carrier:
        err = Crc32cError(rc, what)
        vars(err).update(attrs)
        raise err
    check(rc, what)


def _sized(side, kinds, cap, call, proven=False):
    """Result arrays of the count that ``call(cap, *pointers)`` returns: one
    call when the results fit ``cap``, else a second one with the exact count.
    ``proven``: cap is an upper bound, more is a bug."""
    while True:
        arrays = [side.empty(cap, kind) for kind in kinds]
        n = call(cap, *map(_ptr, arrays))
        if n <= cap:
            return [a[:n] for a in arrays]
        assert not proven, "item count above the proven bound"
        cap = n


def _spans(side, buf, offsets, stride, lens, length, crc_in, out):
    """(crc32c_spans, out) of a batch."""
    if offsets is not None:
        n = len(offsets)
    elif lens is not None:
        n = len(lens)
    else:
        raise ValueError("need offsets or lens to know the batch size")
    buf, nbytes = side.buffer(buf)
    offsets = side.desc(offsets, "offsets", _U64, n)
    lens = side.desc(lens, "lens", _U32, n)
    crc_in = side.desc(crc_in, "crc_in", _U32, n)
    out = side.out(out, "out", _U32, n)
    s = _lib.Spans(_ptr(buf), nbytes, _ptr(offsets), stride, _ptr(lens), length, _ptr(crc_in), _ptr(out), n)
    s.arrays = buf, offsets, lens, crc_in  # the struct holds bare addresses: converted copies live as long as it does
    return s, out


def batch(buf, offsets=None, stride: int = 0, lens=None, length: int = 0, crc_in=None, out=None,
          stream=None, asynchronous: bool = False, aligned16=None):
    """Batched CRC-32C of spans of ``buf``.

    Span i = buf[off_i : off_i + len_i] with off_i = offsets[i] (or i*stride)
    and len_i = lens[i] (or ``length``).  Host numpy inputs take the pinned
    staging path; torch device tensors run in place on the current stream.
    Returns ``out`` (uint32, one CRC per span).  ``aligned16`` is accepted and
    ignored, as the C ABI ignores its retired flag bit 0x4 (the kernels test
    alignment themselves).
    """
    if aligned16 is not None:
        import warnings
        warnings.warn("batch(aligned16=...) is ignored (alignment is detected per batch)", DeprecationWarning,
                      stacklevel=2)
    side = _side(buf, stream)
    s, out = _spans(side, buf, offsets, stride, lens, length, crc_in, out)
    flags = side.flag | (CRC32C_ASYNC if side.dev and asynchronous else 0)
    check(lib.crc32c_batch(ctypes.byref(s), flags, side.stream), "crc32c_batch")
    return out


def batch_multi(buf, offsets=None, stride: int = 0, lens=None, length: int = 0, crc_in=None, ngpus: int = 0):
    """Host batch split across ``ngpus`` devices (0 = all) by bytes."""
    s, out = _spans(_HOST, buf, offsets, stride, lens, length, crc_in, None)
    check(lib.crc32c_batch_multi(ctypes.byref(s), ngpus), "crc32c_batch_multi")
    return out


def _items(what, buf, item_offsets, region_bytes, stream, flags, inplace=None):
    """crc32c_verify_items / crc32c_stamp_items: (ok, nbad)."""
    side = _side(buf, stream)
    buf, nbytes = side.buffer(buf, inplace=inplace)
    offs = side.desc(item_offsets, "item_offsets", _U64)
    n = _count(offs)
    ok = side.empty(n, _U8)
    nbad = ctypes.c_uint64(0)
    check(getattr(lib, what)(_ptr(buf), nbytes, region_bytes, _ptr(offs), n, _ptr(ok), ctypes.byref(nbad),
                             side.flag | flags, side.stream), what)
    return ok, int(nbad.value)


def verify_items(buf, item_offsets, region_bytes=0, stream=None, cflags64=False):
    """Verify packed item images; returns (ok uint8 array / tensor, nbad).

    ``region_bytes``: the write-buffer size; an item whose header claims a
    span crossing a multiple of it is reported bad without being read
    (extstore never splits an item across wbufs).  0 = no such bound.
    ``cflags64``: images of a LARGE_CLIENT_FLAGS build (8-byte client flags)."""
    return _items("crc32c_verify_items", buf, item_offsets, region_bytes, stream, _flags(cflags64))


def stamp_items(buf, item_offsets, region_bytes=0, stream=None, cflags64=False, keep_stamped=False):
    """Write the spill CRC of every item image into its exptime field, in place
    (storage.c:567 for a whole wbuf at once).  Returns (ok, nbad): ok marks
    stamped images (1), nbad counts malformed ones (left untouched).

    ``keep_stamped`` (CRC32C_KEEP_STAMPED): an image whose exptime is not 0
    carries its CRC already (compaction copies images with it); it is verified
    against that value and never written: ok = 2 when it matches, else 0 and
    counted in nbad."""
    return _items("crc32c_stamp_items", buf, item_offsets, region_bytes, stream, _flags(cflags64, keep_stamped),
                  inplace="stamp_items needs {} (stamped in place)")


def copy_items(src, src_offsets, dst, dst_offsets, region_bytes=0, stream=None, cflags64=False):
    """Copy the item images at ``src_offsets`` of ``src`` to ``dst_offsets`` of
    ``dst`` and verify them from the same loads (compaction's rescue copy,
    storage.c:1004-1006, checked).  Returns (ok, nbad): ok[i] is 1 for an image
    written whose stored CRC matches, 3 for one written verbatim whose stored
    CRC does not match, 0 when nothing was written (a malformed image, or one
    that does not fit ``dst``: the call then raises Crc32cError(CRC32C_ERANGE)
    after the other images are copied, with ok and nbad as attributes of the
    error); nbad counts every ok that is not 1.

    ``src`` and ``dst`` are both torch device tensors (the call runs on the
    current stream) or both host buffers, ``dst`` a writable contiguous uint8
    numpy array; ``region_bytes`` and ``cflags64`` apply to the source, as for
    verify_items."""
    side = _side(src, stream)
    if side.dev != _is_dev(dst):
        raise ValueError("copy_items: src and dst must both be device tensors or both be host buffers")
    dst, dst_bytes = side.buffer(dst, "dst", inplace="copy_items needs {} as dst (written in place)")
    src, src_bytes = side.buffer(src, "src")
    soffs = side.desc(src_offsets, "src_offsets", _U64)
    n = _count(soffs)
    doffs = side.desc(dst_offsets, "dst_offsets", _U64, n, exact=True)
    ok = side.empty(n, _U8)
    nbad = ctypes.c_uint64(0)
    rc = lib.crc32c_copy_items(_ptr(src), src_bytes, region_bytes, _ptr(soffs), _ptr(dst), dst_bytes, _ptr(doffs), n,
                               _ptr(ok), ctypes.byref(nbad), side.flag | _flags(cflags64), side.stream)
    # everything that fits is copied: the verdicts travel with the error
    _check_carrying(rc, "crc32c_copy_items", _lib.CRC32C_ERANGE, ok=ok, nbad=int(nbad.value))
    return ok, int(nbad.value)


def _walk_bound(nbytes, wbuf_bytes):
    """No walk counts more: an image is >= 50 bytes and each wbuf's last
    counted image may run past its end."""
    return nbytes // 50 + -(-nbytes // wbuf_bytes)


def _pages(what, side, buf, nbytes, wbuf_bytes, flags, cap, proven):
    """crc32c_verify_pages / crc32c_stamp_pages with result arrays of ``cap``
    items (_sized): (item offsets, ok flags, nbad) in walk order.  ``cap``
    None: the count-only query, no arrays; returns the walk's item count."""
    nitems, nbad = ctypes.c_uint64(0), ctypes.c_uint64(0)

    def walk(cap, offs, ok):
        check(getattr(lib, what)(_ptr(buf), nbytes, wbuf_bytes, offs, ok, cap, ctypes.byref(nitems),
                                 ctypes.byref(nbad), side.flag | flags, side.stream), what)
        return nitems.value

    if cap is None:  # count only
        return walk(0, None, None)
    offs, ok = _sized(side, (_U64, _U8), cap, walk, proven)
    return offs, ok, int(nbad.value)


def stamp_pages(buf, wbuf_bytes, keep_stamped=False, stream=None, cflags64=False):
    """Walk every wbuf-sized piece of ``buf`` on the device, as verify_pages
    does, and stamp each item image found, in place (``keep_stamped`` as for
    stamp_items).  Returns (item offsets, ok flags, nbad) in walk order.

    An open wbuf whose tail is not zeroed yet is passed as a slice of the
    bytes used.  Device buffers are walked once more beforehand (a count-only
    crc32c_verify_pages query) to size the result tensors exactly."""
    wbuf_bytes = _wbuf_bytes(wbuf_bytes)
    side = _side(buf, stream)
    buf, nbytes = side.buffer(buf, inplace="stamp_pages needs {} (stamped in place)")
    args = side, buf, nbytes, wbuf_bytes, _flags(cflags64, keep_stamped)
    cap = _pages("crc32c_verify_pages", *args, None, False) if side.dev else _walk_bound(nbytes, wbuf_bytes)
    return _pages("crc32c_stamp_pages", *args, cap, True)


def verify_pages(buf, wbuf_bytes, stream=None, cflags64=False):
    """Walk every wbuf-sized read of ``buf`` on the device and verify each
    item found.  Returns (item offsets, ok flags, nbad) in walk order.

    Device buffers take one library call when the items fit a first guess of
    the capacity (images of >= 1 KiB on average), otherwise a second call with
    the exact count the first one reported.  A host call stages the whole
    buffer, so there the capacity is the walk's upper bound at once."""
    wbuf_bytes = _wbuf_bytes(wbuf_bytes)
    side = _side(buf, stream)
    buf, nbytes = side.buffer(buf)
    cap = _walk_bound(nbytes, wbuf_bytes)
    if side.dev:
        cap = min(nbytes // 1024 + -(-nbytes // wbuf_bytes), cap)
    return _pages("crc32c_verify_pages", side, buf, nbytes, wbuf_bytes, _flags(cflags64), cap, not side.dev)


def salvage_pages(buf, wbuf_bytes, walked=None, walked_ok=None, stream=None, cflags64=False):
    """The intact images of ``buf`` that the page walk did not reach
    (crc32c_salvage_pages): every offset outside the walk's good images is
    tried as an image start, and those whose stored CRC matches are returned.

    ``walked`` / ``walked_ok``: the offsets and flags verify_pages returned for
    the same buffer (None: nothing is covered, every intact image is found
    from scratch).  Returns (offsets, {"scanned": eligible offsets, "ncand":
    those with a sane header and a CRLF}) for numpy and torch buffers, like
    verify_pages.  When the candidates' spans exceed the work bound the call
    raises Crc32cError(CRC32C_EWORK) with ``scanned`` and ``ncand`` as
    attributes of the error."""
    wbuf_bytes = _wbuf_bytes(wbuf_bytes)
    if (walked is None) != (walked_ok is None):
        raise ValueError("walked and walked_ok go together")
    side = _side(buf, stream)
    buf, nbytes = side.buffer(buf)
    nwalked = 0 if walked is None else len(walked)
    if not nwalked:
        walked = walked_ok = None
    walked = side.desc(walked, "walked", _U64, nwalked)
    walked_ok = side.desc(walked_ok, "walked_ok", _U8, nwalked, exact=True)
    nfound, scanned, ncand = ctypes.c_uint64(0), ctypes.c_uint64(0), ctypes.c_uint64(0)

    def scan(cap, offs):
        rc = lib.crc32c_salvage_pages(_ptr(buf), nbytes, wbuf_bytes, _ptr(walked), _ptr(walked_ok), nwalked, offs, cap,
                                      ctypes.byref(nfound), ctypes.byref(scanned), ctypes.byref(ncand),
                                      side.flag | _flags(cflags64), side.stream)
        _check_carrying(rc, "crc32c_salvage_pages", _lib.CRC32C_EWORK, scanned=int(scanned.value),
                        ncand=int(ncand.value))
        return nfound.value

    # a first guess of the capacity: the images behind the damage of one wbuf in a hundred, 1 KiB each
    offs, = _sized(side, (_U64,), nbytes // (100 * 1024) + 64, scan)
    return offs, {"scanned": int(scanned.value), "ncand": int(ncand.value)}


def recover_pages(buf, wbuf_bytes, stream=None, cflags64=False):
    """The whole read-back of a page in one call (crc32c_recover_pages):
    verify_pages' walk, salvage_pages over its lists and the two results
    merged, with the buffer staged once and the lists kept on the device.

    Returns (offsets, lens, kind, info), ascending by offset, for numpy and
    torch buffers like verify_pages: kind is the walk's verdict (0 or 1) or
    CRC32C_ITEM_SALVAGED (4) for an image the salvage found, lens the image's
    ITEM_ntotal (0 when its header is not sane), info = {"nbad": the walk's bad
    images, "nsalvaged", "scanned", "ncand"}.  When the candidates' spans exceed
    the work bound the call raises Crc32cError(CRC32C_EWORK) with the walk's
    part (``offsets``, ``lens``, ``kind``) and the counts as attributes of the
    error."""
    wbuf_bytes = _wbuf_bytes(wbuf_bytes)
    side = _side(buf, stream)
    buf, nbytes = side.buffer(buf)
    counts = [ctypes.c_uint64(0) for _ in range(5)]  # nitems, nbad, nsalvaged, scanned, ncand
    status = []

    def run(cap, offs, lens, kind):
        rc = lib.crc32c_recover_pages(_ptr(buf), nbytes, wbuf_bytes, offs, lens, kind, cap,
                                      *map(ctypes.byref, counts), side.flag | _flags(cflags64), side.stream)
        if rc != _lib.CRC32C_EWORK:  # (that one comes with the walk's part: raised below, with it)
            check(rc, "crc32c_recover_pages")
        status[:] = [rc]
        return counts[0].value

    # a host call stages the whole buffer, so there the capacity is an upper bound at once (the walk's, and
    # disjoint images of 50 bytes or more); a device call guesses as verify_pages and salvage_pages do
    cap = _walk_bound(nbytes, wbuf_bytes)
    if side.dev:
        cap = min(nbytes // 1024 + -(-nbytes // wbuf_bytes), cap) + nbytes // (100 * 1024) + 64
    else:
        cap += nbytes // 50
    offs, lens, kind = _sized(side, (_U64, _U32, _U8), cap, run)
    info = dict(zip(("nbad", "nsalvaged", "scanned", "ncand"), (int(c.value) for c in counts[1:])))
    _check_carrying(status[0], "crc32c_recover_pages", _lib.CRC32C_EWORK, offsets=offs, lens=lens, kind=kind, **info)
    return offs, lens, kind, info


def triage_pages(buf, wbuf_bytes, stream=None, cflags64=False):
    """recover_pages with the damaged images the walk never reaches listed too
    (crc32c_triage_pages): an unreached candidate (sane header, CRLF at its
    end) whose stored CRC does not match comes back as kind
    CRC32C_ITEM_SUSPECT (6), with its ITEM_ntotal in lens, so that
    repair_items can be handed it.

    Returns (offsets, lens, kind, info) as recover_pages does, info with
    ``"nsuspect"`` beside recover_pages' counts; with the kind-6 entries taken
    out the result is recover_pages'.  Past the work bound the call raises
    Crc32cError(CRC32C_EWORK) with the walk's part and the counts (nsuspect 0)
    as attributes of the error."""
    wbuf_bytes = _wbuf_bytes(wbuf_bytes)
    side = _side(buf, stream)
    buf, nbytes = side.buffer(buf)
    counts = [ctypes.c_uint64(0) for _ in range(6)]  # nitems, nbad, nsalvaged, nsuspect, scanned, ncand
    status = []

    def run(cap, offs, lens, kind):
        rc = lib.crc32c_triage_pages(_ptr(buf), nbytes, wbuf_bytes, offs, lens, kind, cap,
                                     *map(ctypes.byref, counts), side.flag | _flags(cflags64), side.stream)
        if rc != _lib.CRC32C_EWORK:  # (that one comes with the walk's part: raised below, with it)
            check(rc, "crc32c_triage_pages")
        status[:] = [rc]
        return counts[0].value

    # the capacity as recover_pages guesses it (a host call's bound holds for the walk's and the found entries
    # alone: suspects may overlap, so a second call sized from nitems takes what is above it)
    cap = _walk_bound(nbytes, wbuf_bytes)
    if side.dev:
        cap = min(nbytes // 1024 + -(-nbytes // wbuf_bytes), cap) + nbytes // (100 * 1024) + 64
    else:
        cap += nbytes // 50
    offs, lens, kind = _sized(side, (_U64, _U32, _U8), cap, run)
    info = dict(zip(("nbad", "nsalvaged", "nsuspect", "scanned", "ncand"), (int(c.value) for c in counts[1:])))
    _check_carrying(status[0], "crc32c_triage_pages", _lib.CRC32C_EWORK, offsets=offs, lens=lens, kind=kind, **info)
    return offs, lens, kind, info


def repair_items(buf, item_offsets, region_bytes=0, max_span=0, locate_only=False, stream=None, cflags64=False):
    """Correct single-bit damage of item images from their stored CRC
    (crc32c_repair_items): for every image whose stored CRC does not match,
    the one bit of its stored CRC or span whose inversion explains the
    mismatch is looked for; when it exists, is no length-determining header bit
    and leaves the value ending in CRLF, it is inverted again in ``buf``.

    Returns (ok, bit, {"nrepaired", "nbad"}) for numpy and torch buffers: ok[i]
    is 1 for an intact image, CRC32C_ITEM_REPAIRED (5) for a repaired one with
    bit[i] the image's bit index (bit k % 8 of image byte k // 8), else 0 with
    bit[i] = CRC32C_NO_BIT (not sane, longer than ``max_span`` -- 0: 2 MiB --
    or not explained by one bit).  ``locate_only``: the same verdicts, ``buf``
    is left as it is; a host buffer that is not a writable contiguous uint8
    numpy array is accepted only so.  ``region_bytes`` and ``cflags64`` as for
    verify_items.  Raises Crc32cError(CRC32C_EWORK) when the damaged images'
    spans add up to more than the buffer (a list of overlapping images)."""
    side = _side(buf, stream)
    buf, nbytes = side.buffer(buf, inplace=None if locate_only else
                              "repair_items needs {} (repaired in place) unless locate_only is set")
    offs = side.desc(item_offsets, "item_offsets", _U64)
    n = _count(offs)
    ok, bit = side.empty(n, _U8), side.empty(n, _U64)
    nrepaired, nbad = ctypes.c_uint64(0), ctypes.c_uint64(0)
    flags = side.flag | _flags(cflags64) | (_lib.CRC32C_LOCATE_ONLY if locate_only else 0)
    check(lib.crc32c_repair_items(_ptr(buf), nbytes, region_bytes, _ptr(offs), n, max_span, _ptr(ok), _ptr(bit),
                                  ctypes.byref(nrepaired), ctypes.byref(nbad), flags, side.stream),
          "crc32c_repair_items")
    return ok, bit, {"nrepaired": int(nrepaired.value), "nbad": int(nbad.value)}


def repair_bytes(buf, item_offsets, region_bytes=0, max_span=0, locate_only=False, stream=None, cflags64=False):
    """Restore one damaged byte of item images from their stored CRC
    (crc32c_repair_bytes): for every image whose stored CRC does not match,
    the one byte of its stored CRC or span and the XOR mask (any of the 255)
    that explain the mismatch are looked for; when they exist, the mask
    inverts no length-determining header bit and the corrected value ends in
    CRLF, the byte is put back in ``buf``.

    Returns (ok, byte, mask, {"nrepaired", "nbad"}) for numpy and torch
    buffers: ok[i] is 1 for an intact image, CRC32C_ITEM_REPAIRED (5) for a
    repaired one with byte[i] the image's byte index and mask[i] what it was
    XORed with, else 0 with byte[i] = CRC32C_NO_BIT and mask[i] = 0 (not sane,
    longer than ``max_span`` -- 0: 64 KiB, at most
    CRC32C_REPAIR_BYTES_SPAN_MAX -- or not explained by one byte).  Everything
    repair_items finds this call finds too, but on 32 times weaker evidence: a
    damaged image of another kind (two bits in different bytes included)
    passes for a one-byte error with probability 255 (4 + L) / 2^32.
    ``locate_only``, ``region_bytes``, ``cflags64`` and CRC32C_EWORK as for
    repair_items."""
    side = _side(buf, stream)
    buf, nbytes = side.buffer(buf, inplace=None if locate_only else
                              "repair_bytes needs {} (repaired in place) unless locate_only is set")
    offs = side.desc(item_offsets, "item_offsets", _U64)
    n = _count(offs)
    ok, byte, mask = side.empty(max(n, 1), _U8), side.empty(max(n, 1), _U64), side.empty(max(n, 1), _U8)
    opts = _lib.BytesOpts(side.flag | _flags(cflags64) | (_lib.CRC32C_LOCATE_ONLY if locate_only else 0), max_span,
                          side.stream)
    out = _lib.BytesOut(_ptr(ok), _ptr(byte), _ptr(mask), 0, 0)
    check(lib.crc32c_repair_bytes(_ptr(buf), nbytes, region_bytes, _ptr(offs), n, ctypes.byref(opts),
                                  ctypes.byref(out)), "crc32c_repair_bytes")
    return ok[:n], byte[:n], mask[:n], {"nrepaired": int(out.nrepaired), "nbad": int(out.nbad)}


def locate_byte(crc_computed: int, crc_stored: int, length: int):
    """crc32c_locate_byte, on the host: (p, mask) -- the one byte of a
    ``length``-byte span or of its stored CRC (p < 4: stored-CRC byte p; else
    span byte p - 4) and the XOR mask that turn ``crc_stored`` into a match
    for ``crc_computed`` -- or None."""
    mask = ctypes.c_uint8(0)
    p = int(lib.crc32c_locate_byte(crc_computed & 0xFFFFFFFF, crc_stored & 0xFFFFFFFF, length, ctypes.byref(mask)))
    return None if p == _lib.CRC32C_NO_BIT else (p, int(mask.value))


def repair_headers(buf, item_offsets, region_bytes=0, locate_only=False, stream=None, cflags64=False):
    """Undo a flipped length bit in item headers (crc32c_repair_headers): for
    every listed header that does not verify as it stands, the 42 headers with
    one bit of nbytes, nkey or the two it_flags bits that decide ITEM_ntotal
    inverted are tried, each over its own span; when exactly one of them is
    sane, ends in CRLF and has the stored CRC, that bit is inverted again in
    ``buf``.

    Returns (ok, bit, lens, {"nrepaired", "nbad"}) for numpy and torch buffers:
    ok[i] is 1 for an image that verifies as it stands, CRC32C_ITEM_REPAIRED (5)
    for a repaired header with bit[i] the image's bit index (bit k % 8 of image
    byte k // 8), else 0 with bit[i] = CRC32C_NO_BIT; lens[i] is the image's
    ITEM_ntotal (0 with ok 0).  The list is the caller's: from recover_pages,
    every kind 0 entry and each piece's walk end that is not itself an entry
    (include/crc32c_batch.h).  ``locate_only``: the same verdicts, ``buf`` is
    left as it is; a host buffer that is not a writable contiguous uint8 numpy
    array is accepted only so.  ``region_bytes`` and ``cflags64`` as for
    verify_items.  Raises Crc32cError(CRC32C_EWORK) when the candidate
    variants' spans add up to more than CRC32C_HEADER_WORK_MAX times the buffer."""
    side = _side(buf, stream)
    buf, nbytes = side.buffer(buf, inplace=None if locate_only else
                              "repair_headers needs {} (repaired in place) unless locate_only is set")
    offs = side.desc(item_offsets, "item_offsets", _U64)
    n = _count(offs)
    ok, bit, lens = side.empty(n, _U8), side.empty(n, _U64), side.empty(n, _U32)
    nrepaired, nbad = ctypes.c_uint64(0), ctypes.c_uint64(0)
    flags = side.flag | _flags(cflags64) | (_lib.CRC32C_LOCATE_ONLY if locate_only else 0)
    check(lib.crc32c_repair_headers(_ptr(buf), nbytes, region_bytes, _ptr(offs), n, _ptr(ok), _ptr(bit), _ptr(lens),
                                    ctypes.byref(nrepaired), ctypes.byref(nbad), flags, side.stream),
          "crc32c_repair_headers")
    return ok, bit, lens, {"nrepaired": int(nrepaired.value), "nbad": int(nbad.value)}


def scrub_pages(buf, wbuf_bytes, max_span=0, max_rounds=0, locate_only=False, stream=None, cflags64=False,
                gaps=False, byte_rule=False):
    """A page's whole repair flow in one call (crc32c_scrub_pages):
    triage_pages, rounds of repair_headers over every kind-0 entry and each
    piece's walk end, repair_items over the damaged entries and the suspects
    that overlap nothing proven, and the triage again after every round that
    repaired something, with the page staged once and the lists kept on the
    device.

    Returns (offsets, lens, kind, flip_offsets, flip_bits, flip_by, info) for
    numpy and torch buffers: the final triage list, the log of every bit
    inverted in the order made (the image's offset, the image's bit index, and
    CRC32C_SCRUB_BY_HEADER or CRC32C_SCRUB_BY_ITEM), and info = {"rc", "nbad",
    "nsalvaged", "nsuspect", "scanned", "ncand", "nflips", "headers_repaired",
    "items_repaired", "rounds", "complete"}.  complete 1: nothing more can be
    repaired, a second call changes nothing; 0 with rc 0: ``max_rounds`` (0:
    64) was reached.  rc is CRC32C_OK, or the CRC32C_EWORK / CRC32C_EWALK of
    the stage that ended the flow (what was repaired before stays repaired and
    logged); any other status raises.

    ``locate_only`` (host buffers only): ``buf`` is left as it is, the list and
    the log describe the page as it would be.  A host buffer that is not a
    writable contiguous uint8 numpy array is accepted only so.  The result
    arrays are sized as triage_pages sizes them and the log at one flip per
    256 bytes; a host call that outgrows them is made again (it runs
    locate-only, and the logged bits are inverted here), a device call that
    outgrows the list fetches it with triage_pages, and one that outgrows the
    log returns its first entries (info["nflips"] is exact).

    ``gaps`` sets CRC32C_SCRUB_GAPS: the end of every image found (kind 4)
    that is no entry's offset is handed to both repair stages as well, so an
    image with one flipped length or CRLF bit directly behind a proven one
    comes back, one such image per round.

    ``byte_rule`` sets CRC32C_SCRUB_BYTES: when the item stage repairs nothing,
    repair_bytes runs over the same list (spans up to 64 KiB, or ``max_span``
    when that is smaller), so an image with several bits of one byte inverted
    comes back too.  Its flips are logged one entry per bit with
    CRC32C_SCRUB_BY_BYTE, info["nflips"] counts bits and
    info["items_repaired"] counts its images with the item stage's; such an
    image carries repair_bytes' weaker evidence."""
    wbuf_bytes = _wbuf_bytes(wbuf_bytes)
    side = _side(buf, stream)
    buf, nbytes = side.buffer(buf, inplace=None if locate_only else
                              "scrub_pages needs {} (repaired in place) unless locate_only is set")
    mode = side.flag | _flags(cflags64) | (0 if side.dev and not locate_only else _lib.CRC32C_LOCATE_ONLY)
    mode |= CRC32C_SCRUB_GAPS if gaps else 0
    mode |= CRC32C_SCRUB_BYTES if byte_rule else 0
    opts = _lib.ScrubOpts(mode, max_span, max_rounds, side.stream)
    cap = _walk_bound(nbytes, wbuf_bytes)
    if side.dev:
        cap = min(nbytes // 1024 + -(-nbytes // wbuf_bytes), cap) + nbytes // (100 * 1024) + 64
    else:
        cap += nbytes // 50
    flip_cap = nbytes // 256 + 64
    while True:
        arrays = [side.empty(cap, k) for k in (_U64, _U32, _U8)] + [side.empty(flip_cap, k) for k in (_U64, _U64, _U8)]
        out = _lib.ScrubOut(*map(_ptr, arrays[:3]), cap, *map(_ptr, arrays[3:]), flip_cap)
        rc = lib.crc32c_scrub_pages(_ptr(buf), nbytes, wbuf_bytes, ctypes.byref(opts), ctypes.byref(out))
        if rc not in (_lib.CRC32C_EWORK, _lib.CRC32C_EWALK):
            check(rc, "crc32c_scrub_pages")
        if side.dev or (out.nitems <= cap and out.nflips <= flip_cap):
            break
        cap, flip_cap = max(cap, out.nitems), max(flip_cap, out.nflips)
    offs, lens, kind = (a[:min(out.nitems, cap)] for a in arrays[:3])
    flips = [a[:min(out.nflips, flip_cap)] for a in arrays[3:]]
    if side.dev and out.nitems > cap and rc == _lib.CRC32C_OK:
        offs, lens, kind, _ = triage_pages(buf, wbuf_bytes, stream=stream, cflags64=cflags64)
    if not side.dev and not locate_only:
        for o, k in zip(flips[0].tolist(), flips[1].tolist()):
            buf[o + k // 8] ^= 1 << (k % 8)
    info = {name: int(getattr(out, name)) for name in ("nbad", "nsalvaged", "nsuspect", "scanned", "ncand", "nflips",
                                                       "headers_repaired", "items_repaired", "rounds", "complete")}
    info["rc"] = rc
    return (offs, lens, kind, *flips, info)


def locate_bit(crc_computed: int, crc_stored: int, length: int) -> int:
    """crc32c_locate_bit, on the host: the one position of a ``length``-byte
    span or of its stored CRC whose inversion turns ``crc_stored`` into a match
    for ``crc_computed`` -- q < 32: bit q of the stored CRC; else bit (q - 32) %
    8 of span byte (q - 32) // 8 -- or CRC32C_NO_BIT."""
    return int(lib.crc32c_locate_bit(crc_computed & 0xFFFFFFFF, crc_stored & 0xFFFFFFFF, length))


def batch_chains(buf, offsets, lens, chain_first, stream=None):
    """Chained CRC per iov list: chain c covers iovs [chain_first[c],
    chain_first[c+1]) of the spans (offsets[i], lens[i]) of ``buf`` and gets
    crc32c(...crc32c(crc32c(0, iov_a), iov_a+1)..., iov_b-1)."""
    side = _side(buf, stream)
    nchains = len(chain_first) - 1
    s, _iov_out = _spans(side, buf, offsets, 0, lens, 0, None, None)
    chain_first = side.desc(chain_first, "chain_first", _U64, nchains + 1)
    out = side.empty(nchains, _U32)
    check(lib.crc32c_batch_chains(ctypes.byref(s), _ptr(chain_first), nchains, _ptr(out), side.flag, side.stream),
          "crc32c_batch_chains")
    return out


def _ptr_batch(buffers, crc_in, stream):
    """(side, crc32c_ptr_batch, out) of a list of buffers: device tensors (all
    of them: a device batch, its descriptors built on their device) or host
    data (numpy arrays, bytes: read where they lie)."""
    buffers = list(buffers)
    n = len(buffers)
    if any(_is_dev(b) for b in buffers):
        if not all(_is_dev(b) for b in buffers):
            raise ValueError("buffers: device tensors and host data in one batch")
        side = _Device(buffers[0], stream)
    else:
        side = _HOST
    bufs = [side.buffer(b, f"buffers[{i}]") for i, b in enumerate(buffers)]
    ptrs = np.array([_ptr(b) if nb else 0 for b, nb in bufs], np.uint64)
    lens = np.array([nb for _, nb in bufs], np.uint32)
    if side.dev:  # the descriptors of a device batch are device arrays
        ptrs = side.torch.from_numpy(ptrs.view(np.int64)).to(side.device)
        lens = side.torch.from_numpy(lens.view(np.int32)).to(side.device)
    crc_in = side.desc(crc_in, "crc_in", _U32, n)
    out = side.empty(n, _U32)
    b = _lib.PtrBatch(_ptr(ptrs), _ptr(lens), 0, _ptr(crc_in), _ptr(out), n)
    b.arrays = bufs, ptrs, lens, crc_in  # (bare addresses: the converted copies live as long as the struct)
    return side, b, out


def batch_ptrs(buffers, crc_in=None, stream=None):
    """crc32c_batch_ptrs: the CRC-32C of each of ``buffers`` -- a list of numpy
    arrays or bytes wherever they lie (page-locked ones are read in place, the
    others' bytes are packed), or a list of device tensors from any
    allocations.  Returns uint32 CRCs, one per buffer; crc_in[i] starts the
    i-th (default 0)."""
    side, b, out = _ptr_batch(buffers, crc_in, stream)
    opts = _lib.PtrOpts(side.flag, side.stream)
    check(lib.crc32c_batch_ptrs(ctypes.byref(b), ctypes.byref(opts)), "crc32c_batch_ptrs")
    return out


def chains_ptrs(buffers, chain_first, stream=None):
    """crc32c_chains_ptrs: batch_chains over iovs given as a list of buffers
    (as for batch_ptrs): chain c covers buffers [chain_first[c],
    chain_first[c+1])."""
    side, b, _iov_out = _ptr_batch(buffers, None, stream)
    nchains = len(chain_first) - 1
    chain_first = side.desc(chain_first, "chain_first", _U64, nchains + 1)
    out = side.empty(nchains, _U32)
    opts = _lib.PtrOpts(side.flag, side.stream)
    check(lib.crc32c_chains_ptrs(ctypes.byref(b), _ptr(chain_first), nchains, _ptr(out), ctypes.byref(opts)),
          "crc32c_chains_ptrs")
    return out


def shard_cuts(lens, parts: int):
    """crc32c_shard_cuts: the parts + 1 cut points of the byte-balanced split
    crc32c_batch_multi uses over spans of lengths ``lens`` (uint32)."""
    lens = np.ascontiguousarray(lens, dtype=np.uint32)
    cuts = np.empty(parts + 1, dtype=np.uint64)
    check(lib.crc32c_shard_cuts(lens.ctypes.data, 0, lens.size, parts, cuts.ctypes.data), "crc32c_shard_cuts")
    return cuts.astype(np.int64)


def queue_stats():
    """(launches, spans, jobs, solo_jobs) of the current device's coalescing queue."""
    v = [ctypes.c_uint64(0) for _ in range(4)]
    check(lib.crc32c_queue_stats(*[ctypes.byref(x) for x in v]), "crc32c_queue_stats")
    return tuple(int(x.value) for x in v)


def set_small_max(n: int) -> int:
    """Batches of at most n spans take the single-launch kernel (0: none); returns the previous value."""
    return int(lib.crc32c_set_small_max(n))


def set_k1_tail_min(steps: int) -> int:
    """Batches of equal 4 KiB spans with at least `steps` steps per wave have their last eighth claimed in
    chunks (2**64 - 1: never); returns the previous value."""
    return int(lib.crc32c_set_k1_tail_min(steps))

"""CPU model of the stamp calls with and without CRC32C_KEEP_STAMPED, and of
the page walk that crc32c_stamp_pages shares with crc32c_verify_pages.

Built on the oracle (oracle.item_crc) and layout.ntotal_of only: nothing here
comes from libmcrc32c.so.  It is _expected_verdicts of test_gpu_items_queue.py
extended with the stored-zero rule:

    header not sane          untouched, ok 0, counted bad
    exptime == 0 (fresh)     exptime = crc, ok 1
    exptime != 0 (carried)   untouched; ok 2 when exptime == crc, else ok 0, bad

Without the flag every sane image is stamped (ok 1)."""
import numpy as np

from memcached_amd import layout

from . import oracle

STAMPED, KEPT = 1, 2


def _u32(buf, at):
    return int.from_bytes(bytes(buf[at:at + 4]), "little")


def header_sane(buf, o, wbuf, cfl=4):
    """The library's rule for an image at o: the header lies in the buffer,
    nkey != 0, nbytes < 2^31, and the image ends inside the buffer and inside
    its own wbuf (wbuf == 0: no such bound)."""
    o = int(o)
    if o + 48 > buf.size or buf[o + layout.NKEY_OFF] == 0:
        return False
    if _u32(buf, o + layout.NBYTES_OFF) >= 1 << 31:
        return False
    nt = layout.ntotal_of(buf, o, cfl)
    return o + nt <= buf.size and (wbuf == 0 or o // wbuf == (o + nt - 1) // wbuf)


def expected_stamp(buf, offs, wbuf, keep, cfl=4):
    """(bytes after the call, ok per image, nbad) of a stamp of the images at
    offs.  Images must not overlap a fresh image's exptime (the header documents
    that case as undefined)."""
    out = buf.copy()
    ok = np.zeros(len(offs), np.uint8)
    for i, o in enumerate(np.asarray(offs, np.uint64).tolist()):
        if not header_sane(buf, o, wbuf, cfl):
            continue
        crc = oracle.item_crc(buf, o, cfl)
        stored = _u32(buf, o + layout.EXPTIME_OFF)
        if keep and stored != 0:
            ok[i] = KEPT if stored == crc else 0
        else:
            out[o + 28:o + 32] = np.frombuffer(int(crc).to_bytes(4, "little"), np.uint8)
            ok[i] = STAMPED
    return out, ok, int((ok == 0).sum())


def expected_verify(buf, offs, wbuf, cfl=4):
    """ok per image of crc32c_verify_items."""
    ok = np.zeros(len(offs), np.uint8)
    for i, o in enumerate(np.asarray(offs, np.uint64).tolist()):
        if header_sane(buf, o, wbuf, cfl):
            ok[i] = _u32(buf, o + layout.EXPTIME_OFF) == oracle.item_crc(buf, o, cfl)
    return ok


def host_walk(buf, wbuf, cfl=4):
    """Offsets of the images the page walk finds in buf (storage.c:950-960):
    every wbuf-sized piece from its start, nkey == 0 or fewer than 48 bytes
    left end it, the next image at + ITEM_ntotal (unsigned)."""
    offs = []
    for w0 in range(0, buf.size, wbuf):
        o, end = w0, min(w0 + wbuf, buf.size)
        while o + 48 <= end and buf[o + layout.NKEY_OFF] != 0:
            offs.append(o)
            nbytes = _u32(buf, o + layout.NBYTES_OFF)
            o += layout.ntotal_of(buf, o, cfl) - int(np.int32(np.uint32(nbytes))) + nbytes
    return np.asarray(offs, np.uint64)

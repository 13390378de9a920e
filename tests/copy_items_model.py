"""CPU model of crc32c_copy_items.

Built on keep_stamped_model.header_sane, layout.ntotal_of and oracle.item_crc
only: nothing here comes from libmcrc32c.so.

    source image not sane          nothing written, ok 0, counted bad
    sane, does not fit dst         nothing written, ok 0, counted bad, ERANGE
    sane, fits, exptime == crc     all ITEM_ntotal bytes written, ok 1
    sane, fits, exptime != crc     all ITEM_ntotal bytes written, ok 3, counted bad
"""
import numpy as np

from memcached_amd import layout

from . import oracle
from .keep_stamped_model import _u32, header_sane

COPIED, DAMAGED = 1, 3


def expected_copy(src, src_offs, wbuf, dst_init, dst_offs, cfl=4):
    """(dst after the call, ok per image, nbad, erange) of a copy of the images
    at src_offs of src (wbuf: the source's region_bytes, 0 = none) to dst_offs
    of a buffer that holds dst_init.  Destination images must not overlap."""
    dst = np.array(dst_init, np.uint8)
    ok = np.zeros(len(src_offs), np.uint8)
    erange = False
    pairs = zip(np.asarray(src_offs, np.uint64).tolist(), np.asarray(dst_offs, np.uint64).tolist())
    for i, (so, do) in enumerate(pairs):
        if not header_sane(src, so, wbuf, cfl):
            continue
        nt = layout.ntotal_of(src, so, cfl)
        if do + nt > dst.size:
            erange = True
            continue
        dst[do:do + nt] = src[so:so + nt]
        ok[i] = COPIED if _u32(src, so + layout.EXPTIME_OFF) == oracle.item_crc(src, so, cfl) else DAMAGED
    return dst, ok, int((ok != COPIED).sum()), erange

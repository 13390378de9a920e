"""Buffers for the crc32c_copy_items tests (no GPU, no library call):
tests/test_gpu_copy_items.py and tests/interleave_cases.py share them."""
import functools

import numpy as np

from memcached_amd import layout

from . import keep_stamped_model as ks
from . import oracle

WBUF = 1 << 20


def stamp_all(buf, offs, cfl=4):
    """Every image carries its spill CRC (storage.c:567)."""
    crcs = np.array([oracle.item_crc(buf, o, cfl) for o in offs], np.uint32)
    assert (crcs != 0).all()
    layout.store_crcs(buf, offs, crcs)


@functools.lru_cache(maxsize=None)
def mixed_case():
    """The `mixed` shape of test_gpu_keep_stamped.py (900 images, values of
    0..9000 B, 1 MiB wbufs), every image carrying its CRC, then damaged; the
    destinations are packed back to back from the headers as found."""
    rng = np.random.default_rng(371)
    items = [layout.make_item(b"ks%06d" % i, rng.integers(0, 256, int(rng.integers(0, 9000)), dtype=np.uint8).tobytes(),
                              cas=i + 1) for i in range(900)]
    src, offs = layout.pack_wbufs(items, WBUF)
    stamp_all(src, offs)
    data_bit = list(range(0, 900, 10))
    for i in data_bit:
        o, nt = int(offs[i]), layout.ntotal_of(src, int(offs[i]))
        src[o + 48 + int(rng.integers(0, nt - 48))] ^= 1 << int(rng.integers(0, 8))
    clsid, lenbit_sane, lenbit_out, nokey = 123, 457, 401, 301
    src[int(offs[clsid]) + 40] ^= 0x40        # slabs_clsid: in the span, the header stays sane
    assert int(offs[lenbit_sane + 1]) // WBUF == int(offs[lenbit_sane]) // WBUF  # (not the last of its wbuf)
    src[int(offs[lenbit_sane]) + 32] ^= 0x01  # nbytes +- 1: still sane, another ITEM_ntotal
    src[int(offs[lenbit_out]) + 34] ^= 0x10   # nbytes += 1 MiB: the image leaves its wbuf
    src[int(offs[nokey]) + 41] = 0
    soffs = np.concatenate([offs, np.array([src.size - 20], np.uint64)])  # a header cut by the buffer's end
    damaged = set(data_bit) | {clsid, lenbit_sane}
    dropped = {lenbit_out, nokey, 900}
    doffs, at = [], 0
    for o in soffs.tolist():
        doffs.append(at)
        if ks.header_sane(src, o, WBUF):
            at += layout.ntotal_of(src, o)  # (the damaged header's own length, as a caller would)
    src.flags.writeable = False
    return src, soffs, np.array(doffs, np.uint64), at, damaged, dropped

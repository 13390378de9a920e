"""The batches of tests/test_gpu_routes.py (no GPU, no library call): the
smallest ones on each side of the boundaries that host_route.h draws, and what
the oracle and the CPU models of tests/keep_stamped_model.py expect of them.
tests/interleave_cases.py runs the same batches between other calls.  Built
once per process and left read-only."""
import functools

import numpy as np

from memcached_amd import layout

from . import keep_stamped_model as model
from . import oracle

MiB = 1 << 20
WBUF = 4 * MiB


# -- spans ---------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def short_spans():
    """8193 spans of 1..300 B at unaligned offsets of a buffer under 8 MiB, and
    their CRCs."""
    rng = np.random.default_rng(811)
    lens = rng.integers(1, 301, 8193).astype(np.uint32)
    offs = (np.cumsum(lens + rng.integers(0, 40, 8193)) - lens + 3).astype(np.uint64)
    buf = rng.integers(0, 256, int(offs[-1]) + 300 + 5, dtype=np.uint8)
    assert buf.size <= 8 * MiB and len(set((offs % 16).tolist())) == 16
    return buf, offs, lens, oracle.batch(buf, offs, lens)


# -- items ---------------------------------------------------------------------

def mixed(items, rng, pad_to=None, nokey=True):
    """The images back to back (in a buffer of pad_to bytes): by i % 3 fresh,
    carried, carried; of every 500 (at least 5) carried images one with a
    flipped data bit, and two images with nkey = 0."""
    offs = np.cumsum([0] + [len(im) for im in items[:-1]]).astype(np.uint64)
    raw = b"".join(bytes(im) for im in items)
    buf = np.zeros(pad_to or len(raw), np.uint8)
    buf[:len(raw)] = np.frombuffer(raw, np.uint8)
    n = len(items)
    carried = np.array([i for i in range(n) if i % 3])
    crcs = np.array([oracle.item_crc(buf, o) for o in offs[carried]], np.uint32)
    assert (crcs != 0).all()
    layout.store_crcs(buf, offs[carried], crcs)
    for i in rng.choice(carried, max(5, n // 500), replace=False).tolist():
        o = int(offs[i])
        buf[o + 48 + int(rng.integers(0, layout.ntotal_of(buf, o) - 48))] ^= 1 << int(rng.integers(0, 8))
    for i in (7, n - 2) if nokey else ():
        buf[int(offs[i]) + layout.NKEY_OFF] = 0
    buf.flags.writeable = False
    return buf, offs


@functools.lru_cache(maxsize=None)
def items_case(name):
    rng = np.random.default_rng(len(name) * 1000 + sum(name.encode()))
    if name.startswith("64"):  # 64 images in exactly 8 MiB (small) or 128 B more (planned)
        items = [layout.make_item(b"r%05d" % i,
                                  rng.integers(0, 256, int(rng.integers(0, 9000)), dtype=np.uint8).tobytes(), cas=i + 1)
                 for i in range(64)]
        buf, offs = mixed(items, rng, pad_to=8 * MiB + (128 if name == "64+128" else 0))
    else:  # 4095 (planned) or 4096 (K5 with a fallback list) images of 4165 B, every 400th of another size
        n = int(name)
        vals = [4096 if i % 400 else int(rng.integers(100, 9000)) for i in range(n)]
        items = [layout.make_item(b"key%07d" % i, rng.integers(0, 256, v, dtype=np.uint8).tobytes(), cas=i + 1)
                 for i, v in enumerate(vals)]
        assert len(items[1]) == 4165
        buf, offs = mixed(items, rng)
        assert buf.size > 8 * MiB
    return buf, offs


@functools.lru_cache(maxsize=None)
def items_want(name, mode):
    """(the buffer afterwards, ok, nbad) of a verify, a stamp or a stamp that
    keeps carried CRCs."""
    buf, offs = items_case(name)
    if mode == "verify":
        ok = model.expected_verify(buf, offs, 0)
        return buf, ok, int((ok == 0).sum())
    return model.expected_stamp(buf, offs, 0, keep=mode == "keep")


# -- pages ---------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def pages_case(nwbufs):
    """nwbufs 4 MiB wbufs of 4165-B images (1007 each: one wbuf is a small
    batch, five are past 4096 items) with zero tails, mixed as mixed() makes
    them but for the nkey = 0 images (they would end their wbuf's walk)."""
    rng = np.random.default_rng(nwbufs)
    per = WBUF // 4165
    buf = np.zeros(nwbufs * WBUF, np.uint8)
    for w in range(nwbufs):
        items = [layout.make_item(b"key%07d" % (w * per + i), rng.integers(0, 256, 4096, dtype=np.uint8).tobytes(),
                                  cas=i + 1) for i in range(per)]
        part, _ = mixed(items, rng, nokey=False)
        buf[w * WBUF:w * WBUF + part.size] = part
    walked = model.host_walk(buf, WBUF)
    assert walked.size == nwbufs * per and (nwbufs == 1) == (walked.size <= 4096)
    buf.flags.writeable = False
    return buf, walked


@functools.lru_cache(maxsize=None)
def pages_want(nwbufs):
    """(verify's ok, the keeping stamp's (buffer, ok, nbad), the plain stamp's)."""
    buf, walked = pages_case(nwbufs)
    v_ok = model.expected_verify(buf, walked, WBUF)
    return v_ok, model.expected_stamp(buf, walked, WBUF, keep=True), model.expected_stamp(buf, walked, WBUF, keep=False)

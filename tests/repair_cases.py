"""Buffers for the crc32c_repair_items tests (no GPU, no library call):
tests/test_gpu_repair.py and tests/interleave_cases.py share them."""
import numpy as np

from tests import repair_model as rm
from tests import salvage_cases as sc


def flip(buf, o, k):
    buf[o + k // 8] ^= 1 << (k % 8)


def place(images, align=1, lead=0):
    """(buffer, offsets): the images packed, each start rounded up to align, + lead."""
    offs, o = [], 0
    for img in images:
        o = -(-o // align) * align + lead
        offs.append(o)
        o += len(img)
    buf = np.zeros(o + 64, np.uint8)
    for at, img in zip(offs, images):
        buf[at:at + len(img)] = np.frombuffer(bytes(img), np.uint8)
    return buf, np.array(offs, np.uint64)


def mixed(rng, n, max_span):
    """n small images in one buffer, damaged by class, two long ones among them."""
    images = [sc.image_nt(rng, int(rng.integers(60, 200)), cas=bool(i & 1)) for i in range(n)]
    images[n // 3] = sc.image_nt(rng, max_span + 32 + 1)  # one byte over max_span
    images[n // 2] = sc.image_nt(rng, max_span + 32)      # just within
    buf, offs = place(images)
    kinds = []
    for i, (o, img) in enumerate(zip(offs.tolist(), images)):
        nt, c = len(img), i % 10
        if i in (n // 3, n // 2) or c in (3, 9):  # one bit
            k = int(rng.integers(224, 8 * nt))
            while rm.length_bit(k):
                k = int(rng.integers(224, 8 * nt))
            flip(buf, o, k)
        elif c in (4, 5):  # two bits, three bits
            for k in rng.choice(np.arange(224, 8 * nt), 2 + (c == 5), replace=False).tolist():
                flip(buf, o, int(k))
        elif c == 6:  # outside what the CRC covers
            flip(buf, o, int(rng.integers(0, 224)))
        elif c == 7:  # a length bit
            flip(buf, o, [8 * 32 + int(rng.integers(0, 32)), 8 * 41 + int(rng.integers(0, 8)), 8 * 38 + 1,
                           8 * 39][int(rng.integers(0, 4))])
        elif c == 8:  # not sane
            buf[o + 41] = 0
        kinds.append(c)
    return buf, offs, np.array(kinds)

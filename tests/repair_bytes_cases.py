"""Buffers for the crc32c_repair_bytes tests (no GPU, no library call):
tests/test_repair_bytes_model.py and tests/test_gpu_repair_bytes.py share them."""
import numpy as np

from tests import repair_bytes_model as bm
from tests import salvage_cases as sc
from tests.repair_cases import place

TWO_BYTES_SEED = 1414  # pinned: two_bytes() asserts that the model locates nothing in what this seed makes


def xor_byte(buf, o, p, m):
    buf[o + p] ^= m


def heavy_mask(rng):
    """A byte mask of weight >= 2."""
    while True:
        m = int(rng.integers(1, 256))
        if m & (m - 1):
            return m


def two_bytes(n=64):
    """(buffer, offsets): n images of 52..600 bytes, each with two different
    covered bytes XORed by masks of their own (no length byte among them), the
    even ones by one bit each -- the damage crc32c_repair_items' even-weight
    guarantee covers and this rule does not.  None has a located pair under
    the model (a chance of 255 (4 + L) / 2^32 each; the seed is pinned)."""
    rng = np.random.default_rng(TWO_BYTES_SEED)
    nts = rng.integers(52, 601, n).tolist()
    images = [sc.image_nt(rng, nt, cas=bool(i & 2) and nt >= 60) for i, nt in enumerate(nts)]
    buf, offs = place(images, align=1, lead=1)
    for i, (o, img) in enumerate(zip(offs.tolist(), images)):
        while True:
            p, q = sorted(rng.choice(np.arange(28, len(img)), 2, replace=False).tolist())
            if not ({p, q} & {32, 33, 34, 35, 38, 39, 41}):
                break
        for at in (p, q):
            xor_byte(buf, o, at, 1 << int(rng.integers(0, 8)) if i % 2 == 0 else int(rng.integers(1, 256)))
        assert bm.located_syndrome(buf[o:o + len(img)]) == [], (i, p, q)
        if len(img) <= 80:
            assert bm.located_brute(buf[o:o + len(img)]) == [], (i, p, q)
    return buf, offs


def mixed(rng, n, percent=1):
    """(buffer, offsets, damaged): n images of 52 (the smallest there is) to
    4200 bytes, `percent` of a hundred with one covered byte XORed by a mask of
    weight >= 2; damaged[i] is (image byte, mask) or None."""
    nts = rng.integers(52, 4201, n).tolist()
    images = [sc.image_nt(rng, nt, cas=bool(i & 1) and nt >= 60) for i, nt in enumerate(nts)]
    buf, offs = place(images)
    damaged = [None] * n
    for i in rng.choice(n, n * percent // 100, replace=False).tolist():
        p, m = int(rng.integers(28, len(images[i]))), heavy_mask(rng)
        xor_byte(buf, int(offs[i]), p, m)
        damaged[i] = (p, m)
    return buf, offs, damaged


def edge_steps(length):
    """The byte steps the edge test damages in a codeword of 4 + length bytes."""
    steps = 4 + length
    return sorted({j for j in (0, 3, 4, 5, 255, 256, steps - 1) if j < steps})

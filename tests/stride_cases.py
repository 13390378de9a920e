"""Fixed-stride span batches (crc32c_spans with offsets == NULL: span i starts
at i * stride) at every route they can take.  Plain numpy, no GPU and no
library call: tests/test_host_route.py asks span_route itself whether each case
takes the route it names and whether its buffer is the smallest the library
accepts, tests/test_gpu_strides.py runs the library over the same cases.

A case is n spans of `length` bytes (or of lens[i] bytes: the shape
mc.batch(buf, stride=..., lens=...) builds) in a seeded buffer of exactly
(n - 1) * stride + length bytes (with lens[]: up to the last span's end, and
`length` is a decoy the library must ignore).  Every expected CRC is the
oracle over that buffer.

The strides of a length L, each a different layout for the kernels:
    L                   back to back
    L + 32              the extstore image shape (a 4133-byte span per 4165-byte image)
    L up to a 128       every span at one residue mod 128
    L - 1               each span overlaps the next by a byte
    1                   every residue mod 128 in sequence, maximal overlap
    0                   every span the same bytes: every output equal
Strides that coincide are listed once; a length of 4096 keeps only strides
that are no multiple of 16 (the others are K1's shape).
"""
from __future__ import annotations

import functools
from dataclasses import dataclass, field

import numpy as np

from . import oracle

N = 131  # odd, over two K5 waves' worth (64 each), past k_blocks' first look-ahead of 2 gstep groups
DECOY_LEN = 12345  # `len` of a case that gives lens[]

ROUTES = ("small", "k5", "id_blocks", "id_spans", "id_final", "planned")


@dataclass(frozen=True)
class Case:
    name: str
    n: int
    length: int                # every span's length; with lens: the decoy
    stride: int
    small_max: int | None      # crc32c_set_small_max for the call (None: the default, 8192)
    route: str                 # span_route's answer at a 16-byte aligned base
    seed: int
    lens_kind: str = ""        # "": no lens[]; else the name of the lens[] recipe
    host: bool = False         # also run through the host path
    _cache: dict = field(default_factory=dict, compare=False, repr=False)

    @property
    def lens(self) -> np.ndarray | None:
        if not self.lens_kind:
            return None
        if "lens" not in self._cache:
            self._cache["lens"] = _ro(_mixed_lens(self.n, self.seed))
        return self._cache["lens"]

    @property
    def nbytes(self) -> int:
        """(n - 1) * stride + length; with lens[] the last byte any span reaches."""
        if self.lens is None:
            return (self.n - 1) * self.stride + self.length
        return int((self.offsets().astype(np.int64) + self.lens.astype(np.int64)).max())

    def offsets(self) -> np.ndarray:
        return np.arange(self.n, dtype=np.uint64) * np.uint64(self.stride)

    def span_lens(self) -> np.ndarray:
        return np.full(self.n, self.length, np.uint64) if self.lens is None else self.lens.astype(np.uint64)

    @property
    def buf(self) -> np.ndarray:
        if "buf" not in self._cache:
            rng = np.random.default_rng(self.seed)
            self._cache["buf"] = _ro(rng.integers(1, 256, self.nbytes, dtype=np.uint8))
        return self._cache["buf"]

    @property
    def crc_in(self) -> np.ndarray:
        if "cin" not in self._cache:
            rng = np.random.default_rng(self.seed + 1)
            self._cache["cin"] = _ro(rng.integers(0, 2**32, self.n, dtype=np.uint64).astype(np.uint32))
        return self._cache["cin"]

    def expected(self, with_crc_in: bool) -> np.ndarray:
        """The oracle's CRC of every span, from 0 or from crc_in[i] (computed once)."""
        key = ("want", with_crc_in)
        if key not in self._cache:
            self._cache[key] = _ro(oracle.batch(self.buf, self.offsets(), self.span_lens(),
                                                self.crc_in if with_crc_in else None))
        return self._cache[key]


def _ro(a):
    a.setflags(write=False)
    return a


def _mixed_lens(n, seed):
    """Lengths 0..5000 with every 16th span (from the 5th) of 70 000..300 000 bytes, the shortest and
    the longest of both kinds among them."""
    rng = np.random.default_rng(seed + 2)
    lens = rng.integers(0, 5001, n)
    lens[:6] = [0, 1, 511, 512, 513, 5000]
    long_at = np.arange(5, n - 3, 16)
    lens[long_at] = rng.integers(70000, 300001, long_at.size)
    lens[long_at[:2]] = [70000, 300000]
    return lens.astype(np.uint32)


def strides_of(L: int) -> list[int]:
    """The strides of the module's docstring for length L, without repeats, in that order."""
    want = [L, L + 32, (L + 127) // 128 * 128, L - 1, 1, 0]
    if L == 4096:
        want = [4096 + 40, 4095, 1]  # (K1 takes 4096-byte spans at a stride that is a multiple of 16)
    out = []
    for s in want:
        if s >= 0 and s not in out:
            out.append(s)
    return out


# route -> (lengths, small_max)
FIXED = {
    "k5": ((4099, 4133, 4227), 0),
    "id_blocks": ((4081, 4097, 4096), 0),
    "id_final": ((0, 1, 385), 0),
    "id_spans": ((386, 512, 4080, 4098, 4228, 8195, 131072), 0),
    "planned": ((131073,), 0),
    "small": ((77, 4133, 65537), None),
}
K5_SIZES = (1, 63, 64, 65, 8193)  # around one wave's 64 images; 8193: two steps a run on 256 CUs, the last run cut
# the strides of the host-path subset, per route (the overlapping L - 1 among them)
_HOST = {("k5", 4133): 4165, ("id_blocks", 4097): 4096, ("id_final", 385): 384, ("id_spans", 4098): 4097,
         ("id_spans", 131072): 131071, ("planned", 131073): 131072, ("small", 4133): 4132}


@functools.lru_cache(maxsize=None)
def cases() -> tuple[Case, ...]:
    out = []
    seed = 2100
    for route, (lengths, sm) in FIXED.items():
        for L in lengths:
            for stride in strides_of(L):
                seed += 3
                out.append(Case(f"{route}_len{L}_stride{stride}", N, L, stride, sm, route, seed,
                                host=_HOST.get((route, L)) == stride))
    for n in K5_SIZES:
        seed += 3
        out.append(Case(f"k5_len4133_stride4165_n{n}", n, 4133, 4165, 0, "k5", seed))
    # stride with lens[]: k_count's stride branch (planned), and k_small's
    for name, stride, sm, route in (("planned_lens_apart", 300032, 0, "planned"),      # no span reaches the next
                                    ("planned_lens_overlap", 4096, 0, "planned"),     # the long ones cover 17-73 others
                                    ("small_lens_overlap", 4096, None, "small")):
        seed += 3
        out.append(Case(name, N, DECOY_LEN, stride, sm, route, seed, lens_kind="mixed", host=True))
    assert len({c.name for c in out}) == len(out)
    return tuple(out)


def by_name(name: str) -> Case:
    return {c.name: c for c in cases()}[name]


# The 2^31 line: k1_shape refuses stride >= 2^31 (K1 multiplies by a 32-bit stride); the routes that take
# over must keep i * stride in 64 bits.  (length, stride, route with small_max 0); three spans each, so the
# last one starts at or past 2^32.
LINE = 1 << 31
LINE_CASES = ((4096, LINE - 16, "k1"), (4096, LINE, "id_blocks"), (4096, LINE + 16, "id_blocks"),
              (4133, LINE + 32, "k5"), (4098, LINE + 1, "id_spans"))
LINE_N = 3

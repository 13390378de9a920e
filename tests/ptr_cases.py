"""Cases for the pointer batches (crc32c_batch_ptrs, crc32c_chains_ptrs).
Plain numpy, no GPU and no library call; tests/test_gpu_ptrs.py runs them.

A case names its spans by (allocation, offset, length): `bufs` are the
allocations' bytes, span i lies in bufs[where[i]] at offs[i].  Where the test
places each allocation (device, pageable, page-locked) decides the pointers:
ptrs[i] = base(where[i]) + offs[i].

Every existing span and chain case is re-expressed so, over its one buffer:
routes_cases.short_spans(), every case of stride_cases.cases() and of
chain_cases.small_cases().  scattered() adds what only pointers can say: spans
in three allocations, in descending address order, one listed twice, two
overlapping."""
from __future__ import annotations

import functools
from dataclasses import dataclass, field

import numpy as np

from . import chain_cases as cc
from . import oracle
from . import routes_cases as rc
from . import stride_cases as sc


@dataclass
class Case:
    name: str
    bufs: list                     # uint8 arrays, one per allocation
    where: np.ndarray              # per span: its allocation
    offs: np.ndarray               # uint64, per span: its offset there
    lens: np.ndarray | None        # uint32; None: every span `length` bytes
    length: int = 0                # with lens given: a decoy the library must ignore
    small_max: int | None = None   # crc32c_set_small_max for the call (None: leave it)
    first: np.ndarray | None = None  # chain cases: chain_first
    source: object = None          # the re-expressed case (None: only pointers can say this one)
    _cache: dict = field(default_factory=dict, compare=False, repr=False)

    @property
    def n(self) -> int:
        return self.offs.size

    def span_lens(self) -> np.ndarray:
        return np.full(self.n, self.length, np.uint64) if self.lens is None else self.lens.astype(np.uint64)

    @property
    def crc_in(self) -> np.ndarray:
        if "cin" not in self._cache:
            rng = np.random.default_rng(self.n * 7 + len(self.name))
            self._cache["cin"] = _ro(rng.integers(0, 2**32, self.n, dtype=np.uint64).astype(np.uint32))
        return self._cache["cin"]

    def expected(self, with_crc_in: bool = False) -> np.ndarray:
        """The oracle's CRC of every span, from 0 or from crc_in[i] (computed once)."""
        if with_crc_in not in self._cache:
            want = np.zeros(self.n, np.uint32)
            lens = self.span_lens()
            for k, buf in enumerate(self.bufs):
                at = np.flatnonzero(self.where == k)
                if at.size:
                    want[at] = oracle.batch(buf, self.offs[at], lens[at], self.crc_in[at] if with_crc_in else None)
            self._cache[with_crc_in] = _ro(want)
        return self._cache[with_crc_in]

    def expected_chains(self) -> np.ndarray:
        """out[c] of crc32c_chains_ptrs: the oracle over the chain's bytes, one after the other."""
        if "chains" not in self._cache:
            lens = self.span_lens().astype(np.int64)
            out = np.zeros(self.first.size - 1, np.uint32)
            for c in range(out.size):
                crc = 0
                for i in range(int(self.first[c]), int(self.first[c + 1])):
                    o = int(self.offs[i])
                    crc = oracle.crc32c(crc, self.bufs[int(self.where[i])][o:o + int(lens[i])])
                out[c] = crc
            self._cache["chains"] = _ro(out)
        return self._cache["chains"]


def _ro(a):
    a.setflags(write=False)
    return a


def _one(name, buf, offs, lens, length, small_max, source, first=None):
    offs = np.asarray(offs, np.uint64)
    return Case(name, [buf], np.zeros(offs.size, np.int64), offs, lens, length, small_max, first, source)


@functools.lru_cache(maxsize=None)
def span_cases() -> tuple[Case, ...]:
    """short_spans() as it routes by default and planned, and every fixed-stride case."""
    buf, offs, lens, _ = rc.short_spans()
    out = [_one("short_spans", buf, offs, lens, 0, None, "short_spans"),
           _one("short_spans_first_8192", buf, offs[:8192], lens[:8192], 0, None, "short_spans"),
           _one("short_spans_planned", buf, offs, lens, 0, 0, "short_spans")]
    for c in sc.cases():
        out.append(_one("stride_" + c.name, c.buf, c.offsets(), c.lens, c.length, c.small_max, c))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def chain_cases() -> tuple[Case, ...]:
    return tuple(_one("chain_" + c.name, c.buf, c.iov_offsets(), c.lens, c.length, c.small_max, c, first=c.first)
                 for c in cc.small_cases())


SCATTER_LENS = (0, 1, 3, 15, 16, 17, 4095, 4096, 4097, 4133)


@functools.lru_cache(maxsize=None)
def scattered() -> Case:
    """48 spans in three allocations: allocation k holds spans k, k + 3, ...,
    span i at phase i % 16 of a 4 KiB-aligned place of its own and of length
    SCATTER_LENS[i % 10].  Span 46 is span 5 again (one buffer listed twice),
    span 47 starts one byte into span 7 (4096 bytes: they overlap).  The last
    span of allocation 2 ends with the allocation's last byte.  The test orders
    the pointers descending once it knows where the allocations lie."""
    rng = np.random.default_rng(48)
    n = 48
    where = np.arange(n) % 3
    lens = np.array([SCATTER_LENS[i % 10] for i in range(n)], np.uint32)
    offs = (np.arange(n) // 3 * 8192 + np.arange(n) % 16).astype(np.uint64)
    where[46], offs[46], lens[46] = where[5], offs[5], lens[5]
    assert lens[7] == 4096
    where[47], offs[47], lens[47] = where[7], offs[7] + 1, 4096
    sizes = [int((offs[where == k].astype(np.int64) + lens[where == k]).max()) for k in range(3)]
    bufs = [_ro(rng.integers(0, 256, s + (64 if k < 2 else 0), dtype=np.uint8)) for k, s in enumerate(sizes)]
    ends = offs[where == 2].astype(np.int64) + lens[where == 2]
    assert ends.max() == bufs[2].size and sorted(set((offs % 16).tolist())) == list(range(16))
    assert set(SCATTER_LENS) <= set(lens.tolist())
    # chains over them, empty ones among them, iovs of different allocations in each
    first = np.array([0, 0, 5, 5, 6, 30, 48, 48], np.uint64)
    return Case("scattered", bufs, where, offs, lens, 0, None, first)

"""Cases and the reference for crc32c_batch_chains (no GPU here).

A case is one call's descriptors in host memory: the buffer, the iovs in
either form of crc32c_spans (offsets[] or a stride, lens[] or one length) and
chain_first.  expected_chains is the reference's own definition
(storage.c:163-170: crc = crc32c(crc, iov) over the chain's iovs, from 0) run
through the oracle round by round; tests/test_chain_model.py checks it against
the CRC of the concatenated bytes and against the combine fold the kernel uses,
tests/test_gpu_chains.py runs the library on the same cases.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from . import oracle

PATTERN = (0, 1, 2, 7)  # iovs per chain, repeated: 10 iovs per 4 chains


@dataclass
class Case:
    name: str
    buf: np.ndarray            # uint8
    first: np.ndarray          # uint64, nchains + 1 entries
    n: int                     # iovs
    offsets: np.ndarray | None = None  # uint64; None: iov i at i * stride
    stride: int = 0
    lens: np.ndarray | None = None     # uint32; None: every iov `length` bytes
    length: int = 0            # with lens given: a decoy the library must ignore
    small_max: int | None = None  # crc32c_set_small_max for the call (None: leave it)
    route: str = ""            # the span route the device call takes (for the reader)

    @property
    def nchains(self) -> int:
        return self.first.size - 1

    def iov_offsets(self) -> np.ndarray:
        if self.offsets is not None:
            return self.offsets
        return np.arange(self.n, dtype=np.uint64) * np.uint64(self.stride)

    def iov_lens(self) -> np.ndarray:
        if self.lens is not None:
            return self.lens.astype(np.uint64)
        return np.full(self.n, self.length, np.uint64)


def expected_iovs(case: Case) -> np.ndarray:
    """iovs->out: each iov's own CRC from 0."""
    return oracle.batch(case.buf, case.iov_offsets(), case.iov_lens())


def expected_chains(buf, offs, lens, first) -> np.ndarray:
    """out[c] = crc32c(...crc32c(crc32c(0, iov_a), iov_a+1)..., iov_b-1) for chain
    c = iovs [first[c], first[c+1]); a chain of no iovs gives 0.  Round k feeds
    every chain that has more than k iovs its k-th iov with crc_in = its value
    so far."""
    first = np.asarray(first).astype(np.int64)
    offs = np.asarray(offs, np.uint64)
    lens = np.asarray(lens, np.uint64)
    counts = np.diff(first)
    assert (counts >= 0).all() and (first.size == 1 or first[-1] <= offs.size)
    crc = np.zeros(counts.size, np.uint32)
    for k in range(int(counts.max(initial=0))):
        live = np.flatnonzero(counts > k)
        idx = first[live] + k
        crc[live] = oracle.batch(buf, offs[idx], lens[idx], crc_in=crc[live])
    return crc


def expected(case: Case) -> np.ndarray:
    return expected_chains(case.buf, case.iov_offsets(), case.iov_lens(), case.first)


def zero_crc_bytes(crc_in: int = 0) -> bytes:
    """The four bytes m with crc32c(crc_in, m) == 0.  crc32c(crc_in, m) is affine
    in the 32 bits of m over GF(2): f(m) = f(0) ^ L(m) with L linear and
    invertible, so L(m) = f(0) is a 32 x 32 system, solved here by elimination
    on the columns L(e_j) that the oracle gives."""
    def f(m: int) -> int:
        return oracle.crc32c(crc_in, int(m).to_bytes(4, "little"))
    f0 = f(0)
    # rows: [L(e_j) | e_j]; reduce to a basis indexed by leading bit
    basis = {}
    for j in range(32):
        v, tag = f(1 << j) ^ f0, 1 << j
        while v:
            top = v.bit_length() - 1
            if top not in basis:
                basis[top] = (v, tag)
                break
            bv, bt = basis[top]
            v, tag = v ^ bv, tag ^ bt
        assert v, "L is not invertible"
    target, m = f0, 0
    while target:
        bv, bt = basis[target.bit_length() - 1]
        target, m = target ^ bv, m ^ bt
    out = m.to_bytes(4, "little")
    assert oracle.crc32c(crc_in, out) == 0
    return out


def _first_of(counts) -> np.ndarray:
    return np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64)


def _pattern_first(n_iovs: int) -> np.ndarray:
    """Chains of 0, 1, 2 and 7 iovs over n_iovs iovs (a multiple of 10), an empty
    chain at the front (the pattern's) and one more at the end."""
    assert n_iovs % sum(PATTERN) == 0
    return _first_of(list(PATTERN) * (n_iovs // sum(PATTERN)) + [0])


def _mixed_offsets(n: int, length: int) -> tuple[np.ndarray, int]:
    """n disjoint iovs of `length` bytes whose starts take n different residues
    mod 128 (37 is odd: i * 37 mod 128 repeats after 128)."""
    pitch = (length + 255) // 128 * 128
    i = np.arange(n, dtype=np.uint64)
    return i * np.uint64(pitch) + (i * np.uint64(37)) % np.uint64(128), n * pitch + 256


def route_cases() -> list[Case]:
    """One case per span route that crc32c_batch_chains can send its iovs
    through; chains of 0, 1, 2 and 7 iovs in each."""
    cases = []
    rng = np.random.default_rng(163)
    # lens[]: the single-launch kernel, and the same batch planned.  Offsets in
    # random order (chain order is not memory order: the host path permutes).
    n = 600
    buf = rng.integers(0, 256, 1 << 20, dtype=np.uint8)
    lens = rng.integers(0, 3000, n).astype(np.uint32)
    lens[:8] = [0, 1, 1023, 1024, 1025, 15, 16, 17]
    lens = rng.permutation(lens)
    offs = rng.integers(0, buf.size - 3000, n).astype(np.uint64)
    for name, sm in (("lens_small", None), ("lens_planned", 0)):
        cases.append(Case(name, buf, _pattern_first(n), n, offsets=offs, lens=lens, length=12345, small_max=sm,
                          route="small" if sm is None else "planned"))
    n = 60
    # K1: equal 4096-B iovs at a 16-B aligned stride, no offsets, no lens
    stride = 4096 + 16
    buf = rng.integers(0, 256, n * stride, dtype=np.uint8)
    cases.append(Case("fixed4096_k1", buf, _pattern_first(n), n, stride=stride, length=4096, route="k1"))
    for length, route in ((4133, "k5"), (4090, "id_blocks"), (9000, "id_spans"), (100, "id_final")):
        offs, size = _mixed_offsets(n, length)
        buf = rng.integers(0, 256, size, dtype=np.uint8)
        cases.append(Case(f"fixed{length}_{route}", buf, _pattern_first(n), n, offsets=offs, length=length,
                          small_max=0, route=route))
    # the same two kernels taking the iovs by stride (k_lines<0, false>, k_blocks<true, false>): the extstore
    # image shape, a span at +32 of every 4165-byte image, and 4097-byte iovs that overlap by a byte
    for length, stride, route in ((4133, 4165, "k5"), (4097, 4096, "id_blocks")):
        buf = rng.integers(0, 256, (n - 1) * stride + length, dtype=np.uint8)
        cases.append(Case(f"fixed{length}_{route}_stride", buf, _pattern_first(n), n, stride=stride, length=length,
                          small_max=0, route=route))
    return cases


def zero_cases() -> list[Case]:
    """Zero-length iovs at the start, the end and all through a chain, empty
    chains at the front, in the middle and at the end of chain_first, and chains
    whose running value is exactly 0 in mid-chain: after a first iov that is
    zero_crc_bytes(), and after a second iov made to cancel the first's CRC."""
    rng = np.random.default_rng(170)
    buf = rng.integers(0, 256, 1 << 16, dtype=np.uint8)
    zc = zero_crc_bytes()
    buf[1001:1005] = np.frombuffer(zc, np.uint8)
    a, b, c = (5000, 777), (9003, 1024), (20011, 4097)
    zc_iov = (1001, 4)
    cancel = zero_crc_bytes(oracle.crc32c(0, buf[a[0]:a[0] + a[1]]))  # crc32c(crc(a), cancel) == 0
    buf[3003:3007] = np.frombuffer(cancel, np.uint8)
    cancel_iov = (3003, 4)
    z = lambda o: (o, 0)  # noqa: E731  (a zero-length iov at offset o)
    chains = [
        [],                                  # empty, at the front
        [z(0), a, b],                        # begins with a zero-length iov
        [a, b, z(buf.size)],                 # ends with one (at the buffer's very end)
        [z(7), z(7), z(65535)],              # only zero-length iovs
        [z(123)],
        [],                                  # empty, in the middle
        [zc_iov, a, b, c],                   # the running value is 0 after the first iov
        [zc_iov],                            # a chain whose CRC is 0
        [zc_iov, z(9), a],                   # 0, then a zero-length iov
        [zc_iov, zc_iov, b],                 # 0 twice
        [a, cancel_iov, b, c],               # 0 after the second iov
        [a, cancel_iov],                     # ends on 0
        [a, b],
        [], [],                              # empty, at the end
    ]
    flat = [iov for ch in chains for iov in ch]
    offs = np.array([o for o, _ in flat], np.uint64)
    lens = np.array([n for _, n in flat], np.uint32)
    first = _first_of([len(ch) for ch in chains])
    cases = [Case("zeros_lens", buf, first, len(flat), offsets=offs, lens=lens, route="small"),
             Case("zeros_lens_planned", buf, first, len(flat), offsets=offs, lens=lens, small_max=0, route="planned")]
    # every iov empty through the fixed-length form (lens == NULL, len == 0)
    cases.append(Case("zeros_fixed_len0", buf, _pattern_first(20), 20, stride=16, length=0, route="small"))
    return cases


DIGIT_LENS = (1023, 1024, 1025, (1 << 20) - 1, 1 << 20, (1 << 20) + 1, 3 * (1 << 20) + 5)


def digit_case() -> Case:
    """The fold multiplies the running value by x^(8 len) from a table of
    base-1024 digits of len: every digit boundary as the *second* iov's length
    (the first iov's CRC is what gets shifted), and as the middle one of three.
    Overlapping iovs in a 4 MiB buffer.  (The 2^30 digit needs an iov of 1 GiB:
    test_maximum_length_spans reaches it in xpow8_dev through crc_in.)"""
    rng = np.random.default_rng(1 << 20)
    buf = rng.integers(0, 256, 4 << 20, dtype=np.uint8)
    chains = []
    for k, length in enumerate(DIGIT_LENS):
        head, tail = (13 + 1000 * k, 900 + k), (77 + 5000 * k, 333 + k)
        big = (int(rng.integers(0, buf.size - length)), length)
        chains += [[head, big], [head, big, tail]]
    flat = [iov for ch in chains for iov in ch]
    return Case("digits", buf, _first_of([len(ch) for ch in chains]), len(flat),
                offsets=np.array([o for o, _ in flat], np.uint64), lens=np.array([n for _, n in flat], np.uint32),
                route="small")


MILLION_CHAINS = 1048577 + 300  # k_chain's grid is capped at 4096 x 256 threads: its loop's second trip


def million_case() -> Case:
    """More chains than k_chain has threads, and more iovs than one pipeline slot
    of the host path holds (2^20): 0-2 iovs of 0-40 bytes over 64 KiB."""
    rng = np.random.default_rng(4096 * 256)
    buf = rng.integers(0, 256, 1 << 16, dtype=np.uint8)
    counts = rng.choice(3, MILLION_CHAINS, p=[0.25, 0.4, 0.35])
    counts[-301:] = np.resize([1, 2, 0, 2], 301)  # the second trip's chains: every count
    first = _first_of(counts)
    n = int(first[-1])
    assert n > 1 << 20
    lens = rng.integers(0, 41, n).astype(np.uint32)
    offs = rng.integers(0, buf.size - 40, n).astype(np.uint64)
    return Case("million", buf, first, n, offsets=offs, lens=lens, route="planned")


def range_case() -> tuple[Case, int, int]:
    """(case, bad, base_bytes): iov `bad` ends past base_bytes (the buffer itself
    is longer, and no other iov touches those bytes)."""
    rng = np.random.default_rng(5)
    n = 40
    buf = rng.integers(0, 256, 1 << 16, dtype=np.uint8)
    base_bytes = buf.size - 4096
    lens = rng.integers(1, 2000, n).astype(np.uint32)
    offs = rng.integers(0, base_bytes - 4000, n).astype(np.uint64)
    bad = 23
    offs[bad], lens[bad] = base_bytes - 10, 100
    return Case("range", buf, _pattern_first(n), n, offsets=offs, lens=lens, route="small"), bad, base_bytes


def small_cases() -> list[Case]:
    """Every case the CPU model check walks chain by chain."""
    return route_cases() + zero_cases() + [digit_case(), range_case()[0]]

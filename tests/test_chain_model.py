"""tests/chain_cases.py checked on the CPU: expected_chains (the oracle chained
through crc_in, round by round) equals the CRC of each chain's concatenated
bytes, and equals the fold k_chain computes, acc = combine(acc, crc_i, len_i)
over the iovs' own CRCs; the generated cases have the shapes their names
promise.  So what the GPU tests compare against is itself pinned here."""
import numpy as np
import pytest

from . import chain_cases as cc
from . import oracle

SMALL = cc.small_cases()


class _Walk:
    """One case's chains, iov by iov (the arrays expanded once)."""

    def __init__(self, case):
        self.case, self.offs, self.lens = case, case.iov_offsets(), case.iov_lens()
        self.iov_crc = cc.expected_iovs(case)

    def iovs(self, c):
        return range(int(self.case.first[c]), int(self.case.first[c + 1]))

    def by_concatenation(self, c):
        parts = [self.case.buf[int(self.offs[i]):int(self.offs[i]) + int(self.lens[i])] for i in self.iovs(c)]
        return oracle.crc32c(0, np.concatenate(parts) if parts else b"")

    def by_fold(self, c):
        acc = 0
        for i in self.iovs(c):
            acc = int(oracle.lib().oracle_crc32c_combine(acc, int(self.iov_crc[i]), int(self.lens[i])))
        return acc


@pytest.mark.parametrize("case", SMALL, ids=[c.name for c in SMALL])
def test_expected_chains_equals_concatenation_and_fold(case):
    want = cc.expected(case)
    w = _Walk(case)
    assert want.dtype == np.uint32 and want.shape == (case.nchains,) and w.iov_crc.shape == (case.n,)
    for c in range(case.nchains):
        assert int(want[c]) == w.by_concatenation(c), (case.name, c)
        assert int(want[c]) == w.by_fold(c), (case.name, c)


def test_million_case_shape_and_sampled_chains():
    """More chains than k_chain's 4096 x 256 threads, more iovs than a host
    pipeline slot, every count among the loop's second-trip chains; expected
    against concatenation and fold on a sample and on the whole second trip."""
    case = cc.million_case()
    assert case.nchains == 1048577 + 300 and case.n > 1 << 20
    counts = np.diff(case.first.astype(np.int64))
    assert counts.min() == 0 and counts.max() == 2
    assert set(counts[4096 * 256:].tolist()) == {0, 1, 2}
    assert case.iov_lens().max() == 40 and case.iov_lens().min() == 0
    assert int((case.iov_offsets() + case.iov_lens()).max()) <= case.buf.size
    want = cc.expected(case)
    w = _Walk(case)
    sample = np.random.default_rng(1).choice(4096 * 256, 3000, replace=False).tolist()
    for c in sample + list(range(4096 * 256, case.nchains)):
        assert int(want[c]) == w.by_concatenation(c) == w.by_fold(c), c


def test_zero_crc_bytes():
    m = cc.zero_crc_bytes()
    assert len(m) == 4 and oracle.crc32c(0, m) == 0 and oracle.crc32c_bitwise(0, m) == 0
    for cin in (1, 0xdeadbeef, 0xffffffff):
        assert oracle.crc32c(cin, cc.zero_crc_bytes(cin)) == 0


def test_zero_cases_hold_what_they_promise():
    case = cc.zero_cases()[0]
    counts = np.diff(case.first.astype(np.int64)).tolist()
    assert counts[0] == 0 and counts[-1] == 0 and 0 in counts[1:-2]
    iov_crc = cc.expected_iovs(case)
    lens = case.iov_lens()
    zero_mid = only_empty = 0
    for c in range(case.nchains):
        lo, hi = int(case.first[c]), int(case.first[c + 1])
        only_empty += hi > lo and not lens[lo:hi].any()
        acc = 0
        for i in range(lo, hi):
            acc = int(oracle.lib().oracle_crc32c_combine(acc, int(iov_crc[i]), int(lens[i])))
            zero_mid += acc == 0 and lens[i] != 0 and i + 1 < hi  # 0 with iovs still to come
    assert zero_mid >= 3 and only_empty >= 2
    assert lens[int(case.first[1])] == 0 and lens[int(case.first[3]) - 1] == 0  # a chain begins / ends with one


def test_route_and_digit_cases_have_their_shapes():
    by_name = {c.name: c for c in cc.route_cases()}
    assert set(by_name) == {"lens_small", "lens_planned", "fixed4096_k1", "fixed4133_k5", "fixed4090_id_blocks",
                            "fixed9000_id_spans", "fixed100_id_final", "fixed4133_k5_stride",
                            "fixed4097_id_blocks_stride"}
    for name in ("fixed4133_k5_stride", "fixed4097_id_blocks_stride"):
        c = by_name[name]
        assert c.offsets is None and c.lens is None and c.small_max == 0
        assert c.buf.size == (c.n - 1) * c.stride + c.length  # (the smallest buffer the library accepts)
    for c in by_name.values():
        counts = set(np.diff(c.first.astype(np.int64)).tolist())
        assert counts == {0, 1, 2, 7}, c.name
        assert int((c.iov_offsets() + c.iov_lens()).max()) <= c.buf.size
        if c.name.startswith("fixed") and c.offsets is not None:
            assert len(set((c.offsets % 128).tolist())) == c.n  # mixed alignments mod 128
            assert c.small_max == 0 and c.lens is None
    k1 = by_name["fixed4096_k1"]
    assert k1.offsets is None and k1.lens is None and k1.stride % 16 == 0 and k1.length == 4096
    assert by_name["lens_small"].buf.size <= 8 << 20 and by_name["lens_small"].n <= 8192
    d = cc.digit_case()
    second = [int(d.iov_lens()[int(f) + 1]) for f in d.first[:-1]]
    assert set(second) == set(cc.DIGIT_LENS)
    case, bad, base_bytes = cc.range_case()
    offs, lens = case.iov_offsets().astype(np.int64), case.iov_lens().astype(np.int64)
    ends = offs + lens
    assert ends[bad] > base_bytes and (np.delete(ends, bad) <= offs[bad]).all()  # alone out of range, overlapped by none

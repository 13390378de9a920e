"""crc32c_batch_chains through the C ABI (ctypes, so `len`, `stride` and
iovs->out are reachable) on the cases of tests/chain_cases.py: every span route
under the fold, fixed-length iovs, each iov's own CRC, empty and zero-valued
chains, the fold's length digits, more chains than k_chain has threads, a
caller's stream, and the return codes.  Device path, and host path over
pageable and page-locked buffers.  Bit-exact against the oracle
(chain_cases.expected_chains, itself checked by tests/test_chain_model.py)."""
import ctypes
import time

import numpy as np
import pytest

try:  # GPU processes load torch (and its HIP runtime) before libmcrc32c.so
    import torch as _torch  # noqa: F401
except ImportError:
    pass

from memcached_amd import _lib

from . import chain_cases as cc
from . import raw_calls

pytestmark = pytest.mark.gpu

SENT = 0x5A5A5A5A  # what every output array holds before a call
WHERE = ("device", "host", "pinned")


@pytest.fixture(scope="module")
def torch():
    return raw_calls.need_gpu()


_want = {}


def _expected(case):
    """(iovs' CRCs, chains' CRCs) of a case: computed once, shared, read-only."""
    if case.name not in _want:
        pair = (cc.expected_iovs(case), cc.expected(case))
        for a in pair:
            a.setflags(write=False)
        _want[case.name] = pair
    return _want[case.name]


def _dev(torch, a, view):
    return None if a is None else torch.from_numpy(a.view(view)).cuda()


def _ptr(x):
    if x is None:
        return None
    return x.data_ptr() if hasattr(x, "data_ptr") else x.ctypes.data


def _run(torch, case, where, *, base_bytes=None, first=None, nchains=None, crc_in=False, null_first=False,
         null_out=False, flags=0, stream=None):
    """One crc32c_batch_chains call over `case`; returns (rc, iovs->out, out),
    both prefilled with SENT.  `first` / `nchains` / `base_bytes` override the
    case's; crc_in, null_first and null_out build the calls that must be refused."""
    n = case.n
    first = case.first if first is None else first
    nchains = first.size - 1 if nchains is None else nchains
    base_bytes = case.buf.size if base_bytes is None else base_bytes
    nout = max(first.size - 1, 1)
    keep = []  # (everything the call reads stays referenced until it returns)
    if where == "device":
        buf = torch.from_numpy(case.buf).cuda()
        offs, lens = _dev(torch, case.offsets, np.int64), _dev(torch, case.lens, np.int32)
        dfirst = _dev(torch, first, np.int64)
        iov_out = torch.full((max(n, 1),), SENT, dtype=torch.int32, device="cuda")
        out = torch.full((nout,), SENT, dtype=torch.int32, device="cuda")
        cin = torch.zeros(max(n, 1), dtype=torch.int32, device="cuda") if crc_in else None
        torch.cuda.synchronize()
        flags |= _lib.CRC32C_DEVICE
        if stream is None:
            stream = torch.cuda.current_stream().cuda_stream
    else:
        buf = torch.from_numpy(case.buf).pin_memory() if where == "pinned" else case.buf
        offs, lens, dfirst = case.offsets, case.lens, first
        iov_out = np.full(max(n, 1), SENT, np.uint32)
        out = np.full(nout, SENT, np.uint32)
        cin = np.zeros(max(n, 1), np.uint32) if crc_in else None
        stream = None
    keep += [buf, offs, lens, dfirst, cin]
    sp = _lib.Spans(_ptr(buf), base_bytes, _ptr(offs), case.stride, _ptr(lens), case.length, _ptr(cin),
                    _ptr(iov_out), n)
    with raw_calls.small_max(case.small_max):
        rc = _lib.lib.crc32c_batch_chains(ctypes.byref(sp), None if null_first else _ptr(dfirst), nchains,
                                          None if null_out else _ptr(out), flags, stream)
    if where == "device":
        torch.cuda.synchronize()
        iov_out, out = iov_out.cpu().numpy().view(np.uint32), out.cpu().numpy().view(np.uint32)
    del keep
    return rc, iov_out[:n], out[:first.size - 1]


def _check_exact(torch, case, where):
    want_iov, want = _expected(case)
    rc, iov_out, out = _run(torch, case, where)
    assert rc == _lib.CRC32C_OK, (case.name, where, rc)
    np.testing.assert_array_equal(iov_out, want_iov, err_msg=f"{case.name} {where}: iovs->out")
    np.testing.assert_array_equal(out, want, err_msg=f"{case.name} {where}: chains")


ROUTES = cc.route_cases()
ZEROS = cc.zero_cases()


@pytest.mark.parametrize("where", WHERE)
@pytest.mark.parametrize("case", ROUTES, ids=[c.name for c in ROUTES])
def test_every_span_route_under_the_fold(torch, case, where):
    """The iovs go through k_small, the planned path, K1, K5, k_blocks, k_spans
    or k_final alone (device path; the host path stages them with offsets, so
    its K1 case runs the small route); chains of 0, 1, 2 and 7 iovs; lens[]
    given (with a decoy `len` the library must ignore) or NULL.  Each iov's own
    CRC and every chain's."""
    _check_exact(torch, case, where)


@pytest.mark.parametrize("where", WHERE)
@pytest.mark.parametrize("case", ZEROS, ids=[c.name for c in ZEROS])
def test_zero_length_iovs_empty_chains_and_zero_running_values(torch, case, where):
    """Chains that begin with, end with and consist of zero-length iovs, empty
    chains at the front, middle and end, and a running value of exactly 0 in
    mid-chain (k_chain skips the multiply there)."""
    _check_exact(torch, case, where)


@pytest.mark.parametrize("where", ["device", "host"])
def test_no_chains_is_ok_and_writes_nothing(torch, where):
    case = ZEROS[0]
    rc, _, _ = _run(torch, case, where, nchains=0)
    assert rc == _lib.CRC32C_OK
    # (out as the call saw it: one chain's room, still the fill)
    rc, _, out = _run(torch, case, where, first=case.first[:2].copy(), nchains=0)
    assert rc == _lib.CRC32C_OK and out.tolist() == [SENT]


@pytest.mark.parametrize("where", WHERE)
def test_fold_length_digits(torch, where):
    """The second iov's length at every boundary of the x^(8 len) table's
    base-1024 digits below 2^30 (1023 .. 3 * 2^20 + 5).  An iov of 2^30 bytes or
    more (the table's last digit) would need a 1 GiB buffer per chain:
    test_maximum_length_spans reaches that digit of xpow8_dev through crc_in."""
    _check_exact(torch, cc.digit_case(), where)


@pytest.mark.parametrize("where", WHERE)
def test_more_chains_than_k_chain_has_threads(torch, where):
    """1 048 877 chains: k_chain's grid-stride loop makes a second trip; about
    1.15 M iovs: the host path crosses a pipeline slot (2^20 items)."""
    t0 = time.perf_counter()
    case = cc.million_case()
    want_iov, want = _expected(case)
    t1 = time.perf_counter()
    rc, iov_out, out = _run(torch, case, where)
    t2 = time.perf_counter()
    print(f"\nmillion chains [{where}]: case, and the oracle on first use, {(t1 - t0) * 1e3:.0f} ms, "
          f"library call with its copies {(t2 - t1) * 1e3:.0f} ms")
    assert rc == _lib.CRC32C_OK
    assert np.array_equal(iov_out, want_iov)
    bad = np.flatnonzero(out != want)
    assert bad.size == 0, (bad.size, bad[:5].tolist(), bad[-5:].tolist())


def test_async_on_a_callers_stream(torch):
    """CRC32C_DEVICE | CRC32C_ASYNC on a stream that is not the default one: the
    buffer and the descriptors arrive by copies enqueued on that stream, the
    results are read after stream.synchronize()."""
    st = torch.cuda.Stream()
    for case in ROUTES[:2] + [cc.digit_case()]:
        want_iov, want = _expected(case)
        pins = [torch.from_numpy(a).pin_memory() for a in
                (case.buf, case.offsets.view(np.int64), case.lens.view(np.int32), case.first.view(np.int64))]
        with torch.cuda.stream(st):
            buf, offs, lens, first = (p.to("cuda", non_blocking=True) for p in pins)
            iov_out = torch.full((case.n,), SENT, dtype=torch.int32, device="cuda")
            out = torch.full((case.nchains,), SENT, dtype=torch.int32, device="cuda")
            sp = _lib.Spans(buf.data_ptr(), case.buf.size, offs.data_ptr(), 0, lens.data_ptr(), case.length, None,
                            iov_out.data_ptr(), case.n)
            with raw_calls.small_max(case.small_max):
                rc = _lib.lib.crc32c_batch_chains(ctypes.byref(sp), first.data_ptr(), case.nchains, out.data_ptr(),
                                                  _lib.CRC32C_DEVICE | _lib.CRC32C_ASYNC,
                                                  ctypes.c_void_p(st.cuda_stream))
        assert rc == _lib.CRC32C_OK, case.name
        st.synchronize()
        np.testing.assert_array_equal(iov_out.cpu().numpy().view(np.uint32), want_iov, err_msg=case.name)
        np.testing.assert_array_equal(out.cpu().numpy().view(np.uint32), want, err_msg=case.name)


@pytest.mark.parametrize("small_max", [None, 0], ids=["small", "planned"])
def test_out_of_range_iov(torch, small_max):
    """One iov ends past base_bytes.  Device: CRC32C_ERANGE, that iov is not read
    and its out is 0, every other iov and every chain without it exact (the chain
    that holds it has an unspecified value).  Host: the batch is refused whole,
    CRC32C_EINVAL, nothing written."""
    case, bad, base_bytes = cc.range_case()
    case.small_max = small_max
    want_iov, want = _expected(case)
    rc, iov_out, out = _run(torch, case, "device", base_bytes=base_bytes)
    assert rc == _lib.CRC32C_ERANGE
    assert iov_out[bad] == 0
    np.testing.assert_array_equal(np.delete(iov_out, bad), np.delete(want_iov, bad))
    holder = int(np.searchsorted(case.first, bad, side="right")) - 1
    assert case.first[holder] <= bad < case.first[holder + 1]
    np.testing.assert_array_equal(np.delete(out, holder), np.delete(want, holder))
    for where in ("host", "pinned"):
        rc, iov_out, out = _run(torch, case, where, base_bytes=base_bytes)
        assert rc == _lib.CRC32C_EINVAL, where
        assert (iov_out == SENT).all() and (out == SENT).all(), where


def test_refused_arguments(torch):
    """CRC32C_EINVAL and nothing written: crc_in given, chain_first NULL, chains
    without an out, and on the host path a chain_first that descends or runs past
    the iovs.  (On the device path chain_first is device memory and is not
    validated: see include/crc32c_batch.h.)"""
    case = ROUTES[0]
    for where in ("device", "host"):
        for kw in ({"crc_in": True}, {"null_first": True}, {"null_out": True}):
            rc, iov_out, out = _run(torch, case, where, **kw)
            assert rc == _lib.CRC32C_EINVAL, (where, kw)
            assert (iov_out == SENT).all() and (out == SENT).all(), (where, kw)
    descending = case.first.copy()
    descending[5], descending[6] = descending[6], descending[5]
    assert descending[6] < descending[5]
    past = case.first.copy()
    past[-1] = case.n + 1
    for first in (descending, past):
        for where in ("host", "pinned"):
            rc, iov_out, out = _run(torch, case, where, first=first)
            assert rc == _lib.CRC32C_EINVAL, where
            assert (iov_out == SENT).all() and (out == SENT).all(), where

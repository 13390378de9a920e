"""crc32c_batch_ptrs, crc32c_ptrs_submit and crc32c_chains_ptrs on the GPU:
the cases of tests/ptr_cases.py with their allocations in device, pageable and
page-locked memory and mixed between the two host kinds.  Every output array is
pre-filled with a sentinel and checked behind its end; every expected value is
the oracle's and, for a re-expressed case, also what crc32c_batch or
crc32c_batch_chains returns for its offsets form: all comparisons are exact."""
import contextlib
import ctypes
import threading

import numpy as np
import pytest

try:  # GPU processes load torch (and its HIP runtime) before libmcrc32c.so
    import torch as _torch  # noqa: F401
except ImportError:
    pass

from memcached_amd import _lib
from memcached_amd import crc32c as mc

from . import oracle
from . import ptr_cases as pc
from . import raw_calls as raw

pytestmark = pytest.mark.gpu
SENT = raw.SENT[4]
PAD = raw.EXTRA
SIDES = ("device", "pageable", "pinned", "mixed")
MAX_SPAN = _lib.CRC32C_MAX_SPAN


@pytest.fixture(scope="module")
def torch():
    return raw.need_gpu()


def _t(torch, a):
    """A numpy array as a device tensor of the signed type of its width."""
    signed = {"uint64": np.int64, "uint32": np.int32}.get(a.dtype.name)
    return torch.from_numpy(np.array(a.view(signed) if signed else a)).cuda()


class Placed:
    """A case's allocations on one side, alive for a with block; bases[k][i]:
    where span i finds allocation k (mixed: even spans in page-locked copies,
    odd ones in pageable copies)."""

    def __init__(self, torch, bufs, side):
        self.torch, self.side, self.dev = torch, side, side == "device"
        self._stack = contextlib.ExitStack()
        self._keep = []
        kinds = {"device": ("device",), "pageable": ("pageable",), "pinned": ("pinned",),
                 "mixed": ("pinned", "pageable")}[side]
        self.addr = [np.array([self._place(b, kind) for b in bufs], np.uint64) for kind in kinds]

    def _place(self, buf, kind):
        if kind == "device":
            t = self.torch.from_numpy(np.array(buf)).cuda()
            self._keep.append(t)
            return t.data_ptr() if buf.size else 0
        a = self._stack.enter_context(raw.pinned(buf.size)) if kind == "pinned" else np.empty(buf.size, np.uint8)
        a[:] = buf
        self._keep.append(a)
        return a.ctypes.data if buf.size else 0

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        if self.dev:
            self.torch.cuda.synchronize()
        return self._stack.__exit__(*exc)

    def ptrs(self, where, offs, lens):
        """ptrs[i] = the base of span i's allocation + offs[i]; NULL for a span
        of no bytes in an allocation of none."""
        i = np.arange(offs.size)
        base = self.addr[0][where] if len(self.addr) == 1 else np.where(i % 2 == 0, self.addr[0][where],
                                                                        self.addr[1][where])
        return np.where((base == 0) & (lens == 0), 0, base + offs).astype(np.uint64)

    def desc(self, a):
        if a is None:
            return None
        return _t(self.torch, a) if self.dev else np.ascontiguousarray(a)

    def out(self, n):
        if self.dev:
            return self.torch.full((n + PAD,), SENT, dtype=self.torch.int32, device="cuda")
        return np.full(n + PAD, SENT, np.uint32)

    def host(self, x):
        return x.cpu().numpy().view(np.uint32) if self.dev else x

    def opts(self, asynchronous=False):
        mode = (_lib.CRC32C_DEVICE if self.dev else 0) | (_lib.CRC32C_ASYNC if asynchronous else 0)
        stream = self.torch.cuda.current_stream().cuda_stream if self.dev else None
        return _lib.PtrOpts(mode, stream)


def call_ptrs(pl, ptrs, lens, length, cin, small_max=None, asynchronous=False):
    """One crc32c_batch_ptrs: (rc, out[:n]); the sentinel behind out's end is asserted."""
    n = ptrs.size
    dp, dl, dc, out = pl.desc(ptrs), pl.desc(lens), pl.desc(cin), pl.out(n)
    b = _lib.PtrBatch(raw.ptr(dp), raw.ptr(dl), length, raw.ptr(dc), raw.ptr(out), n)
    opts = pl.opts(asynchronous)
    with raw.small_max(small_max):
        rc = _lib.lib.crc32c_batch_ptrs(ctypes.byref(b), ctypes.byref(opts))
    if pl.dev:
        pl.torch.cuda.synchronize()
    got = pl.host(out)
    assert (got[n:] == SENT).all(), "written behind out[n]"
    return rc, got[:n]


def call_chains(pl, ptrs, lens, length, first, small_max=None):
    """One crc32c_chains_ptrs: (rc, iovs->out[:n], out[:nchains])."""
    n, nchains = ptrs.size, first.size - 1
    dp, dl, df, iov_out, out = pl.desc(ptrs), pl.desc(lens), pl.desc(first), pl.out(n), pl.out(nchains)
    b = _lib.PtrBatch(raw.ptr(dp), raw.ptr(dl), length, None, raw.ptr(iov_out), n)
    opts = pl.opts()
    with raw.small_max(small_max):
        rc = _lib.lib.crc32c_chains_ptrs(ctypes.byref(b), raw.ptr(df), nchains, raw.ptr(out), ctypes.byref(opts))
    if pl.dev:
        pl.torch.cuda.synchronize()
    gi, go = pl.host(iov_out), pl.host(out)
    assert (gi[n:] == SENT).all() and (go[nchains:] == SENT).all(), "written behind an output's end"
    return rc, gi[:n], go[:nchains]


def _lens32(case):
    return None if case.lens is None else np.ascontiguousarray(case.lens, np.uint32)


def _offsets_form(torch, case, cin, first=None):
    """What crc32c_batch (or crc32c_batch_chains) returns for the case's one
    buffer in its offsets form, on the device."""
    buf = _t(torch, np.concatenate((case.bufs[0], np.zeros(16, np.uint8))))  # (an empty buffer still has an address)
    offs, lens, dcin = _t(torch, case.offs), None if case.lens is None else _t(torch, _lens32(case)), \
        None if cin is None else _t(torch, cin)
    out = torch.full((case.n + PAD,), SENT, dtype=torch.int32, device="cuda")
    sp = _lib.Spans(buf.data_ptr(), case.bufs[0].size, offs.data_ptr(), 0, raw.ptr(lens), case.length, raw.ptr(dcin),
                    out.data_ptr(), case.n)
    with raw.small_max(case.small_max):
        if first is None:
            rc = _lib.lib.crc32c_batch(ctypes.byref(sp), _lib.CRC32C_DEVICE, None)
            res = out
        else:
            res = torch.full((first.size - 1 + PAD,), SENT, dtype=torch.int32, device="cuda")
            rc = _lib.lib.crc32c_batch_chains(ctypes.byref(sp), _t(torch, first).data_ptr(), first.size - 1,
                                              res.data_ptr(), _lib.CRC32C_DEVICE, None)
    torch.cuda.synchronize()
    assert rc == _lib.CRC32C_OK
    return res.cpu().numpy().view(np.uint32)[:res.numel() - PAD]


# ---------------------------------------------------------------------------
# equality with the offsets call
# ---------------------------------------------------------------------------
SPAN_CASES = pc.span_cases()


@pytest.mark.parametrize("case", SPAN_CASES, ids=[c.name for c in SPAN_CASES])
def test_span_cases_equal_the_offsets_call(torch, case):
    """Every re-expressed span case, on every side, from 0 and from crc_in:
    what crc32c_batch returns for base + offsets, which is the oracle's."""
    for cin in (None, case.crc_in):
        ref = _offsets_form(torch, case, cin)
        np.testing.assert_array_equal(ref, case.expected(cin is not None))
        for side in SIDES:
            with Placed(torch, case.bufs, side) as pl:
                ptrs = pl.ptrs(case.where, case.offs, case.span_lens())
                rc, got = call_ptrs(pl, ptrs, _lens32(case), case.length, cin, case.small_max)
            assert rc == _lib.CRC32C_OK, (case.name, side, rc)
            bad = np.flatnonzero(got != ref)
            assert bad.size == 0, (case.name, side, cin is not None, bad.size, bad[:8].tolist())


CHAIN_CASES = pc.chain_cases()


@pytest.mark.parametrize("case", CHAIN_CASES, ids=[c.name for c in CHAIN_CASES])
def test_chain_cases_equal_the_offsets_call(torch, case):
    """chain_cases' small cases through crc32c_chains_ptrs on the device, the
    pageable and the page-locked side: crc32c_batch_chains' answer, the model's."""
    ref = _offsets_form(torch, case, None, case.first)
    np.testing.assert_array_equal(ref, case.expected_chains())
    for side in ("device", "pageable", "pinned"):
        with Placed(torch, case.bufs, side) as pl:
            ptrs = pl.ptrs(case.where, case.offs, case.span_lens())
            rc, iovs, got = call_chains(pl, ptrs, _lens32(case), case.length, case.first, case.small_max)
        assert rc == _lib.CRC32C_OK, (case.name, side, rc)
        np.testing.assert_array_equal(iovs, case.expected(), err_msg=f"{case.name} {side} iovs->out")
        np.testing.assert_array_equal(got, ref, err_msg=f"{case.name} {side}")


# ---------------------------------------------------------------------------
# scattered spans
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("small_max", [None, 0], ids=["small", "planned"])
@pytest.mark.parametrize("side", SIDES)
def test_scattered_spans(torch, side, small_max):
    """48 spans in three allocations, passed in descending address order, from 0
    and from crc_in; with crc32c_set_small_max(0) through the planned path."""
    case = pc.scattered()
    lens = case.span_lens()
    with Placed(torch, case.bufs, side) as pl:
        ptrs = pl.ptrs(case.where, case.offs, lens)
        order = np.argsort(ptrs, kind="stable")[::-1]
        assert (np.diff(ptrs[order].astype(np.int64)) <= 0).all()
        assert len({int(a) for a in pl.addr[0]}) == 3
        for cin in (None, case.crc_in):
            rc, got = call_ptrs(pl, ptrs[order], _lens32(case)[order], 12345, None if cin is None else cin[order],
                                small_max)
            assert rc == _lib.CRC32C_OK, (side, rc)
            np.testing.assert_array_equal(got, case.expected(cin is not None)[order])
            # the buffer listed twice: the same CRC from 0, each entry's own from its crc_in
            twice = got[np.flatnonzero(order == 46)[0]], got[np.flatnonzero(order == 5)[0]]
            assert (twice[0] == twice[1]) == (cin is None)


@pytest.mark.parametrize("side", ("device", "pageable", "pinned"))
def test_chains_across_allocations(torch, side):
    """Chains whose iovs lie in different allocations, empty chains in front,
    between and behind them."""
    case = pc.scattered()
    assert len(set(case.where[int(case.first[4]):int(case.first[5])].tolist())) == 3
    with Placed(torch, case.bufs, side) as pl:
        ptrs = pl.ptrs(case.where, case.offs, case.span_lens())
        rc, iovs, got = call_chains(pl, ptrs, _lens32(case), 0, case.first)
    assert rc == _lib.CRC32C_OK
    np.testing.assert_array_equal(iovs, case.expected())
    np.testing.assert_array_equal(got, case.expected_chains())
    assert got[0] == 0 and got[2] == 0 and got[6] == 0


# ---------------------------------------------------------------------------
# the rebase's edges (device batches)
# ---------------------------------------------------------------------------
class _Dev:
    """The device side without allocations of its own."""

    def __init__(self, torch):
        self.torch, self.dev = torch, True

    desc, out, host, opts = Placed.desc, Placed.out, Placed.host, Placed.opts


@pytest.mark.parametrize("n", [1, 2, 257, 1025])
@pytest.mark.parametrize("small_max", [None, 0], ids=["small", "routed"])
def test_rebase_sizes(torch, n, small_max):
    """One span; two with the second pointer lower; one past a wave multiple and
    one past a workgroup: spans of 1..300 bytes taken from the buffer's end
    towards its start, with lens[] (the rebase runs) and with one length."""
    rng = np.random.default_rng(n)
    buf = rng.integers(0, 256, 310 * n + 64, dtype=np.uint8)
    lens = rng.integers(1, 301, n).astype(np.uint32)
    offs = (310 * (n - 1 - np.arange(n)) + rng.integers(0, 10, n)).astype(np.uint64)
    t = _t(torch, buf)
    ptrs = (t.data_ptr() + offs).astype(np.uint64)
    assert n == 1 or ptrs[1] < ptrs[0]
    pl = _Dev(torch)
    rc, got = call_ptrs(pl, ptrs, lens, 0, None, small_max)
    assert rc == _lib.CRC32C_OK
    np.testing.assert_array_equal(got, oracle.batch(buf, offs, lens))
    rc, got = call_ptrs(pl, ptrs, None, 77, None, small_max)
    assert rc == _lib.CRC32C_OK
    np.testing.assert_array_equal(got, oracle.batch(buf, offs, np.full(n, 77)))


@pytest.mark.parametrize("small_max", [None, 0], ids=["small", "planned"])
def test_empty_spans_and_null_pointers(torch, small_max):
    """All spans empty with NULL pointers: out = crc_in.  One NULL empty span
    among real ones does not drag the extent's start to 0.  A span that ends at
    its allocation's last byte."""
    pl = _Dev(torch)
    cin = np.array([5, 0, 0xFFFFFFFF, 77], np.uint32)
    for lens, length in ((np.zeros(4, np.uint32), 9), (None, 0)):
        rc, got = call_ptrs(pl, np.zeros(4, np.uint64), lens, length, cin, small_max)
        assert rc == _lib.CRC32C_OK
        np.testing.assert_array_equal(got, cin)
        rc, got = call_ptrs(pl, np.zeros(4, np.uint64), lens, length, None, small_max)
        assert rc == _lib.CRC32C_OK and (got == 0).all()
    rng = np.random.default_rng(3)
    buf = rng.integers(0, 256, 5000, dtype=np.uint8)
    t = _t(torch, buf)
    offs = np.array([100, 0, 5000 - 4097, 4999], np.uint64)
    lens = np.array([300, 0, 4097, 1], np.uint32)
    ptrs = (t.data_ptr() + offs).astype(np.uint64)
    ptrs[1] = 0
    for c in (None, cin):
        rc, got = call_ptrs(pl, ptrs, lens, 0, c, small_max)
        assert rc == _lib.CRC32C_OK
        np.testing.assert_array_equal(got, oracle.batch(buf, offs, lens, c))


def test_spans_more_than_4_gib_apart(torch):
    """Two 4 KiB spans more than 4 GiB apart inside one allocation of which only
    those bytes are written: small by the sum of their lengths, and planned."""
    size = (4 << 30) + (64 << 10)
    big = torch.empty(size, dtype=torch.uint8, device="cuda")
    try:
        rng = np.random.default_rng(4)
        a, b = rng.integers(0, 256, 4096, dtype=np.uint8), rng.integers(0, 256, 4096, dtype=np.uint8)
        far = size - 4096 - 3
        big[5:5 + 4096] = torch.from_numpy(a).cuda()
        big[far:far + 4096] = torch.from_numpy(b).cuda()
        ptrs = np.array([big.data_ptr() + far, big.data_ptr() + 5], np.uint64)
        assert int(ptrs[0] - ptrs[1]) > 1 << 32
        want = np.array([oracle.crc32c(0, b), oracle.crc32c(0, a)], np.uint32)
        pl = _Dev(torch)
        for small_max in (None, 0):
            for lens, length in ((np.full(2, 4096, np.uint32), 0), (None, 4096)):
                rc, got = call_ptrs(pl, ptrs, lens, length, None, small_max)
                assert rc == _lib.CRC32C_OK
                np.testing.assert_array_equal(got, want)
    finally:
        # the 4 GiB segment goes back to the driver: left in torch's cache it would be
        # carved up for every later test's buffers
        del big
        torch.cuda.synchronize()
        torch.cuda.empty_cache()


@pytest.mark.parametrize("small_max", [None, 0], ids=["small", "planned"])
def test_a_span_past_max_span_is_not_read(torch, small_max):
    """One span longer than CRC32C_MAX_SPAN among good ones: its out is 0, the
    call returns CRC32C_ERANGE and the others are exact.  (An asynchronous call
    cannot report it; the outputs are the same.)  With one length: CRC32C_EINVAL."""
    rng = np.random.default_rng(5)
    buf = rng.integers(0, 256, 20000, dtype=np.uint8)
    t = _t(torch, buf)
    offs = np.array([0, 7, 5000, 9000, 19000], np.uint64)
    lens = np.array([4133, 100, MAX_SPAN + 1, 8000, 1000], np.uint32)
    ptrs = (t.data_ptr() + offs).astype(np.uint64)
    want = oracle.batch(buf, offs, np.where(lens > MAX_SPAN, 0, lens))
    want[2] = 0
    pl = _Dev(torch)
    for asynchronous in (False, True):
        rc, got = call_ptrs(pl, ptrs, lens, 0, None, small_max, asynchronous)
        assert rc == (_lib.CRC32C_OK if asynchronous else _lib.CRC32C_ERANGE)
        np.testing.assert_array_equal(got, want)
    rc, got = call_ptrs(pl, ptrs, None, MAX_SPAN + 1, None, small_max)
    assert rc == _lib.CRC32C_EINVAL and (got == SENT).all()


# ---------------------------------------------------------------------------
# host routes
# ---------------------------------------------------------------------------
def test_half_pinned_half_pageable(torch):
    """A batch with half its spans in page-locked memory and half pageable
    equals the all-pageable and the all-page-locked runs (and the oracle)."""
    case = pc.scattered()
    got = {}
    for side in ("mixed", "pageable", "pinned"):
        with Placed(torch, case.bufs, side) as pl:
            rc, got[side] = call_ptrs(pl, pl.ptrs(case.where, case.offs, case.span_lens()), _lens32(case), 0,
                                      case.crc_in)
        assert rc == _lib.CRC32C_OK
    np.testing.assert_array_equal(got["mixed"], got["pageable"])
    np.testing.assert_array_equal(got["mixed"], got["pinned"])
    np.testing.assert_array_equal(got["mixed"], case.expected(True))


@pytest.mark.parametrize("side", ("pageable", "pinned"))
def test_long_spans_in_separate_arrays(torch, side):
    """3 x 200 KiB in separate arrays (page-locked: one DMA per span, past the
    queue's span limit): exact, and the call leaves a kernel time."""
    rng = np.random.default_rng(200)
    bufs = [rng.integers(0, 256, 200 << 10, dtype=np.uint8) for _ in range(3)]
    want = np.array([oracle.crc32c(0, b[3:]) for b in bufs], np.uint32)
    with Placed(torch, bufs, side) as pl:
        ptrs = pl.ptrs(np.arange(3), np.full(3, 3, np.uint64), np.full(3, 1))
        rc, got = call_ptrs(pl, ptrs, None, (200 << 10) - 3, None)
        ms = _lib.lib.crc32c_last_kernel_ms()
    assert rc == _lib.CRC32C_OK and ms >= 0
    np.testing.assert_array_equal(got, want)


def test_host_refusals_write_nothing(torch):
    """A NULL pointer with bytes, and a span past the host limit: CRC32C_EINVAL, out untouched."""
    buf = np.arange(256, dtype=np.uint8)
    out = np.full(2 + PAD, SENT, np.uint32)
    for ptrs, lens in ((np.array([buf.ctypes.data, 0], np.uint64), np.array([10, 1], np.uint32)),
                       (np.array([buf.ctypes.data] * 2, np.uint64), np.array([10, (256 << 20) - 15], np.uint32))):
        b = _lib.PtrBatch(ptrs.ctypes.data, lens.ctypes.data, 0, None, out.ctypes.data, 2)
        job = ctypes.c_void_p()
        assert _lib.lib.crc32c_batch_ptrs(ctypes.byref(b), None) == _lib.CRC32C_EINVAL
        assert _lib.lib.crc32c_ptrs_submit(ctypes.byref(b), None, ctypes.byref(job)) == _lib.CRC32C_EINVAL
        assert (out == SENT).all()


def test_python_face(torch):
    """mc.batch_ptrs and mc.chains_ptrs over lists of host buffers and of device tensors."""
    rng = np.random.default_rng(6)
    bufs = [rng.integers(0, 256, k, dtype=np.uint8) for k in (0, 1, 4133, 70000)]
    want = np.array([oracle.crc32c(0, b) for b in bufs], np.uint32)
    first = np.array([0, 2, 2, 4], np.uint64)
    chains = np.array([oracle.crc32c(0, bufs[1]), 0, oracle.crc32c(want[2], bufs[3])], np.uint32)
    np.testing.assert_array_equal(mc.batch_ptrs([bytes(bufs[0]), bufs[1], bufs[2], bytes(bufs[3])]), want)
    np.testing.assert_array_equal(mc.chains_ptrs(bufs, first), chains)
    dev = [torch.from_numpy(b).cuda() for b in bufs]
    np.testing.assert_array_equal(mc.batch_ptrs(dev).cpu().numpy().view(np.uint32), want)
    got = mc.chains_ptrs(dev, torch.from_numpy(first.view(np.int64)).cuda())
    np.testing.assert_array_equal(got.cpu().numpy().view(np.uint32), chains)
    with pytest.raises(ValueError):
        mc.batch_ptrs([dev[1], bufs[2]])


# ---------------------------------------------------------------------------
# the queue
# ---------------------------------------------------------------------------
def _delta(before):
    """(launches, spans, jobs, solo_jobs) since `before`."""
    return tuple(a - b for a, b in zip(mc.queue_stats(), before))


def test_ptr_jobs_share_launches_with_ordinary_jobs(torch):
    """Eight threads submit one pointer job each, 8 spans in two registered
    arrays; four more submit ordinary crc32c_batch_submit jobs over one of the
    arrays.  They queue up behind a pageable job that runs alone: all twelve are
    counted as coalesced, in fewer than twelve launches, every CRC exact."""
    rng = np.random.default_rng(12)
    lib = _lib.lib
    arrays = [rng.integers(0, 256, 1 << 20, dtype=np.uint8) for _ in range(2)]
    blocker = rng.integers(0, 256, 32 << 20, dtype=np.uint8)
    for a in arrays:
        assert lib.crc32c_host_register(a.ctypes.data, a.size) == _lib.CRC32C_OK
    try:
        jobs = []
        for k in range(12):
            lens = rng.integers(0, 5000, 8).astype(np.uint32)
            offs = rng.integers(0, (1 << 20) - 5000, 8).astype(np.uint64)
            which = rng.integers(0, 2, 8) if k < 8 else np.zeros(8, np.int64)
            cin = rng.integers(0, 2**32, 8, dtype=np.uint64).astype(np.uint32)
            want = np.array([oracle.crc32c(int(cin[i]), arrays[which[i]][int(offs[i]):int(offs[i]) + int(lens[i])])
                             for i in range(8)], np.uint32)
            out = np.full(8 + PAD, SENT, np.uint32)
            if k < 8:
                ptrs = np.array([arrays[w].ctypes.data for w in which], np.uint64) + offs
                desc = _lib.PtrBatch(ptrs.ctypes.data, lens.ctypes.data, 0, cin.ctypes.data, out.ctypes.data, 8)
            else:
                ptrs = None
                desc = _lib.Spans(arrays[0].ctypes.data, arrays[0].size, offs.ctypes.data, 0, lens.ctypes.data, 0,
                                  cin.ctypes.data, out.ctypes.data, 8)
            jobs.append(dict(desc=desc, keep=(ptrs, lens, offs, cin), out=out, want=want, rc=None))
        boffs = (np.arange(512, dtype=np.uint64) << 16)
        bout = np.empty(512, np.uint32)
        bspans = _lib.Spans(blocker.ctypes.data, blocker.size, boffs.ctypes.data, 0, None, 1 << 16, None,
                            bout.ctypes.data, 512)
        ready, go = threading.Barrier(13), threading.Barrier(13)

        def run(j, k):
            handle = ctypes.c_void_p()
            ready.wait()
            go.wait()
            if k < 8:
                rc = lib.crc32c_ptrs_submit(ctypes.byref(j["desc"]), None, ctypes.byref(handle))
            else:
                rc = lib.crc32c_batch_submit(ctypes.byref(j["desc"]), 0, ctypes.byref(handle))
            j["rc"] = rc if rc else lib.crc32c_batch_wait(handle)

        threads = [threading.Thread(target=run, args=(j, k)) for k, j in enumerate(jobs)]
        for t in threads:
            t.start()
        ready.wait()
        s0 = mc.queue_stats()
        bjob = ctypes.c_void_p()
        assert lib.crc32c_batch_submit(ctypes.byref(bspans), 0, ctypes.byref(bjob)) == _lib.CRC32C_OK
        go.wait()
        for t in threads:
            t.join()
        assert lib.crc32c_batch_wait(bjob) == _lib.CRC32C_OK
        launches, spans, njobs, solo = _delta(s0)
        print(f"\n12 jobs of 8 spans went out in {launches} launches")
        assert [j["rc"] for j in jobs] == [_lib.CRC32C_OK] * 12
        for j in jobs:
            np.testing.assert_array_equal(j["out"][:8], j["want"])
            assert (j["out"][8:] == SENT).all()
        assert (njobs, spans, solo) == (12, 96, 1)  # (solo: the blocker)
        assert 1 <= launches < 12
        np.testing.assert_array_equal(bout, oracle.batch(blocker, boffs, np.full(512, 1 << 16)))
    finally:
        for a in arrays:
            lib.crc32c_host_unregister(a.ctypes.data)


def test_a_ptr_job_with_a_pageable_span_runs_alone(torch):
    """One pageable span among registered ones: the job runs solo, packed, and is exact."""
    rng = np.random.default_rng(13)
    lib = _lib.lib
    reg, page = rng.integers(0, 256, 1 << 16, dtype=np.uint8), rng.integers(0, 256, 1 << 16, dtype=np.uint8)
    assert lib.crc32c_host_register(reg.ctypes.data, reg.size) == _lib.CRC32C_OK
    try:
        offs = np.array([3, 1000, 20000, 65535 - 4133], np.uint64)
        lens = np.array([100, 4133, 0, 4133], np.uint32)
        src = [reg, reg, reg, page]
        ptrs = np.array([a.ctypes.data for a in src], np.uint64) + offs
        want = np.array([oracle.crc32c(0, a[int(o):int(o) + int(n)]) for a, o, n in zip(src, offs, lens)], np.uint32)
        for last_pageable, nsolo in ((True, 1), (False, 0)):
            if not last_pageable:
                ptrs[3] = reg.ctypes.data + int(offs[3])
                want[3] = oracle.crc32c(0, reg[int(offs[3]):int(offs[3]) + 4133])
            out = np.full(4 + PAD, SENT, np.uint32)
            b = _lib.PtrBatch(ptrs.ctypes.data, lens.ctypes.data, 0, None, out.ctypes.data, 4)
            s0 = mc.queue_stats()
            job = ctypes.c_void_p()
            assert lib.crc32c_ptrs_submit(ctypes.byref(b), None, ctypes.byref(job)) == _lib.CRC32C_OK
            assert lib.crc32c_batch_wait(job) == _lib.CRC32C_OK
            assert _delta(s0) == ((0, 0, 0, 1) if nsolo else (1, 4, 1, 0))
            np.testing.assert_array_equal(out[:4], want)
            assert (out[4:] == SENT).all()
    finally:
        lib.crc32c_host_unregister(reg.ctypes.data)


def test_device_ptr_job_is_ordered_behind_the_default_stream(torch):
    """A CRC32C_DEVICE pointer job runs alone on the queue, behind the copy the
    submitter queued on its default stream."""
    rng = np.random.default_rng(14)
    host = rng.integers(0, 256, 1 << 20, dtype=np.uint8)
    dev = torch.zeros(1 << 20, dtype=torch.uint8, device="cuda")
    offs = np.array([0, 4097, 500000], np.uint64)
    lens = np.array([4097, 300000, 12], np.uint32)
    dp, dl = _t(torch, (dev.data_ptr() + offs).astype(np.uint64)), _t(torch, lens)
    out = torch.full((3 + PAD,), SENT, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    with raw.pinned(host.size) as pin:
        pin[:] = host
        dev.copy_(torch.from_numpy(pin), non_blocking=True)
        b = _lib.PtrBatch(dp.data_ptr(), dl.data_ptr(), 0, None, out.data_ptr(), 3)
        opts = _lib.PtrOpts(_lib.CRC32C_DEVICE, None)
        job = ctypes.c_void_p()
        s0 = mc.queue_stats()
        assert _lib.lib.crc32c_ptrs_submit(ctypes.byref(b), ctypes.byref(opts), ctypes.byref(job)) == _lib.CRC32C_OK
        assert _lib.lib.crc32c_batch_wait(job) == _lib.CRC32C_OK
        assert _delta(s0) == (0, 0, 0, 1)
    got = out.cpu().numpy().view(np.uint32)
    np.testing.assert_array_equal(got[:3], oracle.batch(host, offs, lens))
    assert (got[3:] == SENT).all()

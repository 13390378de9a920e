"""The coalescing queue (memcached_amd/csrc/shim_queue.h) at its limits: the
conditions that decide whether a job shares a launch, each at its edge (spans of
256 KiB, 8192 spans, at least one span, a device-visible buffer), the cut that
ends a launch at 8192 spans, and every descriptor form through Queue::launch,
which rebuilds absolute addresses.  Counters from crc32c_queue_stats as deltas;
every CRC against the oracle."""
import ctypes

import numpy as np
import pytest

try:  # GPU processes load torch (and its HIP runtime) before libmcrc32c.so
    import torch as _torch  # noqa: F401
except ImportError:
    pass

from memcached_amd import _lib
from memcached_amd import crc32c as mc

from . import oracle
from . import raw_calls

pytestmark = pytest.mark.gpu

SIZE = 4 << 20
SMALL_MAX = 8192          # mcrc_dev::kSmallMax
SPAN_MAX = 256 << 10      # kQueueSpanMax


@pytest.fixture(scope="module")
def torch():
    return raw_calls.need_gpu()


@pytest.fixture(scope="module")
def bufs(torch):
    """(pageable, page-locked): the same 4 MiB twice."""
    host = np.random.default_rng(853).integers(0, 256, SIZE, dtype=np.uint8)
    host.setflags(write=False)
    pin = torch.from_numpy(host.copy()).pin_memory()
    return host, pin


class Job:
    """One submitted batch: its arrays stay alive until wait()."""

    def __init__(self, base, offs=None, lens=None, cin=None, n=None, stride=0, length=0, size=SIZE):
        self.offs = None if offs is None else np.ascontiguousarray(offs, np.uint64)
        self.lens = None if lens is None else np.ascontiguousarray(lens, np.uint32)
        self.cin = None if cin is None else np.ascontiguousarray(cin, np.uint32)
        self.n = int(n if n is not None else (self.offs if self.offs is not None else self.lens).size)
        self.stride, self.length = stride, length
        self.out = np.full(max(self.n, 1), 0x5A5A5A5A, np.uint32)
        p = lambda a: None if a is None else a.ctypes.data  # noqa: E731
        self.spans = _lib.Spans(base, size, p(self.offs), stride, p(self.lens), length, p(self.cin),
                                self.out.ctypes.data, self.n)
        self.handle = None

    def submit(self):
        self.handle = ctypes.c_void_p()
        _lib.check(_lib.lib.crc32c_batch_submit(ctypes.byref(self.spans), 0, ctypes.byref(self.handle)), "submit")
        return self

    def wait(self):
        rc = _lib.lib.crc32c_batch_wait(self.handle)
        self.handle = None
        return rc

    def batch(self):
        return _lib.lib.crc32c_batch(ctypes.byref(self.spans), 0, None)

    def want(self, host):
        offs = self.offs if self.offs is not None else np.arange(self.n, dtype=np.uint64) * np.uint64(self.stride)
        lens = self.lens if self.lens is not None else np.full(self.n, self.length, np.uint64)
        return oracle.batch(host, offs, lens, self.cin)

    def exact(self, host):
        return np.array_equal(self.out[:self.n], self.want(host))


def _delta(before):
    """(launches, spans, jobs, solo_jobs) since `before`."""
    return tuple(a - b for a, b in zip(mc.queue_stats(), before))


def test_span_length_edge(torch, bufs):
    """One span of 256 KiB shares a launch; one byte more and the job runs alone."""
    host, pin = bufs
    for length, coalesced in ((SPAN_MAX, True), (SPAN_MAX + 1, False)):
        s0 = mc.queue_stats()
        job = Job(pin.data_ptr(), offs=[5], lens=[length], cin=[0xDEADBEEF]).submit()
        assert job.wait() == _lib.CRC32C_OK
        launches, spans, jobs, solo = _delta(s0)
        assert (jobs, solo) == ((1, 0) if coalesced else (0, 1)), length
        assert (launches, spans) == ((1, 1) if coalesced else (0, 0)), length
        assert job.exact(host), length


def test_span_count_edge(torch, bufs):
    """8192 spans fit one launch; 8193 run alone.  The same through synchronous
    crc32c_batch, which takes the queue for the first and stages the second."""
    host, pin = bufs
    rng = np.random.default_rng(8192)
    for n, coalesced in ((SMALL_MAX, True), (SMALL_MAX + 1, False)):
        lens = rng.integers(1, 65, n)
        offs = rng.integers(0, SIZE - 64, n)
        cin = rng.integers(0, 1 << 32, n, dtype=np.uint64)
        s0 = mc.queue_stats()
        job = Job(pin.data_ptr(), offs, lens, cin).submit()
        assert job.wait() == _lib.CRC32C_OK
        assert _delta(s0) == ((1, n, 1, 0) if coalesced else (0, 0, 0, 1)), n
        assert job.exact(host), n
        s0 = mc.queue_stats()
        sync = Job(pin.data_ptr(), offs, lens, cin)
        assert sync.batch() == _lib.CRC32C_OK
        assert _delta(s0) == ((1, n, 1, 0) if coalesced else (0, 0, 0, 0)), n
        assert sync.exact(host), n


def test_launches_are_cut_at_8192_spans(torch, bufs):
    """Behind a blocker that runs alone (pageable, 64 spans of 64 KiB), seven
    coalescible jobs wait together; the dispatcher packs them in order and cuts a
    launch where the next job would pass 8192 spans.  Every job has its own
    lengths and initial CRCs, so a hand-out from the wrong place shows.  How the
    jobs pack depends on when the dispatcher looks, so only the bounds are
    asserted: every span once, seven jobs, between ceil(total / 8192) and seven
    launches."""
    host, pin = bufs
    rng = np.random.default_rng(7)
    blocker = Job(host.ctypes.data, offs=np.arange(64) * 65536, lens=np.full(64, 65536))
    sizes = [3000, 3000, 2192, 1, 5000, 4000, 8192]
    jobs = []
    for k, n in enumerate(sizes):
        lens = rng.integers(0, 40, n) + 100 * k  # job k: lengths 100 k .. 100 k + 39
        jobs.append(Job(pin.data_ptr(), rng.integers(0, SIZE - 1024, n), lens,
                        rng.integers(0, 1 << 32, n, dtype=np.uint64)))
    s0 = mc.queue_stats()
    blocker.submit()
    for j in jobs:
        j.submit()
    assert blocker.wait() == _lib.CRC32C_OK
    for j in jobs:
        assert j.wait() == _lib.CRC32C_OK
    launches, spans, njobs, solo = _delta(s0)
    total = sum(sizes)
    print(f"\n{len(sizes)} jobs of {sizes} spans went out in {launches} launches (4 when all seven waited together)")
    assert blocker.exact(host)
    assert [j.exact(host) for j in jobs] == [True] * len(jobs)
    assert spans == total and njobs == len(sizes) and solo == 1
    assert -(-total // SMALL_MAX) <= launches <= len(sizes)


def test_descriptor_forms_through_the_coalesced_launch(torch, bufs):
    """Queue::launch turns every form of crc32c_spans into absolute addresses,
    lengths and initial CRCs: a stride and one length without crc_in; offsets
    with one length; offsets and lengths with empty spans among others, the
    span [0, 1), a span that ends on the buffer's last byte and starts at all 16
    residues mod 16.  Submitted together, all coalesced, all exact."""
    host, pin = bufs
    rng = np.random.default_rng(16)
    base = pin.data_ptr()
    strided = Job(base, n=500, stride=100, length=77)
    fixed = Job(base, offs=rng.integers(0, SIZE - 333, 300), length=333, cin=rng.integers(0, 1 << 32, 300,
                                                                                             dtype=np.uint64))
    offs = [0, SIZE - 4097, SIZE, 17, SIZE - 1] + [4096 * 3 + r * 17 for r in range(16)]
    lens = [1, 4097, 0, 0, 1] + [1000 + r for r in range(16)]
    assert sorted(o % 16 for o in offs[5:]) == list(range(16))
    mixed = Job(base, offs, lens, cin=rng.integers(0, 1 << 32, len(offs), dtype=np.uint64))
    unseeded = Job(base, offs, lens)
    jobs = [strided, fixed, mixed, unseeded]
    s0 = mc.queue_stats()
    for j in jobs:
        j.submit()
    for j in jobs:
        assert j.wait() == _lib.CRC32C_OK
    launches, spans, njobs, solo = _delta(s0)
    assert (njobs, solo) == (len(jobs), 0) and spans == sum(j.n for j in jobs) and 1 <= launches <= len(jobs)
    assert [j.exact(host) for j in jobs] == [True] * len(jobs)


def test_pageable_buffer_is_not_coalesced(torch, bufs):
    """The same short job over pageable memory runs alone."""
    host, _ = bufs
    s0 = mc.queue_stats()
    job = Job(host.ctypes.data, offs=[0, 100], lens=[50, 60]).submit()
    assert job.wait() == _lib.CRC32C_OK
    assert _delta(s0) == (0, 0, 0, 1) and job.exact(host)


def test_empty_job(torch, bufs):
    """n == 0 through submit and wait: CRC32C_OK, no launch, nothing written."""
    _, pin = bufs
    s0 = mc.queue_stats()
    job = Job(pin.data_ptr(), offs=np.zeros(0), lens=np.zeros(0), n=0).submit()
    assert job.wait() == _lib.CRC32C_OK
    launches, spans, jobs, _ = _delta(s0)
    assert (launches, spans, jobs) == (0, 0, 0) and job.out[0] == 0x5A5A5A5A

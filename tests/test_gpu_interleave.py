"""The library's calls out of their files' order, right behind calls that
returned early, back to back without a synchronize, on two streams at once and
beside running K1 batches and queue launches: every op of
tests/interleave_cases.py, every time compared exactly -- each array with the
sentinel behind it, each count, each return code -- with what the oracle and
the CPU models expect.  All calls of a process share the Device's grow-only
scratch and hand it from stream to stream; nothing expected here comes from the
library."""
import collections
import ctypes
import threading

import numpy as np
import pytest

try:  # GPU processes load torch (and its HIP runtime) before libmcrc32c.so
    import torch as _torch  # noqa: F401
except ImportError:
    pass

from memcached_amd import _lib, layout
from memcached_amd import crc32c as mc

from . import copy_items_model
from . import interleave_cases as ic
from . import keep_stamped_model as ks
from . import oracle
from . import raw_calls
from . import routes_cases

pytestmark = pytest.mark.gpu

ORDERS = ("seed1", "seed2", "seed3", "seed4", "seed5", "seed6", "largest_first", "smallest_first")
ASYNC = _lib.CRC32C_DEVICE | _lib.CRC32C_ASYNC


@pytest.fixture(scope="module")
def torch():
    return raw_calls.need_gpu()


def _run_and_check(torch, op, stream=None, tag="", tune=True):
    """tune: the chain ops that name a route below the small-batch limit get
    it through crc32c_set_small_max, which is process-wide: one thread only."""
    with raw_calls.small_max(op.small_max if tune else None):
        got = op.run(torch, stream)
    ic.check(op, got, tag)


# -- 1 and 2: one stream ---------------------------------------------------------

@pytest.mark.parametrize("order", ORDERS)
def test_orders_on_one_stream(torch, order):
    """The whole table on the default stream in six seeded permutations, from
    the largest scratch demand to the smallest and back; behind each error op
    comes a different entry point that succeeds."""
    ops = ic.orders()[order]
    for k, op in enumerate(ops):
        _run_and_check(torch, op, tag=f"{order}[{k}] after {ops[k - 1].name if k else 'nothing'}")


ERRORS = ic.error_ops()


@pytest.mark.parametrize("err", ERRORS, ids=[op.name for op in ERRORS])
def test_every_op_after_every_error(torch, err):
    """Each call that succeeds, directly behind a call that returned early (at
    CRC32C_EWORK after the count pass, at CRC32C_EINVAL from the list check, at
    CRC32C_ERANGE), which is checked every time as well."""
    for op in ic.success_ops():
        _run_and_check(torch, err, tag=f"before {op.name}")
        _run_and_check(torch, op, tag=f"after {err.name}")


# -- 3: asynchronous calls, no synchronize between them ----------------------------

@pytest.fixture(scope="module")
def stamp_then_copy():
    """The 4096 images of the item routes: what a stamp that keeps carried CRCs
    leaves, and what a copy of the images as stamped, packed back to back,
    writes."""
    buf, offs = routes_cases.items_case("4096")
    s_buf, s_ok, _ = routes_cases.items_want("4096", "keep")
    doffs, at = [], 0
    for o in offs.tolist():
        doffs.append(at)
        if ks.header_sane(s_buf, o, 0):
            at += layout.ntotal_of(s_buf, o)
    doffs = np.array(doffs, np.uint64)
    dst_init = np.full(at + 7, 0xa5, np.uint8)
    c_dst, c_ok, c_bad, erange = copy_items_model.expected_copy(s_buf, offs, 0, dst_init, doffs)
    assert not erange and set(c_ok.tolist()) == {0, 1, 3} and c_bad == int((s_ok == 0).sum())
    return buf, offs, s_buf, s_ok, doffs, dst_init, c_dst, c_ok


@pytest.mark.parametrize("nstreams", [1, 2])
def test_async_calls_back_to_back(torch, stamp_then_copy, nstreams):
    """CRC32C_DEVICE | CRC32C_ASYNC, no synchronize between the calls: stamp
    items, copy those images, chains, a planned span batch, K1, one
    synchronize.  On one caller stream, and with consecutive calls on two
    alternating streams, so that the scratch crosses streams at every call; the
    copy then waits for the stamp through an event of the test's."""
    buf, offs, s_buf, s_ok, doffs, dst_init, c_dst, c_ok = stamp_then_copy
    chains, planned, k1 = (ic.by_name(n) for n in ("chains_lens_small", "spans_planned", "k1_4099"))
    lib = _lib.lib
    side = ic.Side(torch, None, "device")
    n = offs.size
    d_buf, d_offs, d_doffs, d_dst = side.data(buf), side.desc(offs), side.desc(doffs), side.data(dst_init)
    s_okay, c_okay = side.out(n, np.uint8), side.out(n, np.uint8)
    ch_buf, ch_first = side.data(chains.inputs["buf"]), side.desc(chains.inputs["first"])
    ch_iov, ch_out = side.out(chains.inputs["n"], np.uint32), side.out(chains.inputs["nchains"], np.uint32)
    ch_spans = ic.spans_struct(side, chains, ch_buf, ch_iov)
    pl_out = side.out(planned.inputs["n"], np.uint32)
    pl_spans = ic.spans_struct(side, planned, side.data(planned.inputs["buf"]), pl_out)
    k1_out = side.out(k1.inputs["n"], np.uint32)
    k1_spans = ic.spans_struct(side, k1, side.data(k1.inputs["buf"]), k1_out)
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream() for _ in range(nstreams)]
    handle = [ctypes.c_void_p(st.cuda_stream) for st in streams]
    at = lambda k: k % nstreams  # noqa: E731
    rcs = [lib.crc32c_stamp_items(d_buf.data_ptr(), buf.size, 0, d_offs.data_ptr(), n, s_okay.data_ptr(), None,
                                  ASYNC | _lib.CRC32C_KEEP_STAMPED, handle[at(0)])]
    if nstreams > 1:
        stamped = torch.cuda.Event()
        stamped.record(streams[at(0)])
        streams[at(1)].wait_event(stamped)
    rcs.append(lib.crc32c_copy_items(d_buf.data_ptr(), buf.size, 0, d_offs.data_ptr(), d_dst.data_ptr(),
                                     dst_init.size, d_doffs.data_ptr(), n, c_okay.data_ptr(), None, ASYNC,
                                     handle[at(1)]))
    rcs.append(lib.crc32c_batch_chains(ctypes.byref(ch_spans), ch_first.data_ptr(), chains.inputs["nchains"],
                                       ch_out.data_ptr(), ASYNC, handle[at(2)]))
    rcs.append(lib.crc32c_batch(ctypes.byref(pl_spans), ASYNC, handle[at(3)]))
    rcs.append(lib.crc32c_batch(ctypes.byref(k1_spans), ASYNC, handle[at(4)]))
    for st in streams:  # (one synchronize; with two streams, one each)
        st.synchronize()
    assert rcs == [_lib.CRC32C_OK] * 5
    host = side.host
    np.testing.assert_array_equal(host(s_okay, np.uint8), ic.ended(s_ok))
    np.testing.assert_array_equal(host(d_buf, np.uint8), s_buf)
    np.testing.assert_array_equal(host(c_okay, np.uint8), ic.ended(c_ok))
    np.testing.assert_array_equal(host(d_dst, np.uint8), c_dst)
    np.testing.assert_array_equal(host(ch_iov, np.uint32), chains.want["iov_out"])
    np.testing.assert_array_equal(host(ch_out, np.uint32), chains.want["out"])
    np.testing.assert_array_equal(host(pl_out, np.uint32), planned.want["out"])
    np.testing.assert_array_equal(host(k1_out, np.uint32), k1.want["out"])


# -- 4 to 6: more than one thread --------------------------------------------------

def _walker(torch, ops, errors, name, done=None):
    """A thread's body: every op once on a stream of its own, each checked; the
    first failure ends the walk (nothing is run again)."""
    def body():
        try:
            st = torch.cuda.Stream()
            for k, op in enumerate(ops):
                _run_and_check(torch, op, stream=st, tag=f"{name}[{k}]", tune=False)
        except BaseException as e:  # noqa: BLE001
            errors.append(f"{name}: {e!r}"[:2000])
        finally:
            if done is not None:
                done.set()
    return threading.Thread(target=body, name=name)


def _join(threads, errors):
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors, errors


@pytest.mark.parametrize("pair", [("seed1", "smallest_first"), ("largest_first", "seed2")], ids="-".join)
def test_ops_on_two_streams(torch, pair):
    """Two threads, a stream each, the table in two different orders with
    synchronous calls: the lease's wait for the previous call's event is all
    that keeps them from sharing scratch."""
    errors, orders = [], ic.orders()
    _join([_walker(torch, orders[name], errors, name) for name in pair], errors)


@pytest.fixture(scope="module")
def k1_cache():
    """(The 256 MiB batch lives as long as this module's tests.)"""
    cache = {}
    yield cache
    cache.clear()


def _k1_batch(cache, torch, with_cin):
    """16 x CUs x 16 items of 4 KiB (8 steps per wave: below K1's lockstep
    rounds and its claimed tail, so no barrier is involved) and the oracle's
    CRCs, computed once."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    if "data" not in cache:
        n = 16 * cus * 16
        rng = np.random.default_rng(16 * 16)
        cache["data"] = np.frombuffer(rng.bytes(n * 4096), np.uint8)
        cache["cin"] = rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
    data, cin = cache["data"], cache["cin"] if with_cin else None
    if with_cin not in cache:
        n = data.size // 4096
        cache[with_cin] = ic.ended(oracle.batch(data, np.arange(n, dtype=np.uint64) * 4096, np.full(n, 4096), cin))
    return data, cin, cache[with_cin]


def _k1_thread(torch, batch, ready, stop, errors, launches):
    def body():
        try:
            data, cin, want = batch
            n = data.size // 4096
            st = torch.cuda.Stream()
            with torch.cuda.stream(st):
                d = torch.from_numpy(data).cuda()
                d_cin = None if cin is None else torch.from_numpy(cin.view(np.int32)).cuda()
                outs = [torch.full((n + 1,), ic.SENT[4], dtype=torch.int32, device="cuda") for _ in range(2)]
                st.synchronize()
                inflight = collections.deque()
                k = 0
                while k < 20 or (not stop.is_set() and k < 100000):
                    if len(inflight) == 4:  # (a few batches ahead of the device, not an unbounded backlog)
                        inflight.popleft().synchronize()
                    s = _lib.Spans(d.data_ptr(), data.size, None, 4096, None, 4096, ic.ptr(d_cin),
                                   outs[k % 2].data_ptr(), n)
                    rc = _lib.lib.crc32c_batch(ctypes.byref(s), ASYNC, ctypes.c_void_p(st.cuda_stream))
                    assert rc == _lib.CRC32C_OK, (k, rc)
                    ev = torch.cuda.Event()
                    ev.record(st)
                    inflight.append(ev)
                    k += 1
                    ready.set()
                st.synchronize()
                launches.append(k)
                for out in outs:  # (the last batch's and the one before it)
                    np.testing.assert_array_equal(out.cpu().numpy().view(np.uint32), want)
        except BaseException as e:  # noqa: BLE001
            errors.append(f"k1: {e!r}"[:2000])
        finally:
            ready.set()
    return threading.Thread(target=body, name="k1")


@pytest.mark.parametrize("with_cin", [False, True], ids=["plain", "with_cin"])
def test_ops_beside_k1(torch, k1_cache, with_cin):
    """One thread keeps asynchronous K1 batches in flight on its own stream (an
    asynchronous K1 batch takes neither the device's mutex nor a lease) while
    another runs every op of the table once: the walk, K5, k_copy, the salvage
    scan and the repair search share the SIMDs with k_fixed, and every result
    of both is exact."""
    batch = _k1_batch(k1_cache, torch, with_cin)
    errors, launches = [], []
    ready, stop = threading.Event(), threading.Event()
    k1 = _k1_thread(torch, batch, ready, stop, errors, launches)
    k1.start()
    ready.wait()
    walker = _walker(torch, ic.table(), errors, "ops", done=stop)
    walker.start()
    walker.join()
    stop.set()
    k1.join()
    assert not errors, errors
    assert launches and launches[0] >= 20
    print(f"\nK1 batches beside the table: {launches[0]}")


def test_ops_beside_the_queue(torch):
    """The same beside the queue's coalesced launches on the queue's own
    stream: one thread submits and waits 12 coalescable jobs at a time, every
    job checked, while another runs every op once."""
    errors, rounds = [], []
    ready, stop = threading.Event(), threading.Event()
    queue_op = ic.by_name("queue_12_jobs")

    def submit():
        try:
            k = 0
            while k < 3 or (not stop.is_set() and k < 100000):
                ic.check(queue_op, queue_op.run(torch), f"round {k}")
                k += 1
                ready.set()
            rounds.append(k)
        except BaseException as e:  # noqa: BLE001
            errors.append(f"queue: {e!r}"[:2000])
        finally:
            ready.set()

    before = mc.queue_stats()
    q = threading.Thread(target=submit, name="queue")
    q.start()
    ready.wait()
    walker = _walker(torch, ic.table(), errors, "ops", done=stop)
    walker.start()
    walker.join()
    stop.set()
    q.join()
    assert not errors, errors
    launches, spans, jobs, _ = (a - b for a, b in zip(mc.queue_stats(), before))
    assert rounds and rounds[0] >= 3 and jobs >= 12 * rounds[0] and 0 < launches <= jobs
    print(f"\nqueue rounds beside the table: {rounds[0]}, {jobs} jobs in {launches} launches")

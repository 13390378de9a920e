"""K1's claimed tail on the GPU: with the threshold at its minimum T0
(crc32c_set_k1_tail_min, restored afterwards) every CRC is checked against the
CPU oracle, with and without crc_in, at stride 4096 (the non-temporal
instantiations) and 4112 (the default-policy ones), with a sentinel behind
out[n].

With W = 16 x CUs waves:
  2 W T0 - 1, 2 W T0,     the first launches with a tail (cg = T0: a static part
  2 W T0 + 1              of 4 steps, which the tail loop runs as its first chunk)
  2 W T0 - W - 3          cg = T0 still, the pool short of a full eighth
  2 (8 W + 9)             a pool of 3 chunks: 13 of the 16 sub-pools are empty
  2 W (T0 + 1) + 2 W + 11 the last chunk cut to two groups, the last of one item
  2 W 4 T0 + 5            a static part of 28 steps, a pool of more than W chunks
  2 W 40 at stride 2048   (overlapping items, no more bytes than the rest) a
                          static part of 32 steps: lockstep rounds, their make-up
                          arrival and the tail in one launch
and three launches of different counts back to back on one stream (the reset),
two threads on two streams, more streams than counter slots (the launches
without a slot are static), and the tail switched off (UINT64_MAX).

A miscounted barrier would hang, not miscompute, so tools/gpu_suite.sh runs
this module in its first step beside test_gpu_k1_lockstep.py, alone and under
that step's limit.  The data and the oracle's CRCs are computed once for the
largest case: item i at a given stride is the same bytes in every case."""
import ctypes
import threading

import numpy as np
import pytest

try:  # GPU processes load torch (and its HIP runtime) before libmcrc32c.so
    import torch as _torch  # noqa: F401
except ImportError:
    pass

from memcached_amd import _lib

from . import k1_rounds_model as m
from . import k1_tail_model as t
from . import oracle

pytestmark = pytest.mark.gpu
STRIDES = (4096, 4112)
NEVER = 2**64 - 1
SENTINEL = 0x5a5a5a5a
ROUNDS_STEPS, ROUNDS_STRIDE = 40, 2048  # test_rounds_and_tail_in_one_launch

CASES = {
    "2WT0-1": lambda W, T0: 2 * W * T0 - 1, "2WT0": lambda W, T0: 2 * W * T0, "2WT0+1": lambda W, T0: 2 * W * T0 + 1,
    "2WT0-W-3": lambda W, T0: 2 * W * T0 - W - 3,
    "few chunks": lambda W, T0: 2 * (8 * W + 9),
    "cut chunk, odd item": lambda W, T0: 2 * W * (T0 + 1) + 2 * W + 11,
    "2W4T0+5": lambda W, T0: 2 * W * 4 * T0 + 5,
}


@pytest.fixture(scope="module")
def world():
    """W, T0, the bytes on the device, crc_in, and the oracle's CRCs per
    (stride, with crc_in) at the largest item count; the threshold is T0 for
    the module's tests."""
    import torch
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    from memcached_amd import crc32c as mc
    assert mc.gpu_count() >= 1, "libmcrc32c.so sees no gfx950 device"
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    W, T0 = 16 * cus, t.consts()["floor"]
    nmax = max(f(W, T0) for f in CASES.values())
    rng = np.random.default_rng(21)
    host = rng.integers(0, 256, nmax * max(STRIDES), dtype=np.uint8)
    cin = rng.integers(0, 2**32, nmax, dtype=np.uint64).astype(np.uint32)
    want = {}
    for stride in STRIDES:
        offs = np.arange(nmax, dtype=np.uint64) * stride
        for c in (None, cin):
            want[stride, c is not None] = oracle.batch(host, offs, np.full(nmax, 4096), c)
    dev = torch.from_numpy(host).cuda()
    dcin = torch.from_numpy(cin.view(np.int32)).cuda()
    prev = _lib.lib.crc32c_set_k1_tail_min(0)  # (clamped up to T0)
    assert _lib.lib.crc32c_set_k1_tail_min(T0) == T0
    yield dict(cus=cus, W=W, T0=T0, nmax=nmax, dev=dev, dcin=dcin, want=want, torch=torch)
    _lib.lib.crc32c_set_k1_tail_min(prev)


def _launch(w, n, stride, with_cin, out, flags=_lib.CRC32C_DEVICE, stream=None):
    s = _lib.Spans(w["dev"].data_ptr(), n * stride, None, stride, None, 4096,
                   w["dcin"].data_ptr() if with_cin else None, out.data_ptr(), n)
    _lib.check(_lib.lib.crc32c_batch(ctypes.byref(s), flags, stream))


def _check(w, n, stride, with_cin, out, what):
    got = out[:n].cpu().numpy().view(np.uint32)
    np.testing.assert_array_equal(got, w["want"][stride, with_cin][:n], err_msg=f"{what} n {n} stride {stride}")
    assert int(out[n]) == SENTINEL, f"{what}: written past the batch"  # (out has n + 1 entries at least)


def _new_out(w, n):
    return w["torch"].full((n + 1,), SENTINEL, dtype=w["torch"].int32, device="cuda")


def test_cases_reach_the_paths_they_name(world):
    W, T0, cus = world["W"], world["T0"], world["cus"]
    c = t.consts()
    ns = {k: f(W, T0) for k, f in CASES.items()}
    assert all(t.tail_on(n, cus, T0) for n in ns.values())
    assert not t.tail_on(2 * W * T0 - 2 * W, cus, T0)
    geo = {k: t.geometry(n, cus) for k, n in ns.items()}
    sp = dict(zip(ns, t.library_splits([(g[1], g[0]) for g in geo.values()])))
    for k in ("2WT0-1", "2WT0", "2WT0-W-3"):
        assert geo[k][2] == T0 and sp[k][0] == 4
    assert geo["2WT0+1"][2] == T0 + 1 and sp["2WT0+1"][0] == 8 and sp["2WT0+1"][2] == 1
    assert 0 < sp["few chunks"][2] < c["pools"]
    k = "cut chunk, odd item"
    assert (geo[k][1] - sp[k][1]) % c["steps"] and ns[k] % 2
    assert sp["2W4T0+5"][0] == 28 and sp["2W4T0+5"][2] > W
    (cg_s, _, nchunks, _), = t.library_splits([(W * ROUNDS_STEPS, W)])
    assert cg_s >= m.rounds_min_steps() and m.library_rounds([cg_s])[1][0] > 0 and nchunks > W


@pytest.mark.parametrize("case", list(CASES))
def test_k1_tail_counts(world, case):
    w = world
    n = CASES[case](w["W"], w["T0"])
    out = _new_out(w, w["nmax"])
    for stride in STRIDES:
        for with_cin in (False, True):
            out.fill_(SENTINEL)
            _launch(w, n, stride, with_cin, out)
            _check(w, n, stride, with_cin, out, case)


def test_rounds_and_tail_in_one_launch(world):
    w = world
    n = 2 * w["W"] * ROUNDS_STEPS
    host = w["dev"][:(n - 1) * ROUNDS_STRIDE + 4096].cpu().numpy()
    want = oracle.batch(host, np.arange(n, dtype=np.uint64) * ROUNDS_STRIDE, np.full(n, 4096), None)
    out = _new_out(w, n)
    s = _lib.Spans(w["dev"].data_ptr(), (n - 1) * ROUNDS_STRIDE + 4096, None, ROUNDS_STRIDE, None, 4096, None,
                   out.data_ptr(), n)
    _lib.check(_lib.lib.crc32c_batch(ctypes.byref(s), _lib.CRC32C_DEVICE, None))
    np.testing.assert_array_equal(out[:n].cpu().numpy().view(np.uint32), want)
    assert int(out[n]) == SENTINEL


def test_tail_off_gives_the_same_crcs(world):
    w = world
    n = CASES["2W4T0+5"](w["W"], w["T0"])
    out = _new_out(w, n)
    prev = _lib.lib.crc32c_set_k1_tail_min(NEVER)
    try:
        assert prev == w["T0"] and _lib.lib.crc32c_set_k1_tail_min(NEVER) == NEVER
        for stride in STRIDES:
            out.fill_(SENTINEL)
            _launch(w, n, stride, True, out)
            _check(w, n, stride, True, out, "tail off")
    finally:
        _lib.lib.crc32c_set_k1_tail_min(prev)


def test_back_to_back_launches_on_one_stream(world):
    """Three asynchronous launches of different counts, no sync between them:
    each finds the counters its predecessor's last workgroup zeroed."""
    w = world
    torch = w["torch"]
    st = torch.cuda.Stream()
    ns = [CASES[k](w["W"], w["T0"]) for k in ("2W4T0+5", "few chunks", "cut chunk, odd item")]
    outs = [_new_out(w, n) for n in ns]
    torch.cuda.synchronize()
    for rep in range(2):
        for n, out in zip(ns, outs):
            _launch(w, n, 4096, False, out, _lib.CRC32C_DEVICE | _lib.CRC32C_ASYNC, ctypes.c_void_p(st.cuda_stream))
    st.synchronize()
    for n, out in zip(ns, outs):
        _check(w, n, 4096, False, out, "back to back")


def test_two_threads_on_two_streams(world):
    w = world
    torch = w["torch"]
    ns = [CASES[k](w["W"], w["T0"]) for k in ("2WT0+1", "2W4T0+5", "cut chunk, odd item", "2WT0-W-3")]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    assert streams[0].cuda_stream != streams[1].cuda_stream
    outs = [[_new_out(w, n) for n in ns] for _ in streams]
    torch.cuda.synchronize()
    errors = []

    def run(k):
        try:
            torch.cuda.set_device(0)
            for n, out in zip(ns, outs[k]):
                _launch(w, n, STRIDES[k], bool(k), out, _lib.CRC32C_DEVICE | _lib.CRC32C_ASYNC,
                        ctypes.c_void_p(streams[k].cuda_stream))
            streams[k].synchronize()
        except Exception as e:  # noqa: BLE001
            errors.append(e)

    th = [threading.Thread(target=run, args=(k,)) for k in range(2)]
    for x in th:
        x.start()
    for x in th:
        x.join()
    assert not errors, errors
    for k in range(2):
        for n, out in zip(ns, outs[k]):
            _check(w, n, STRIDES[k], bool(k), out, f"thread {k}")


def _hip():
    """The HIP runtime this process has loaded (through torch or libmcrc32c.so)."""
    try:
        h = ctypes.CDLL(None)
        h.hipStreamCreateWithFlags
        return h
    except (OSError, AttributeError):
        with open("/proc/self/maps") as f:
            paths = {line.split()[-1] for line in f if "libamdhip64" in line}
        assert paths, "no HIP runtime loaded"
        return ctypes.CDLL(sorted(paths)[0])


def test_more_streams_than_slots(world):
    """Capacity + 2 streams of the runtime's own, one launch each: those
    without a counter slot run the static launch, with the same CRCs."""
    w = world
    hip = _hip()
    hip.hipStreamCreateWithFlags.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_uint]
    hip.hipStreamSynchronize.argtypes = [ctypes.c_void_p]
    hip.hipStreamDestroy.argtypes = [ctypes.c_void_p]
    n = CASES["2WT0+1"](w["W"], w["T0"])
    streams, outs = [], []
    w["torch"].cuda.synchronize()
    try:
        for _ in range(64 + 2):
            s = ctypes.c_void_p()
            assert hip.hipStreamCreateWithFlags(ctypes.byref(s), 1) == 0  # (hipStreamNonBlocking)
            streams.append(s)
            outs.append(_new_out(w, n))
        assert len({s.value for s in streams}) == len(streams)
        w["torch"].cuda.synchronize()
        for s, out in zip(streams, outs):
            _launch(w, n, 4096, True, out, _lib.CRC32C_DEVICE | _lib.CRC32C_ASYNC, s)
        for s in streams:
            assert hip.hipStreamSynchronize(s) == 0
        for out in outs:
            _check(w, n, 4096, True, out, "more streams than slots")
    finally:
        for s in streams:
            hip.hipStreamDestroy(s)

"""Fixed-stride span batches (offsets == NULL) through the C ABI at every route
they can take: the cases of tests/stride_cases.py, whose route labels and
buffer sizes tests/test_host_route.py confirms against span_route on the CPU.

Each family of kernels holds a code path of its own for a stride:
k_lines<0, false> (K5 over a whole batch of equal spans: the benchmark's
config 2r), k_blocks<true, false> (K4 without a plan, which skips its
descriptor ring), the stride branch of decode_unit / k_spans, of k_small and
k_final, and of k_count (a stride with lens[]).  Every call goes through
_lib.Spans (mc.batch refuses a stride with a length), every output array is
pre-filled with a sentinel, every expected value is the oracle over the host
copy of the bytes, and every comparison is exact."""
import ctypes
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

try:  # GPU processes load torch (and its HIP runtime) before libmcrc32c.so
    import torch as _torch  # noqa: F401
except ImportError:
    pass

from memcached_amd import _lib

from . import base_shift_cases as bs
from . import oracle
from . import raw_calls as raw
from . import stride_cases as sc
from .test_gpu_base_shift import _holds, _place

pytestmark = pytest.mark.gpu
SENT = 0x5A5A5A5A
SHIFTS = (0, 1, 127)
CASES = sc.cases()
GiB = 1 << 30
PAD = 256  # allocated behind a buffer that is not framed (the kernels load whole 16-byte and 128-byte granules)


@pytest.fixture(scope="module")
def torch():
    return raw.need_gpu()


def _d(torch, a, view):
    return torch.from_numpy(np.ascontiguousarray(a).view(view).copy()).cuda()


def _u32(t):
    return t.cpu().numpy().view(np.uint32)


def _device_call(torch, base, nbytes, n, length, stride, dlens=None, dcin=None, small_max=0):
    """One crc32c_batch over device memory at `base`: (rc, out), out pre-filled with SENT."""
    out = torch.full((max(n, 1),), SENT, dtype=torch.int32, device="cuda")
    sp = _lib.Spans(base, nbytes, None, stride, None if dlens is None else dlens.data_ptr(), length,
                    None if dcin is None else dcin.data_ptr(), out.data_ptr(), n)
    with raw.small_max(small_max):
        rc = _lib.lib.crc32c_batch(ctypes.byref(sp), _lib.CRC32C_DEVICE, None)
    torch.cuda.synchronize()
    return rc, _u32(out)[:n]


# ---------------------------------------------------------------------------
# parity: every case, device memory, three base residues
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("s", SHIFTS)
@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_parity(torch, case, s):
    """The case's spans where they lie at base shift s (the buffer framed as
    tests/base_shift_cases.py frames it: nothing around it may change), from 0
    and from crc_in."""
    alloc, v = _place(torch, case.buf, s) if case.nbytes else (torch.from_numpy(bs.frame(case.buf, s)).cuda(), None)
    base = alloc.data_ptr() + bs.SLACK + s  # (an empty view has no address of its own)
    assert v is None or v.data_ptr() == base
    dlens = None if case.lens is None else _d(torch, case.lens, np.int32)
    dcin = _d(torch, case.crc_in, np.int32)
    for cin in (None, dcin):
        rc, got = _device_call(torch, base, case.nbytes, case.n, case.length, case.stride, dlens, cin, case.small_max)
        assert rc == _lib.CRC32C_OK, (case.name, s, rc)
        want = case.expected(cin is not None)
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, (case.name, s, cin is not None, bad.size, bad[:8].tolist())
        if case.stride == 0 and case.lens is None:
            # every span is the same bytes
            if cin is None:
                assert (got == got[0]).all()
            else:
                one = oracle.batch(case.buf, np.zeros(case.n, np.uint64), np.full(case.n, case.length, np.uint64),
                                   case.crc_in)
                np.testing.assert_array_equal(got, one)
    _holds(alloc, case.buf, s)


# ---------------------------------------------------------------------------
# the host path: staged by span_off
# ---------------------------------------------------------------------------
HOST_CASES = [c for c in CASES if c.host]


def _host_spans(case, cin, out):
    lens = case.lens
    return _lib.Spans(case.buf.ctypes.data, case.nbytes, None, case.stride, None if lens is None else lens.ctypes.data,
                      case.length, None if cin is None else cin.ctypes.data, out.ctypes.data, case.n)


@pytest.mark.parametrize("how", ["batch", "submit_wait"])
@pytest.mark.parametrize("case", HOST_CASES, ids=[c.name for c in HOST_CASES])
def test_host_path(case, how):
    """One stride per route (the overlapping len - 1 among them) and the stride
    with lens[] shapes from pageable host memory, through crc32c_batch with
    flags 0 and through crc32c_batch_submit / _wait: the pipeline stages the
    spans by span_off and must hand the device the same ones."""
    raw.need_gpu()
    for cin in (None, case.crc_in):
        out = np.full(case.n, SENT, np.uint32)
        sp = _host_spans(case, cin, out)
        with raw.small_max(case.small_max):
            if how == "batch":
                _lib.check(_lib.lib.crc32c_batch(ctypes.byref(sp), 0, None), "batch")
            else:
                job = ctypes.c_void_p()
                _lib.check(_lib.lib.crc32c_batch_submit(ctypes.byref(sp), 0, ctypes.byref(job)), "submit")
                _lib.check(_lib.lib.crc32c_batch_wait(job), "wait")
        np.testing.assert_array_equal(out, case.expected(cin is not None), err_msg=f"{case.name} {how}")


# ---------------------------------------------------------------------------
# K5's second round
# ---------------------------------------------------------------------------
def test_k5_second_round(torch):
    """n = 64 W + 65 spans, W the waves of K5's full grid (16 a CU): runs of 64
    images, one per wave in the first round, and a second round of one whole
    run and one image, so run_start(1) and the round-robin deal are used.
    4133-byte spans back to back (about 1.1 GB on 256 CUs), generated on the
    device and copied to the host once for the oracle."""
    if torch.cuda.mem_get_info()[0] < 4 * GiB:
        pytest.skip("needs 4 GiB of free device memory")
    t0 = time.perf_counter()
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    L = 4133
    n = 64 * 16 * cus + 65
    size = (n - 1) * L + L
    g = torch.Generator(device="cuda").manual_seed(4133)
    data = torch.randint(0, 256, (size + PAD,), dtype=torch.uint8, device="cuda", generator=g)
    cin = np.random.default_rng(4133).integers(0, 2**32, n, dtype=np.uint64).astype(np.uint32)
    dcin = _d(torch, cin, np.int32)
    got = [_device_call(torch, data.data_ptr(), size, n, L, L, None, c, 0) for c in (None, dcin)]
    t1 = time.perf_counter()
    host = data[:size].cpu().numpy()
    offs = np.arange(n, dtype=np.uint64) * np.uint64(L)
    parts = np.array_split(np.arange(n), 8)
    for (rc, out), c in zip(got, (None, cin)):
        assert rc == _lib.CRC32C_OK
        with ThreadPoolExecutor(8) as ex:  # (the oracle's C call releases the GIL)
            want = np.concatenate(list(ex.map(
                lambda ix: oracle.batch(host, offs[ix], np.full(ix.size, L, np.uint64), None if c is None else c[ix]),
                parts)))
        bad = np.flatnonzero(out != want)
        assert bad.size == 0, (c is not None, bad.size, bad[:8].tolist(), bad[-8:].tolist())
    print(f"\nk5 second round: {n} spans, device {(t1 - t0) * 1e3:.0f} ms, copy and oracle "
          f"{(time.perf_counter() - t1) * 1e3:.0f} ms")
    del data, host


# ---------------------------------------------------------------------------
# the 2^31 line
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("length,stride,route", sc.LINE_CASES,
                         ids=[f"{r}_len{L}_stride{s}" for L, s, r in sc.LINE_CASES])
def test_stride_around_2_31(torch, length, stride, route):
    """Three spans in an uninitialised buffer of 2 * stride + len bytes, only the
    spans filled: K1 just below 2^31, and past it the routes that take over,
    whose i * stride must stay in 64 bits (the third span starts at or past
    2^32; a 32-bit product would read the first span's bytes again, which
    differ).  The oracle runs over the three spans gathered on the device."""
    if torch.cuda.mem_get_info()[0] < 10 * GiB:
        pytest.skip("needs 10 GiB of free device memory")
    n = sc.LINE_N
    size = (n - 1) * stride + length
    rng = np.random.default_rng(stride % 1000 + length)
    spans = rng.integers(0, 256, (n, length), dtype=np.uint8)
    assert not np.array_equal(spans[0], spans[2])
    data = torch.empty(size + PAD, dtype=torch.uint8, device="cuda")
    for i in range(n):
        data[i * stride:i * stride + length] = torch.from_numpy(spans[i]).cuda()
    cat = torch.cat([data[i * stride:i * stride + length] for i in range(n)]).cpu().numpy()
    np.testing.assert_array_equal(cat, spans.reshape(-1))
    coffs, clens = np.arange(n, dtype=np.uint64) * np.uint64(length), np.full(n, length, np.uint64)
    cin = rng.integers(0, 2**32, n, dtype=np.uint64).astype(np.uint32)
    dcin = _d(torch, cin, np.int32)
    for c, dc in ((None, None), (cin, dcin)):
        rc, got = _device_call(torch, data.data_ptr(), size, n, length, stride, None, dc, 0)
        assert rc == _lib.CRC32C_OK
        np.testing.assert_array_equal(got, oracle.batch(cat, coffs, clens, c), err_msg=f"{route} crc_in={c is not None}")
    del data


# ---------------------------------------------------------------------------
# a buffer one byte short
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["k5_len4133_stride4165", "id_blocks_len4097_stride4129", "id_spans_len4098_stride4097"])
def test_one_byte_short_is_refused(torch, name):
    """base_bytes one less than (n - 1) * stride + len: CRC32C_EINVAL and out
    untouched (the kernels read fixed-stride spans unchecked); the exact size
    runs."""
    case = sc.by_name(name)
    assert case.nbytes == (case.n - 1) * case.stride + case.length
    data = torch.from_numpy(np.concatenate([case.buf, np.full(PAD, bs.FILL, np.uint8)])).cuda()
    rc, got = _device_call(torch, data.data_ptr(), case.nbytes - 1, case.n, case.length, case.stride, None, None,
                           case.small_max)
    assert rc == _lib.CRC32C_EINVAL
    assert (got == SENT).all()
    rc, got = _device_call(torch, data.data_ptr(), case.nbytes, case.n, case.length, case.stride, None, None,
                           case.small_max)
    assert rc == _lib.CRC32C_OK
    np.testing.assert_array_equal(got, case.expected(False))

"""The smallest batches on each side of every boundary the host's route
functions draw (memcached_amd/csrc/host_route.h; tests/test_host_route.py
checks the functions themselves on the CPU), run on the GPU with the default
small-batch limit and compared exactly -- every CRC, every ok value, every
byte, nbad and nitems -- with the oracle and the CPU models of
tests/keep_stamped_model.py.  Nothing expected here comes from the library."""
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
from .routes_cases import WBUF
from .routes_cases import items_case as _items_case
from .routes_cases import items_want as _items_want
from .routes_cases import pages_case as _pages_case
from .routes_cases import pages_want as _pages_want
from .routes_cases import short_spans as _short_spans

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch():
    return raw_calls.need_gpu()


def _dev(torch, arr):
    return torch.from_numpy(np.array(arr)).cuda()  # (a writable copy: the fixtures are read-only)


# -- spans ---------------------------------------------------------------------

@pytest.mark.parametrize("n", [8192, 8193])
def test_short_spans_small_and_planned(torch, n):
    """8192 spans: one k_small launch; 8193: the planned path."""
    buf, offs, lens, want = _short_spans()
    out = mc.batch(_dev(torch, buf), offsets=_dev(torch, offs[:n].view(np.int64)),
                   lens=_dev(torch, lens[:n].view(np.int32)))
    np.testing.assert_array_equal(out.cpu().numpy().view(np.uint32), want[:n])
    np.testing.assert_array_equal(mc.batch(buf, offsets=offs[:n], lens=lens[:n]), want[:n])


# 4098 | 4099..4227 | 4228: K5's lengths; 4080 | 4081..4097 | 4098: k_blocks'
@pytest.mark.parametrize("length", [4080, 4081, 4097, 4098, 4099, 4227, 4228])
def test_fixed_length_edges(torch, length):
    """8193 spans of one length given by offsets, all at the same alignment
    mod 128 (the spans overlap: they lie 128 B apart), at every 16th of the
    128 alignments, and at eight more that lie 17 apart, so that the offset in
    a 16-B piece varies too."""
    n = 8193
    buf = np.random.default_rng(length).integers(0, 256, n * 128 + 4228 + 128, dtype=np.uint8)
    d = _dev(torch, buf)
    assert d.data_ptr() % 128 == 0
    for al in sorted(set(range(0, 128, 16)) | set(range(0, 128, 17))):
        offs = np.arange(n, dtype=np.uint64) * 128 + al
        out = mc.batch(d, offsets=_dev(torch, offs.view(np.int64)), length=length)
        want = oracle.batch(buf, offs, np.full(n, length))
        np.testing.assert_array_equal(out.cpu().numpy().view(np.uint32), want, err_msg=f"alignment {al}")


# -- items ---------------------------------------------------------------------

@pytest.mark.parametrize("where", ["device", "host"])
@pytest.mark.parametrize("mode", ["verify", "stamp", "keep"])
@pytest.mark.parametrize("name", ["64", "64+128", "4095", "4096"])
def test_item_routes(torch, name, mode, where):
    buf, offs = _items_case(name)
    w_buf, w_ok, w_bad = _items_want(name, mode)
    assert 0 < w_bad < offs.size
    b = _dev(torch, buf) if where == "device" else buf.copy()
    o = _dev(torch, offs.view(np.int64)) if where == "device" else offs
    if mode == "verify":
        ok, nbad = mc.verify_items(b, o)
    else:
        ok, nbad = mc.stamp_items(b, o, keep_stamped=mode == "keep")
    if where == "device":
        torch.cuda.synchronize()
        b, ok = b.cpu().numpy(), ok.cpu().numpy()
    assert nbad == w_bad
    np.testing.assert_array_equal(ok, w_ok)
    np.testing.assert_array_equal(b, w_buf)


# -- pages ---------------------------------------------------------------------

def _pages_call(torch, fn, buf, cap, where, flags=0):
    """One direct call of crc32c_verify_pages / crc32c_stamp_pages with result
    arrays of cap entries: (rc, nitems, nbad, offsets, ok, the buffer after)."""
    nitems, nbad = ctypes.c_uint64(1 << 60), ctypes.c_uint64(1 << 60)
    if where == "device":
        b = _dev(torch, buf)
        offs = torch.full((cap + 1,), -1, dtype=torch.int64, device="cuda")
        ok = torch.full((cap + 1,), 77, dtype=torch.uint8, device="cuda")
        rc = fn(b.data_ptr(), b.numel(), WBUF, offs.data_ptr() if cap else None, ok.data_ptr() if cap else None, cap,
                ctypes.byref(nitems), ctypes.byref(nbad), flags | _lib.CRC32C_DEVICE,
                torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        b, offs, ok = b.cpu().numpy(), offs.cpu().numpy().view(np.uint64), ok.cpu().numpy()
    else:
        b = buf.copy()
        offs, ok = np.full(cap + 1, 2 ** 64 - 1, np.uint64), np.full(cap + 1, 77, np.uint8)
        rc = fn(b.ctypes.data, b.size, WBUF, offs.ctypes.data if cap else None, ok.ctypes.data if cap else None, cap,
                ctypes.byref(nitems), ctypes.byref(nbad), flags, None)
    assert offs[cap] == 2 ** 64 - 1 and ok[cap] == 77  # nothing written past cap
    return rc, nitems.value, nbad.value, offs[:cap], ok[:cap], b


@pytest.mark.parametrize("where", ["device", "host"])
@pytest.mark.parametrize("cap_kind", ["zero", "short", "full"])
@pytest.mark.parametrize("nwbufs", [1, 5])
def test_page_routes(torch, nwbufs, cap_kind, where):
    """One wbuf (k_small) and five (K5 on the device, the planned path for a
    host stamp's staged images): the calls find the model walk's items; a
    verify with cap 0 only counts, a stamp (keeping carried CRCs, then plain)
    stamps whatever cap is; the first min(cap, nitems) offsets and flags are
    written, nbad covers every item."""
    buf, walked = _pages_case(nwbufs)
    v_ok, (s_buf, s_ok, s_bad), (p_buf, p_ok, p_bad) = _pages_want(nwbufs)
    n = walked.size
    assert n == nwbufs * (WBUF // 4165) and 0 < s_bad < n
    cap = {"zero": 0, "short": n - 3, "full": n + 2}[cap_kind]
    k = min(cap, n)
    rc, nitems, nbad, offs, ok, after = _pages_call(torch, _lib.lib.crc32c_verify_pages, buf, cap, where)
    assert rc == 0 and nitems == n
    assert nbad == (0 if cap == 0 else int((v_ok == 0).sum()))
    np.testing.assert_array_equal(offs[:k], walked[:k])
    np.testing.assert_array_equal(ok[:k], v_ok[:k])
    np.testing.assert_array_equal(after, buf)
    rc, s_nitems, nbad, s_offs, ok, after = _pages_call(torch, _lib.lib.crc32c_stamp_pages, buf, cap, where,
                                                        _lib.CRC32C_KEEP_STAMPED)
    assert rc == 0 and s_nitems == nitems and nbad == s_bad
    np.testing.assert_array_equal(s_offs[:k], offs[:k])
    np.testing.assert_array_equal(ok[:k], s_ok[:k])
    np.testing.assert_array_equal(after, s_buf)
    rc, p_nitems, nbad, p_offs, ok, after = _pages_call(torch, _lib.lib.crc32c_stamp_pages, buf, cap, where)
    assert rc == 0 and p_nitems == nitems and nbad == p_bad == 0
    np.testing.assert_array_equal(p_offs[:k], offs[:k])
    np.testing.assert_array_equal(ok[:k], p_ok[:k])
    np.testing.assert_array_equal(after, p_buf)

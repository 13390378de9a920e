"""The device side of memcached_amd/crc32c.py (tests/test_python_face.py pins
the host side without a GPU): every batch wrapper called once with numpy
inputs and once with device tensors gives the same answer element for element,
and that answer is the CPU model's (the oracle's CRCs; nothing from the
library).  Also which stream a device call is enqueued on, and the two-call
capacity retry of verify_pages on the device.

One buffer serves every test: three 4 KiB wbufs of about ten short images
each, stamped with the oracle's CRCs, one image with a flipped value byte."""
import numpy as np
import pytest

try:  # GPU processes load torch (and its HIP runtime) before libmcrc32c.so
    import torch as _torch  # noqa: F401
except ImportError:
    pass

from memcached_amd import _lib, layout
from memcached_amd import crc32c as mc

from . import chain_cases as cc
from . import copy_items_model as cm
from . import keep_stamped_model as ks
from . import oracle
from . import raw_calls
from . import salvage_cases as sc
from . import salvage_model as sm

pytestmark = pytest.mark.gpu

W = 4096
FLIPPED = 4


@pytest.fixture(scope="module")
def torch():
    return raw_calls.need_gpu()


@pytest.fixture(scope="module")
def data():
    """(buffer, item offsets), both read-only: the in-place calls get copies."""
    rng = np.random.default_rng(20)
    items = [layout.make_item(b"k%03d" % i, rng.integers(0, 256, int(rng.integers(200, 450)), dtype=np.uint8).tobytes(),
                              cas=i + 1, client_flags=i % 3) for i in range(45)]
    buf, offs = layout.pack_wbufs(items, W)
    buf, offs = buf[:3 * W].copy(), offs[offs < 3 * W]
    layout.store_crcs(buf, offs, [oracle.item_crc(buf, o) for o in offs])
    buf[int(offs[FLIPPED]) + 70] ^= 0x40  # inside the value (it starts at 61 or 65)
    assert offs[-1] >= 2 * W and 25 <= offs.size <= 36
    buf.setflags(write=False)
    offs.setflags(write=False)
    return buf, offs


def _dev(torch, arr):
    """A device copy; unsigned 32- and 64-bit arrays travel as their signed twins."""
    arr = np.array(arr)
    twin = {np.dtype(np.uint64): np.int64, np.dtype(np.uint32): np.int32}.get(arr.dtype)
    return torch.from_numpy(arr.view(twin) if twin else arr).cuda()


def _host(t, dtype=None):
    a = t.cpu().numpy()
    return a.view(dtype) if dtype else a


class _Recorder:
    """The real library, noting each call's name and arguments on the way."""

    def __init__(self, lib):
        self.lib, self.calls = lib, []

    def __getattr__(self, name):
        f = getattr(self.lib, name)

        def call(*args):
            self.calls.append((name, args))
            return f(*args)
        return call


@pytest.fixture
def recorder(monkeypatch):
    r = _Recorder(mc.lib)
    monkeypatch.setattr(mc, "lib", r)
    return r


SPAN_OFFS = np.array([1, 100, 4096, 5000, 12000], np.uint64)
SPAN_LENS = np.array([0, 33, 4096, 1000, 288], np.uint32)  # the last one ends with the buffer


def test_batch(torch, data):
    buf, _ = data
    want = oracle.batch(buf, SPAN_OFFS, SPAN_LENS)
    host = mc.batch(buf, offsets=SPAN_OFFS, lens=SPAN_LENS)
    dev = mc.batch(_dev(torch, buf), offsets=_dev(torch, SPAN_OFFS), lens=_dev(torch, SPAN_LENS))
    assert host.dtype == np.uint32 and dev.dtype == torch.int32
    np.testing.assert_array_equal(host, want)
    np.testing.assert_array_equal(_host(dev, np.uint32), want)


def test_verify_items(torch, data):
    buf, offs = data
    want = ks.expected_verify(buf, offs, W)
    assert want[FLIPPED] == 0 and want.sum() == offs.size - 1
    h_ok, h_bad = mc.verify_items(buf, offs, region_bytes=W)
    d_ok, d_bad = mc.verify_items(_dev(torch, buf), _dev(torch, offs), region_bytes=W)
    assert h_bad == d_bad == 1 and d_ok.dtype == torch.uint8
    np.testing.assert_array_equal(h_ok, want)
    np.testing.assert_array_equal(_host(d_ok), want)


def _fresh(data):
    """The buffer with two images' CRC fields zeroed (not stamped yet)."""
    buf, offs = data
    buf = buf.copy()
    for i in (0, 17):
        buf[int(offs[i]) + 28:int(offs[i]) + 32] = 0
    return buf


@pytest.mark.parametrize("keep", [False, True])
def test_stamp_items(torch, data, keep):
    offs = data[1]
    buf = _fresh(data)
    w_buf, w_ok, w_bad = ks.expected_stamp(buf, offs, W, keep)
    assert w_bad == (1 if keep else 0) and set(w_ok.tolist()) == ({0, 1, 2} if keep else {1})
    h_buf, d_buf = buf.copy(), _dev(torch, buf)
    h_ok, h_bad = mc.stamp_items(h_buf, offs, region_bytes=W, keep_stamped=keep)
    d_ok, d_bad = mc.stamp_items(d_buf, _dev(torch, offs), region_bytes=W, keep_stamped=keep)
    assert h_bad == d_bad == w_bad
    np.testing.assert_array_equal(h_ok, w_ok)
    np.testing.assert_array_equal(_host(d_ok), w_ok)
    np.testing.assert_array_equal(h_buf, w_buf)
    np.testing.assert_array_equal(_host(d_buf), w_buf)


def test_stamp_pages(torch, data):
    offs = data[1]
    buf = _fresh(data)
    np.testing.assert_array_equal(ks.host_walk(buf, W), offs)
    w_buf, w_ok, w_bad = ks.expected_stamp(buf, offs, W, True)
    h_buf, d_buf = buf.copy(), _dev(torch, buf)
    h_offs, h_ok, h_bad = mc.stamp_pages(h_buf, W, keep_stamped=True)
    d_offs, d_ok, d_bad = mc.stamp_pages(d_buf, W, keep_stamped=True)
    assert h_bad == d_bad == w_bad == 1 and d_offs.dtype == torch.int64 and d_ok.dtype == torch.uint8
    np.testing.assert_array_equal(h_offs, offs)
    np.testing.assert_array_equal(_host(d_offs, np.uint64), offs)
    np.testing.assert_array_equal(h_ok, w_ok)
    np.testing.assert_array_equal(_host(d_ok), w_ok)
    np.testing.assert_array_equal(h_buf, w_buf)
    np.testing.assert_array_equal(_host(d_buf), w_buf)


def test_verify_pages_and_its_second_call_on_the_device(torch, data, recorder):
    """~30 images in 12 KiB are more than the device's first guess of the
    capacity (images of 1 KiB: nbytes // 1024 + one per wbuf), so the device
    call is made twice, the second time with the exact count; the host call
    takes the walk's upper bound at once.  Both return the whole list."""
    buf, offs = data
    guess = buf.size // 1024 + 3
    assert offs.size > guess
    want_offs, want_ok = sc.walk_lists(buf, W)
    np.testing.assert_array_equal(want_offs, offs)
    np.testing.assert_array_equal(want_ok, ks.expected_verify(buf, offs, W))
    h_offs, h_ok, h_bad = mc.verify_pages(buf, W)
    assert [(c[0], c[1][5]) for c in recorder.calls] == [("crc32c_verify_pages", buf.size // 50 + 3)]
    recorder.calls.clear()
    d_offs, d_ok, d_bad = mc.verify_pages(_dev(torch, buf), W)
    assert [(c[0], c[1][5]) for c in recorder.calls] == [("crc32c_verify_pages", guess),
                                                        ("crc32c_verify_pages", offs.size)]
    assert h_bad == d_bad == 1 and d_offs.dtype == torch.int64 and d_ok.dtype == torch.uint8
    np.testing.assert_array_equal(h_offs, offs)
    np.testing.assert_array_equal(_host(d_offs, np.uint64), offs)
    np.testing.assert_array_equal(h_ok, want_ok)
    np.testing.assert_array_equal(_host(d_ok), want_ok)


@pytest.mark.parametrize("with_lists", [True, False])
def test_salvage_pages(torch, data, with_lists):
    """A zeroed nkey ends the second wbuf's walk early: the images behind it
    (and, with the lists, the one with the flipped byte not) are found."""
    buf, offs = data
    buf = buf.copy()
    hit = int(np.searchsorted(offs, W)) + 2
    buf[int(offs[hit]) + layout.NKEY_OFF] = 0
    walked, ok = sc.walk_lists(buf, W) if with_lists else (None, None)
    found, scanned, ncand, _work = sm.salvage_fast(buf, W, walked, ok)
    behind = [int(o) for o in offs[hit + 1:] if o < 2 * W]
    assert len(behind) >= 3 and set(behind) <= set(found) and int(offs[FLIPPED]) not in found
    h_offs, h_info = mc.salvage_pages(buf, W, walked, ok)
    d_lists = (_dev(torch, walked), _dev(torch, ok)) if with_lists else (None, None)
    d_offs, d_info = mc.salvage_pages(_dev(torch, buf), W, *d_lists)
    assert h_info == d_info == {"scanned": scanned, "ncand": ncand} and d_offs.dtype == torch.int64
    assert h_offs.tolist() == found and _host(d_offs, np.uint64).tolist() == found


def test_copy_items(torch, data):
    buf, offs = data
    soffs = offs[::2]  # the image with the flipped byte among them
    sizes = np.array([layout.ntotal_of(buf, int(o)) for o in soffs], np.uint64)
    doffs = np.concatenate([[3], 3 + np.cumsum(sizes)[:-1]]).astype(np.uint64)
    dst_init = np.full(int(doffs[-1] + sizes[-1]) + 5, 0xA5, np.uint8)
    w_dst, w_ok, w_bad, w_erange = cm.expected_copy(buf, soffs, W, dst_init, doffs)
    assert not w_erange and w_bad == 1 and w_ok[FLIPPED // 2] == cm.DAMAGED
    h_dst, d_dst = dst_init.copy(), _dev(torch, dst_init)
    h_ok, h_bad = mc.copy_items(buf, soffs, h_dst, doffs, region_bytes=W)
    d_ok, d_bad = mc.copy_items(_dev(torch, buf), _dev(torch, soffs), d_dst, _dev(torch, doffs), region_bytes=W)
    assert h_bad == d_bad == 1 and d_ok.dtype == torch.uint8
    np.testing.assert_array_equal(h_ok, w_ok)
    np.testing.assert_array_equal(_host(d_ok), w_ok)
    np.testing.assert_array_equal(h_dst, w_dst)
    np.testing.assert_array_equal(_host(d_dst), w_dst)


def test_batch_chains(torch, data):
    buf, _ = data
    offs = np.array([5, 300, 301, 4096, 9000, 12280], np.uint64)
    lens = np.array([295, 1, 3795, 4904, 0, 8], np.uint32)
    first = np.array([0, 3, 6], np.uint64)  # 2 chains of 3 iovs
    want = cc.expected_chains(buf, offs, lens, first)
    host = mc.batch_chains(buf, offs, lens, first)
    dev = mc.batch_chains(_dev(torch, buf), _dev(torch, offs), _dev(torch, lens), _dev(torch, first))
    assert host.dtype == np.uint32 and dev.dtype == torch.int32 and dev.shape == (2,)
    np.testing.assert_array_equal(host, want)
    np.testing.assert_array_equal(_host(dev, np.uint32), want)


def test_stream_choice(torch, data, recorder):
    """A device call goes to the caller's stream, else to torch's current
    stream of the buffer's device, with the same results either way."""
    buf, offs = data
    d_buf, d_offs = _dev(torch, buf), _dev(torch, offs)
    d_so, d_sl = _dev(torch, SPAN_OFFS), _dev(torch, SPAN_LENS)
    want_ok = ks.expected_verify(buf, offs, W)
    want_crc = oracle.batch(buf, SPAN_OFFS, SPAN_LENS)
    torch.cuda.synchronize()  # the inputs are in place whichever stream reads them
    s = torch.cuda.Stream()
    current = torch.cuda.current_stream().cuda_stream
    assert s.cuda_stream != current

    def both(stream=None):
        ok, nbad = mc.verify_items(d_buf, d_offs, region_bytes=W, stream=stream)
        crc = mc.batch(d_buf, offsets=d_so, lens=d_sl, stream=stream)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(_host(ok), want_ok)
        np.testing.assert_array_equal(_host(crc, np.uint32), want_crc)
        assert nbad == 1
        streams = [(name, args[-1]) for name, args in recorder.calls]
        assert all(args[-2] & _lib.CRC32C_DEVICE for _, args in recorder.calls)
        recorder.calls.clear()
        return streams

    assert both() == [("crc32c_verify_items", current), ("crc32c_batch", current)]
    with torch.cuda.stream(s):
        assert both() == [("crc32c_verify_items", s.cuda_stream), ("crc32c_batch", s.cuda_stream)]
    assert both(s.cuda_stream) == [("crc32c_verify_items", s.cuda_stream), ("crc32c_batch", s.cuda_stream)]

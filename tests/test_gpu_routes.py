"""The smallest batches on each side of every boundary the host's route
functions draw (memcached_amd/csrc/host_route.h; tests/test_host_route.py
checks the functions themselves on the CPU), run on the GPU with the default
small-batch limit and compared exactly -- every CRC, every ok value, every
byte, nbad and nitems -- with the oracle and the CPU models of
tests/keep_stamped_model.py.  Nothing expected here comes from the library."""
import ctypes
import functools

import numpy as np
import pytest

try:  # GPU processes load torch (and its HIP runtime) before libmcrc32c.so
    import torch as _torch  # noqa: F401
except ImportError:
    pass

from memcached_amd import _lib, layout
from memcached_amd import crc32c as mc

from . import keep_stamped_model as model
from . import oracle

pytestmark = pytest.mark.gpu

MiB = 1 << 20


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available(), "GPU tests need a visible MI355X"
    assert mc.gpu_count() >= 1, "libmcrc32c.so sees no gfx950 device"
    return t


def _dev(torch, arr):
    return torch.from_numpy(np.array(arr)).cuda()  # (a writable copy: the fixtures are read-only)


# -- spans ---------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _short_spans():
    """8193 spans of 1..300 B at unaligned offsets of a buffer under 8 MiB, and
    their CRCs."""
    rng = np.random.default_rng(811)
    lens = rng.integers(1, 301, 8193).astype(np.uint32)
    offs = (np.cumsum(lens + rng.integers(0, 40, 8193)) - lens + 3).astype(np.uint64)
    buf = rng.integers(0, 256, int(offs[-1]) + 300 + 5, dtype=np.uint8)
    assert buf.size <= 8 * MiB and len(set((offs % 16).tolist())) == 16
    return buf, offs, lens, oracle.batch(buf, offs, lens)


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

def _mixed(items, rng, pad_to=None, nokey=True):
    """The images back to back (in a buffer of pad_to bytes): by i % 3 fresh,
    carried, carried; of every 500 (at least 5) carried images one with a
    flipped data bit, and two images with nkey = 0."""
    offs = np.cumsum([0] + [len(im) for im in items[:-1]]).astype(np.uint64)
    raw = b"".join(bytes(im) for im in items)
    buf = np.zeros(pad_to or len(raw), np.uint8)
    buf[:len(raw)] = np.frombuffer(raw, np.uint8)
    n = len(items)
    carried = np.array([i for i in range(n) if i % 3])
    crcs = np.array([oracle.item_crc(buf, o) for o in offs[carried]], np.uint32)
    assert (crcs != 0).all()
    layout.store_crcs(buf, offs[carried], crcs)
    for i in rng.choice(carried, max(5, n // 500), replace=False).tolist():
        o = int(offs[i])
        buf[o + 48 + int(rng.integers(0, layout.ntotal_of(buf, o) - 48))] ^= 1 << int(rng.integers(0, 8))
    for i in (7, n - 2) if nokey else ():
        buf[int(offs[i]) + layout.NKEY_OFF] = 0
    buf.flags.writeable = False
    return buf, offs


@functools.lru_cache(maxsize=None)
def _items_case(name):
    rng = np.random.default_rng(len(name) * 1000 + sum(name.encode()))
    if name.startswith("64"):  # 64 images in exactly 8 MiB (small) or 128 B more (planned)
        items = [layout.make_item(b"r%05d" % i,
                                  rng.integers(0, 256, int(rng.integers(0, 9000)), dtype=np.uint8).tobytes(), cas=i + 1)
                 for i in range(64)]
        buf, offs = _mixed(items, rng, pad_to=8 * MiB + (128 if name == "64+128" else 0))
    else:  # 4095 (planned) or 4096 (K5 with a fallback list) images of 4165 B, every 400th of another size
        n = int(name)
        vals = [4096 if i % 400 else int(rng.integers(100, 9000)) for i in range(n)]
        items = [layout.make_item(b"key%07d" % i, rng.integers(0, 256, v, dtype=np.uint8).tobytes(), cas=i + 1)
                 for i, v in enumerate(vals)]
        assert len(items[1]) == 4165
        buf, offs = _mixed(items, rng)
        assert buf.size > 8 * MiB
    return buf, offs


@functools.lru_cache(maxsize=None)
def _items_want(name, mode):
    buf, offs = _items_case(name)
    if mode == "verify":
        ok = model.expected_verify(buf, offs, 0)
        return buf, ok, int((ok == 0).sum())
    return model.expected_stamp(buf, offs, 0, keep=mode == "keep")


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

WBUF = 4 * MiB


@functools.lru_cache(maxsize=None)
def _pages_case(nwbufs):
    """nwbufs 4 MiB wbufs of 4165-B images (1007 each: one wbuf is a small
    batch, five are past 4096 items) with zero tails, mixed as _mixed makes
    them but for the nkey = 0 images (they would end their wbuf's walk)."""
    rng = np.random.default_rng(nwbufs)
    per = WBUF // 4165
    buf = np.zeros(nwbufs * WBUF, np.uint8)
    for w in range(nwbufs):
        items = [layout.make_item(b"key%07d" % (w * per + i), rng.integers(0, 256, 4096, dtype=np.uint8).tobytes(),
                                  cas=i + 1) for i in range(per)]
        part, _ = _mixed(items, rng, nokey=False)
        buf[w * WBUF:w * WBUF + part.size] = part
    walked = model.host_walk(buf, WBUF)
    assert walked.size == nwbufs * per and (nwbufs == 1) == (walked.size <= 4096)
    buf.flags.writeable = False
    return buf, walked


@functools.lru_cache(maxsize=None)
def _pages_want(nwbufs):
    buf, walked = _pages_case(nwbufs)
    v_ok = model.expected_verify(buf, walked, WBUF)
    return v_ok, model.expected_stamp(buf, walked, WBUF, keep=True), model.expected_stamp(buf, walked, WBUF, keep=False)


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

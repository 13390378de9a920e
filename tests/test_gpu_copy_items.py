"""crc32c_copy_items on the GPU: item images copied to their new places and
verified from the same loads, through every route (device; host with both
buffers page-locked; pageable host; source page-locked and destination
pageable).  Every comparison is exact -- the whole of dst byte for byte (it is
pre-filled with 0xa5, so a stray or a missing byte shows), src unchanged, every
ok value, nbad and the return code -- against the CPU model of
tests/copy_items_model.py (the oracle's CRCs; nothing from the library)."""
import ctypes

import numpy as np
import pytest

try:  # GPU processes load torch (and its HIP runtime) before libmcrc32c.so
    import torch as _torch  # noqa: F401
except ImportError:
    pass

from memcached_amd import _lib, layout
from memcached_amd import crc32c as mc

from . import copy_items_model as model
from . import raw_calls
from .copy_cases import WBUF, mixed_case
from .copy_cases import stamp_all as _stamp_all

pytestmark = pytest.mark.gpu

ROUTES = ["device", "pinned", "pageable"]


@pytest.fixture(scope="module")
def torch():
    return raw_calls.need_gpu()


def _dev(torch, arr):
    return torch.from_numpy(np.array(arr)).cuda()  # (a writable copy: the fixtures are read-only)


class _Pinned:
    """A crc32c_host_alloc buffer holding a copy of `data`, as a numpy array."""

    def __init__(self, data):
        self.p = _lib.lib.crc32c_host_alloc(max(data.size, 1))
        assert self.p
        self.arr = np.ctypeslib.as_array((ctypes.c_uint8 * data.size).from_address(self.p))
        self.arr[:] = data

    def free(self):
        self.arr = None
        _lib.lib.crc32c_host_free(self.p)


def _call(src_p, src_n, region, so_p, dst_p, dst_n, do_p, n, ok_p, nbad, flags, stream=None):
    return _lib.lib.crc32c_copy_items(src_p, src_n, region, so_p, dst_p, dst_n, do_p, n, ok_p,
                                      ctypes.byref(nbad) if nbad is not None else None, flags, stream)


def _copy(torch, route, src, soffs, dst_init, doffs, wbuf, cflags64=False):
    """One crc32c_copy_items call over copies of src and dst_init on `route`:
    (dst after, ok, nbad, return code); src is checked unchanged here."""
    soffs = np.ascontiguousarray(soffs, np.uint64)
    doffs = np.ascontiguousarray(doffs, np.uint64)
    n = soffs.size
    nbad = ctypes.c_uint64(0)
    fl = _lib.CRC32C_CFLAGS64 if cflags64 else 0
    if route == "device":
        s, d = _dev(torch, src), _dev(torch, dst_init)
        so, do = _dev(torch, soffs.view(np.int64)), _dev(torch, doffs.view(np.int64))
        ok = torch.full((n,), 9, dtype=torch.uint8, device="cuda")
        rc = _call(s.data_ptr(), s.numel(), wbuf, so.data_ptr(), d.data_ptr(), d.numel(), do.data_ptr(), n,
                   ok.data_ptr(), nbad, _lib.CRC32C_DEVICE | fl, None)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(s.cpu().numpy(), src)
        return d.cpu().numpy(), ok.cpu().numpy(), nbad.value, rc
    pins = []
    try:
        if route in ("pinned", "src_pinned"):
            pins.append(_Pinned(src))
            s = pins[-1].arr
        else:
            s = src.copy()
        if route == "pinned":
            pins.append(_Pinned(dst_init))
            d = pins[-1].arr
        else:
            d = dst_init.copy()
        ok = np.full(n, 9, np.uint8)
        rc = _call(s.ctypes.data, s.size, wbuf, soffs.ctypes.data, d.ctypes.data, d.size, doffs.ctypes.data, n,
                   ok.ctypes.data, nbad, fl)
        np.testing.assert_array_equal(s, src)
        return d.copy(), ok, nbad.value, rc
    finally:
        for p in pins:
            p.free()


def _check(got, want):
    (g_dst, g_ok, g_bad, g_rc), (w_dst, w_ok, w_bad, w_erange) = got, want
    assert g_rc == (_lib.CRC32C_ERANGE if w_erange else _lib.CRC32C_OK)
    np.testing.assert_array_equal(g_ok, w_ok)
    assert g_bad == w_bad
    np.testing.assert_array_equal(g_dst, w_dst)


# -- case 1: every alignment pair, block edges ----------------------------------

def _value_len(i):
    k = i // 3
    return (k % 41, 4020 + k % 101, 8110 + k % 101)[i % 3]


@pytest.fixture(scope="module")
def aligned():
    """528 images; image i starts at i % 16 mod 16 in the source (every image's
    ITEM_ntotal is 1 mod 16, set by its key length, with one filler image
    behind a wbuf switch) and goes to the next free destination offset that is
    (i // 16) % 16 mod 16.  Value lengths cycle through 0..40, 4020..4120 and
    8110..8210 (one, two and three blocks, both sides of each block edge), with
    one image of 70 000 and one of 300 000 bytes."""
    n = 528
    rng = np.random.default_rng(1616)
    vlens = [_value_len(i) for i in range(n)]
    vlens[100], vlens[333] = 70_000, 300_000
    wbufs, cur, used, offs = [], bytearray(WBUF), 0, []
    for i, v in enumerate(vlens):
        key = (b"k%05d" % i + b"x" * 16)[:6 + (-v) % 16]
        img = layout.make_item(key, rng.integers(0, 256, v, dtype=np.uint8).tobytes(), cas=i + 1)
        assert len(img) % 16 == 1
        if used + len(img) + 80 > WBUF:
            wbufs.append(cur)
            cur, used = bytearray(WBUF), 0
        need = (i - used) % 16
        if need:  # a filler image (not in the list) whose ITEM_ntotal is `need` mod 16
            fill = layout.make_item(b"filler", b"f" * ((need - 65) % 16 + 16), cas=7)
            assert len(fill) % 16 == need
            cur[used:used + len(fill)] = fill
            used += len(fill)
        cur[used:used + len(img)] = img
        offs.append(len(wbufs) * WBUF + used)
        used += len(img)
    wbufs.append(cur)
    src = np.frombuffer(b"".join(wbufs), np.uint8).copy()
    offs = np.array(offs, np.uint64)
    _stamp_all(src, offs)
    for i in range(5, n, 37):  # damage in the image's last byte (the tail piece) or in its key (the first block)
        o, nt = int(offs[i]), layout.ntotal_of(src, int(offs[i]))
        src[o + (nt - 1 if i % 2 else 57)] ^= 0x20
    doffs, at = [], 0
    for i, o in enumerate(offs.tolist()):
        at += ((i // 16) % 16 - at) % 16
        doffs.append(at)
        at += layout.ntotal_of(src, o)
    src.flags.writeable = False
    dst_init = np.full((at + WBUF - 1) // WBUF * WBUF, 0xa5, np.uint8)
    dst_init.flags.writeable = False
    return src, offs, dst_init, np.array(doffs, np.uint64), vlens


def test_aligned_fixture_covers_every_pair(aligned):
    src, offs, _, doffs, vlens = aligned
    assert offs.size >= 512
    np.testing.assert_array_equal(offs % 16, np.arange(offs.size) % 16)
    np.testing.assert_array_equal(doffs % 16, (np.arange(offs.size) // 16) % 16)
    pairs = set(zip((offs % 16).tolist(), (doffs % 16).tolist()))
    assert len(pairs) == 256
    for lo, hi in ((0, 40), (4020, 4120), (8110, 8210)):
        cls = {(int(s % 16), int(d % 16)) for s, d, v in zip(offs, doffs, vlens) if lo <= v <= hi}
        assert len(cls) >= 16, (lo, hi, len(cls))
    assert 70_000 in vlens and 300_000 in vlens


@pytest.mark.parametrize("route", ROUTES)
def test_alignment_pairs_and_block_edges(torch, aligned, route):
    src, offs, dst_init, doffs, _ = aligned
    want = model.expected_copy(src, offs, WBUF, dst_init, doffs)
    assert not want[3] and want[2] == len(range(5, offs.size, 37)) and set(want[1].tolist()) == {1, 3}
    _check(_copy(torch, route, src, offs, dst_init, doffs, WBUF), want)


# -- case 2: verdicts ------------------------------------------------------------

@pytest.fixture(scope="module")
def mixed():
    return mixed_case()


@pytest.mark.parametrize("route", ROUTES + ["src_pinned"])
def test_verdicts(torch, mixed, route):
    src, soffs, doffs, used, damaged, dropped = mixed
    # dst ends one byte short of the last sane image: that image is dropped and reported
    last = 899
    assert last not in damaged | dropped
    dst_init = np.full(used - 1, 0xa5, np.uint8)
    want = model.expected_copy(src, soffs, WBUF, dst_init, doffs)
    w_dst, w_ok, w_bad, w_erange = want
    assert w_erange and w_ok[last] == 0 and (w_dst[int(doffs[last]):] == 0xa5).all()
    assert set(np.flatnonzero(w_ok == 3).tolist()) == damaged
    assert set(np.flatnonzero(w_ok == 0).tolist()) == dropped | {last}
    assert w_bad == int((w_ok != 1).sum()) == len(damaged) + len(dropped) + 1
    _check(_copy(torch, route, src, soffs, dst_init, doffs, WBUF), want)
    # with room for it, the same call copies it too and returns CRC32C_OK
    full = np.full(used + 3, 0xa5, np.uint8)
    want = model.expected_copy(src, soffs, WBUF, full, doffs)
    assert not want[3] and want[1][last] == 1 and want[2] == w_bad - 1
    _check(_copy(torch, route, src, soffs, full, doffs, WBUF), want)


# -- case 3: round trip ----------------------------------------------------------

def test_round_trip_verify_and_keep_stamped_walk(torch, mixed):
    src, soffs, doffs, used, damaged, dropped = mixed
    dst_init = np.full(used, 0xa5, np.uint8)
    want = model.expected_copy(src, soffs, WBUF, dst_init, doffs)
    got = _copy(torch, "device", src, soffs, dst_init, doffs, WBUF)
    _check(got, want)
    written = got[1] != 0
    ok, nbad = mc.verify_items(_dev(torch, got[0]), _dev(torch, doffs[written].view(np.int64)))
    np.testing.assert_array_equal(ok.cpu().numpy(), (got[1][written] == 1).astype(np.uint8))
    assert nbad == len(damaged)
    # a destination wbuf as compaction fills it: only images that can be written,
    # packed back to back inside zeroed wbufs, then the submit hook's walk
    keep = np.flatnonzero(want[1] != 0)
    k_soffs, k_doffs, at = soffs[keep], [], 0
    for o in k_soffs.tolist():
        nt = layout.ntotal_of(src, o)
        if at % WBUF + nt > WBUF:
            at = (at // WBUF + 1) * WBUF
        k_doffs.append(at)
        at += nt
    k_doffs = np.array(k_doffs, np.uint64)
    zeroed = np.zeros((at + WBUF - 1) // WBUF * WBUF, np.uint8)
    w2 = model.expected_copy(src, k_soffs, WBUF, zeroed, k_doffs)
    g2 = _copy(torch, "device", src, k_soffs, zeroed, k_doffs, WBUF)
    _check(g2, w2)
    d = _dev(torch, g2[0])
    w_offs, w_ok, w_nbad = mc.stamp_pages(d, WBUF, keep_stamped=True)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(w_offs.cpu().numpy().astype(np.uint64), k_doffs)
    np.testing.assert_array_equal(w_ok.cpu().numpy(), np.where(w2[1] == 1, _lib.CRC32C_ITEM_KEPT, 0))
    assert w_nbad == len(damaged) == int((w2[1] == 3).sum())
    np.testing.assert_array_equal(d.cpu().numpy(), g2[0])  # nothing was stamped


# -- case 4: many images, strided groups -----------------------------------------

def test_many_images_strided_groups(torch):
    n, nt = 20_000, 4165
    g = torch.Generator(device="cuda").manual_seed(14)
    d = torch.randint(0, 256, (n * nt + 64,), dtype=torch.uint8, device="cuda", generator=g)
    im = d[:n * nt].view(n, nt)
    # memcached.h:613-636 header: nbytes 4098, it_flags ITEM_CAS, nkey 10 -> ITEM_ntotal 4165; exptime zeroed
    im[:, 28:32] = 0
    im[:, 32:36] = torch.tensor([4098 & 255, 4098 >> 8, 0, 0], dtype=torch.uint8, device="cuda")
    im[:, 38:40] = torch.tensor([2, 0], dtype=torch.uint8, device="cuda")
    im[:, 41] = 10
    offs = np.arange(n, dtype=np.uint64) * nt
    ok, nbad = mc.stamp_items(d, _dev(torch, offs.view(np.int64)))
    assert nbad == 0 and bool(ok.all())
    rescued = np.arange(0, n, 2)
    victims = rescued[17::500]
    assert victims.size == 20
    im[torch.from_numpy(victims).cuda(), 3000] ^= 0x08
    src = d.cpu().numpy()
    soffs = offs[rescued]
    doffs = np.arange(rescued.size, dtype=np.uint64) * nt  # densely packed
    dst_init = np.full(rescued.size * nt + 100, 0xa5, np.uint8)
    want = model.expected_copy(src, soffs, 0, dst_init, doffs)
    assert want[2] == 20 and (np.flatnonzero(want[1] == 3) == np.searchsorted(rescued, victims)).all()
    dd = _dev(torch, dst_init)
    got_ok, got_bad = mc.copy_items(d, _dev(torch, soffs.view(np.int64)), dd, _dev(torch, doffs.view(np.int64)))
    torch.cuda.synchronize()
    _check((dd.cpu().numpy(), got_ok.cpu().numpy(), got_bad, _lib.CRC32C_OK), want)
    np.testing.assert_array_equal(d.cpu().numpy(), src)


# -- case 5: client-flags width --------------------------------------------------

@pytest.mark.parametrize("cfl", [4, 8])
def test_client_flags_width(torch, cfl):
    rng = np.random.default_rng(100 + cfl)
    wbuf = 128 * 1024
    items = [layout.make_item(b"key%07d" % i, rng.integers(0, 256, int(rng.integers(0, 3000)), dtype=np.uint8).tobytes(),
                              cas=i + 1 if i % 5 else None,
                              client_flags=(0x1_0000_0003 if cfl == 8 else 0x3) * (i % 2), cflags_bytes=cfl)
             for i in range(400)]
    src, offs = layout.pack_wbufs(items, wbuf)
    _stamp_all(src, offs, cfl)
    for i in range(0, 400, 25):
        src[int(offs[i]) + 40] ^= 0x01
    doffs, at = [], 3
    for o in offs.tolist():
        doffs.append(at)
        at += layout.ntotal_of(src, o, cfl) + 5
    doffs = np.array(doffs, np.uint64)
    dst_init = np.full(at + 9, 0xa5, np.uint8)
    want = model.expected_copy(src, offs, wbuf, dst_init, doffs, cfl=cfl)
    assert want[2] == 16 and not want[3] and (want[1] != 0).all()
    # (the other width reads other lengths from the same headers: the cases differ)
    other = model.expected_copy(src, offs, wbuf, dst_init, doffs, cfl=12 - cfl)
    assert not np.array_equal(other[0], want[0])
    for route in ("device", "pageable"):
        _check(_copy(torch, route, src, offs, dst_init, doffs, wbuf, cflags64=cfl == 8), want)


# -- case 6: async ---------------------------------------------------------------

def test_async_on_the_current_stream(torch, mixed):
    src, soffs, doffs, used, _, _ = mixed
    dst_init = np.full(used, 0xa5, np.uint8)
    want = model.expected_copy(src, soffs, WBUF, dst_init, doffs)
    s, d = _dev(torch, src), _dev(torch, dst_init)
    so, do = _dev(torch, soffs.view(np.int64)), _dev(torch, doffs.view(np.int64))
    ok = torch.full((soffs.size,), 9, dtype=torch.uint8, device="cuda")
    st = torch.cuda.current_stream()
    rc = _call(s.data_ptr(), s.numel(), WBUF, so.data_ptr(), d.data_ptr(), d.numel(), do.data_ptr(), soffs.size,
               ok.data_ptr(), None, _lib.CRC32C_DEVICE | _lib.CRC32C_ASYNC, ctypes.c_void_p(st.cuda_stream))
    assert rc == _lib.CRC32C_OK
    st.synchronize()
    np.testing.assert_array_equal(ok.cpu().numpy(), want[1])
    np.testing.assert_array_equal(d.cpu().numpy(), want[0])
    np.testing.assert_array_equal(s.cpu().numpy(), src)
    # the next synchronous call reports its own count only
    _check(_copy(torch, "device", src, soffs, dst_init, doffs, WBUF), want)


# -- case 7: argument errors -----------------------------------------------------

@pytest.mark.parametrize("route", ["device", "pageable"])
def test_argument_errors(torch, mixed, route):
    src, soffs, doffs, used, _, _ = mixed
    n = 50
    nbad = ctypes.c_uint64(0)
    if route == "device":
        buf = torch.full((src.size + used,), 0xa5, dtype=torch.uint8, device="cuda")
        buf[:src.size] = _dev(torch, src)
        so, do = _dev(torch, soffs.view(np.int64)), _dev(torch, doffs.view(np.int64))
        ok = torch.full((n,), 9, dtype=torch.uint8, device="cuda")
        base, ptrs, fl = buf.data_ptr(), (so.data_ptr(), do.data_ptr(), ok.data_ptr()), _lib.CRC32C_DEVICE
    else:
        buf = np.full(src.size + used, 0xa5, np.uint8)
        buf[:src.size] = src
        so, do, ok = soffs.copy(), doffs.copy(), np.full(n, 9, np.uint8)
        base, ptrs, fl = buf.ctypes.data, (so.ctypes.data, do.ctypes.data, ok.ctypes.data), 0
    dst = base + src.size

    def call(s=base, sn=src.size, sop=ptrs[0], dp=dst, dn=used, dop=ptrs[1], okp=ptrs[2]):
        return _call(s, sn, WBUF, sop, dp, dn, dop, n, okp, nbad, fl)

    assert call(s=None) == _lib.CRC32C_EINVAL
    assert call(dp=None) == _lib.CRC32C_EINVAL
    assert call(sop=None) == _lib.CRC32C_EINVAL
    assert call(dop=None) == _lib.CRC32C_EINVAL
    assert call(okp=None) == _lib.CRC32C_EINVAL
    # overlapping ranges: dst starting inside src, src reaching into dst, one inside the other
    assert call(dp=dst - 1, dn=used) == _lib.CRC32C_EINVAL
    assert call(sn=src.size + 1) == _lib.CRC32C_EINVAL
    assert call(dp=base + 4096, dn=100) == _lib.CRC32C_EINVAL
    if route == "device":
        torch.cuda.synchronize()
        after, okv = buf.cpu().numpy(), ok.cpu().numpy()
    else:
        after, okv = buf, ok
    np.testing.assert_array_equal(after[:src.size], src)
    assert (after[src.size:] == 0xa5).all() and (okv == 9).all()
    # n == 0 is CRC32C_OK with *nbad = 0
    nbad.value = 5
    assert _call(base, src.size, WBUF, ptrs[0], dst, used, ptrs[1], 0, ptrs[2], nbad, fl) == _lib.CRC32C_OK
    assert nbad.value == 0
    # and the adjacent, non-overlapping ranges are a valid call
    assert call() == _lib.CRC32C_OK

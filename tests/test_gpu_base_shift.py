"""Every entry point with a `base` off the 16-byte grid (tests/base_shift_cases.py
states the rule): the buffer sits at SLACK + s in an allocation filled with
0xA5, the library gets the view that starts there, and every result must
equal the oracle's or the model's for the unshifted buffer and, bit for bit,
the result of the same call at s = 0; after a call that writes, the whole
allocation, slack included, must hold the model's bytes.  Each case runs on
the single-launch route (k_small, the default for up to 8192 spans) and on the
planned path (crc32c_set_small_max(0): k_count, the scans, k_expand, the span
kernels, k_final); the page-recovery calls on the planned path only, their
default route at these sizes being what their own off-grid tests cover.

What these cases caught when they were written: k_count rounded the end of a
whole span's pieces as an offset from base, not as an address, so every case
on the planned path that holds a span of at most 1024 bytes failed at every
shift that is no multiple of 16 (and passed at 16); and k_final took the
caller's out[] word for a kernel's result when a fixed-length batch of
zero-length spans went past the single-launch route, at every shift and at
none (test_chains' zeros_fixed_len0, test_batch_shared_length's length 0:
out[] is pre-filled here)."""
import contextlib
import ctypes
import types

import numpy as np
import pytest

try:  # GPU processes load torch (and its HIP runtime) before libmcrc32c.so
    import torch as _torch  # noqa: F401
except ImportError:
    pass

from memcached_amd import _lib
from memcached_amd import crc32c as mc

from . import base_shift_cases as bs
from . import chain_cases as cc
from . import copy_cases
from . import copy_items_model
from . import header_model as hm
from . import keep_stamped_model as ks
from . import oracle
from . import raw_calls as raw
from . import recover_model
from . import repair_bytes_model as bm
from . import repair_model as rm
from . import salvage_cases as sc
from . import salvage_model as sm
from . import scrub_cases as sca
from . import scrub_gaps_cases as gc
from . import scrub_gaps_model as gm
from . import scrub_model as scm
from . import triage_model as tm
from .salvage_cases import SMALL as SALVAGE_NAMES

pytestmark = pytest.mark.gpu
SLACK = bs.SLACK
LISTS, WORDS = [name for name, _ in raw.SCRUB_LISTS], raw.SCRUB_WORDS


@pytest.fixture(scope="module")
def torch():
    return raw.need_gpu()


@pytest.fixture(params=["small", "planned"])
def route(request):
    """Both span routes, as test_gpu_parity.py's fixture sets them."""
    with raw.small_max(0 if request.param == "planned" else 8192):
        yield request.param


@pytest.fixture
def planned():
    with raw.small_max(0):
        yield "planned"


# ---------------------------------------------------------------------------
# framing
# ---------------------------------------------------------------------------
def _place(torch, B, s):
    """(allocation, the library's view) of buffer B at shift s on the device."""
    alloc = torch.from_numpy(bs.frame(B, s)).cuda()
    assert alloc.data_ptr() % 256 == 0  # (the shift's residues are the base's)
    v = alloc[SLACK + s:SLACK + s + B.size]
    assert v.data_ptr() == alloc.data_ptr() + SLACK + s and v.is_contiguous() and v.numel() == B.size
    return alloc, v


def _holds(alloc, B, s):
    """The whole allocation, slack included, is B framed at s: no store outside the view."""
    got = alloc.cpu().numpy() if hasattr(alloc, "cpu") else alloc
    want = bs.frame(B, s)
    if not np.array_equal(got, want):
        at = np.flatnonzero(got != want)
        raise AssertionError(f"shift {s}: {at.size} bytes differ, first at allocation byte {at[0]} "
                             f"(view byte {int(at[0]) - SLACK - s} of {len(B)})")


@contextlib.contextmanager
def _Pinned(B, s):
    """A crc32c_host_alloc allocation (.arr) holding B framed at s; .view is what the library gets."""
    framed = bs.frame(B, s)
    with raw.pinned(framed.size) as arr:
        assert arr.ctypes.data % 256 == 0
        arr[:] = framed
        view = arr[SLACK + s:SLACK + s + B.size]
        assert view.ctypes.data == arr.ctypes.data + SLACK + s
        yield types.SimpleNamespace(arr=arr, view=view)


def _d(torch, a, view):
    return torch.from_numpy(np.ascontiguousarray(a).view(view).copy()).cuda()


def _u32(t):
    return t.cpu().numpy().view(np.uint32)


def _u64(t):
    return t.cpu().numpy().view(np.uint64)


def _same(got, want, what):
    """Two results of a call, field by field, exactly."""
    assert len(got) == len(want), what
    for k, (g, w) in enumerate(zip(got, want)):
        if isinstance(w, np.ndarray):
            np.testing.assert_array_equal(np.asarray(g), w, err_msg=f"{what}: field {k}")
        else:
            assert g == w, f"{what}: field {k}: {g!r} != {w!r}"


_S0 = {}


def _both(key, run, s, want):
    """run(s) against the model's `want` and against run(0), computed once per key."""
    if key not in _S0:
        _S0[key] = run(0)
        _same(_S0[key], want, f"{key}: shift 0 against the model")
    got = run(s)
    _same(got, want, f"{key}: shift {s} against the model")
    _same(got, _S0[key], f"{key}: shift {s} against shift 0")


# ---------------------------------------------------------------------------
# crc32c_batch
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("order", ["sorted", "shuffled"])
@pytest.mark.parametrize("s", bs.SHIFTS)
def test_batch_lens(torch, route, s, order):
    """offsets[] and lens[] on the device: every length 0..1200 at every start
    residue mod 16 and the long lengths, with and without crc_in."""
    for k, (buf, offs, lens, cin, want, want_in, perm) in enumerate(bs.batch_parts()):
        idx = perm if order == "shuffled" else np.arange(offs.size)
        doffs, dlens, dcin = _d(torch, offs[idx], np.int64), _d(torch, lens[idx], np.int32), _d(torch, cin[idx], np.int32)

        def run(s):
            alloc, v = _place(torch, buf, s)
            out = _u32(mc.batch(v, offsets=doffs, lens=dlens))
            out_in = _u32(mc.batch(v, offsets=doffs, lens=dlens, crc_in=dcin))
            _holds(alloc, buf, s)
            return out, out_in

        _both(("batch_lens", route, order, k), run, s, (want[idx], want_in[idx]))


@pytest.mark.parametrize("s", bs.HOST_SHIFTS)
def test_batch_lens_page_locked(route, s):
    """The same spans read in place from page-locked host memory at ptr + s."""
    for k, (buf, offs, lens, cin, want, want_in, perm) in enumerate(bs.batch_parts()):
        def run(s):
            with _Pinned(buf, s) as pin:
                out = mc.batch(pin.view, offsets=offs[perm], lens=lens[perm])
                out_in = mc.batch(pin.view, offsets=offs, lens=lens, crc_in=cin)
                _holds(pin.arr, buf, s)
                return out, out_in

        _both(("batch_lens_pinned", route, k), run, s, (want[perm], want_in))


def _fixed(torch, v, nbytes, doffs, stride, L, dcin, n):
    out = torch.full((n,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    sp = _lib.Spans(v.data_ptr(), nbytes, None if doffs is None else doffs.data_ptr(), stride, None, L,
                    None if dcin is None else dcin.data_ptr(), out.data_ptr(), n)
    _lib.check(_lib.lib.crc32c_batch(ctypes.byref(sp), _lib.CRC32C_DEVICE, None))
    return _u32(out)


@pytest.mark.parametrize("s", bs.SHIFTS)
@pytest.mark.parametrize("L", bs.SHARED_LENS)
def test_batch_shared_length(torch, route, L, s):
    """offsets[] with one shared length: one unit per span, no plan (k_spans<false>, k_blocks, K5 or k_final alone)."""
    buf, offs, cin, want, want_in = bs.shared_len_case(L)
    doffs, dcin = _d(torch, offs, np.int64), _d(torch, cin, np.int32)

    def run(s):
        alloc, v = _place(torch, buf, s)
        got = _fixed(torch, v, buf.size, doffs, 0, L, None, offs.size), _fixed(torch, v, buf.size, doffs, 0, L, dcin,
                                                                               offs.size)
        _holds(alloc, buf, s)
        return got

    _both(("shared", route, L), run, s, (want, want_in))


@pytest.mark.parametrize("s", bs.SHIFTS)
@pytest.mark.parametrize("stride", [4096, 4112])
def test_batch_fixed_stride(torch, route, stride, s):
    """4096-byte spans at a fixed stride: K1's shape but for the base (k1_shape
    asks for a 16-byte aligned one), so every shift but 16 leaves K1 and must
    still be exact."""
    buf, cin, want, want_in = bs.stride_case(stride)
    dcin = _d(torch, cin, np.int32)

    def run(s):
        alloc, v = _place(torch, buf, s)
        got = _fixed(torch, v, buf.size, None, stride, 4096, None, 33), _fixed(torch, v, buf.size, None, stride, 4096,
                                                                                dcin, 33)
        _holds(alloc, buf, s)
        return got

    _both(("stride", route, stride), run, s, (want, want_in))


# ---------------------------------------------------------------------------
# crc32c_batch_chains
# ---------------------------------------------------------------------------
CHAIN_CASES = {c.name: c for c in cc.small_cases()}
_CHAIN_WANT = {}


@pytest.mark.parametrize("s", bs.THIN)
@pytest.mark.parametrize("name", list(CHAIN_CASES))
def test_chains(torch, route, name, s):
    case = CHAIN_CASES[name]
    if name not in _CHAIN_WANT:
        _CHAIN_WANT[name] = (cc.expected_iovs(case), cc.expected(case))
    doffs = None if case.offsets is None else _d(torch, case.offsets, np.int64)
    dlens = None if case.lens is None else _d(torch, case.lens, np.int32)
    dfirst = _d(torch, case.first, np.int64)

    def run(s):
        alloc, v = _place(torch, case.buf, s)
        iov_out = torch.full((max(case.n, 1),), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
        out = torch.full((max(case.nchains, 1),), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
        sp = _lib.Spans(v.data_ptr(), case.buf.size, None if doffs is None else doffs.data_ptr(), case.stride,
                        None if dlens is None else dlens.data_ptr(), case.length, None, iov_out.data_ptr(), case.n)
        # (the case's own route, and the planned path)
        with raw.small_max(case.small_max if route == "small" else None):
            rc = _lib.lib.crc32c_batch_chains(ctypes.byref(sp), dfirst.data_ptr(), case.nchains, out.data_ptr(),
                                              _lib.CRC32C_DEVICE, torch.cuda.current_stream().cuda_stream)
        assert rc == _lib.CRC32C_OK
        torch.cuda.synchronize()
        _holds(alloc, case.buf, s)
        return _u32(iov_out)[:case.n], _u32(out)[:case.nchains]

    _both(("chains", route, name), run, s, _CHAIN_WANT[name])


# ---------------------------------------------------------------------------
# verify_items / stamp_items, verify_pages / stamp_pages
# ---------------------------------------------------------------------------
MODES = ["verify", "stamp", "keep"]
_ITEM_WANT = {}


def _items_want(kind, name, mode):
    """(bytes after, ok, nbad) of a call over a set, from the model."""
    key = (kind, name, mode)
    if key not in _ITEM_WANT:
        fresh, stamped, offs, wbuf = (bs.item_set if kind == "items" else bs.page_set)(name)
        if mode == "verify":
            ok = ks.expected_verify(stamped, offs, wbuf)
            _ITEM_WANT[key] = (stamped, ok, int((ok == 0).sum()))
        else:
            _ITEM_WANT[key] = ks.expected_stamp(fresh, offs, wbuf, mode == "keep")
        after, ok, nbad = _ITEM_WANT[key]
        assert nbad >= {"verify": 2, "keep": 1, "stamp": 0}[mode]  # (the damage shows where the call can see it)
    return _ITEM_WANT[key]


def _items_call(mode, v, offs, wbuf):
    if mode == "verify":
        return mc.verify_items(v, offs, region_bytes=wbuf)
    return mc.stamp_items(v, offs, region_bytes=wbuf, keep_stamped=mode == "keep")


@pytest.mark.parametrize("s", bs.SHIFTS)
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", ["mixed", "k5", "long"])
def test_items(torch, route, name, mode, s):
    fresh, stamped, offs, wbuf = bs.item_set(name)
    B = stamped if mode == "verify" else fresh
    after, ok, nbad = _items_want("items", name, mode)
    doffs = _d(torch, offs, np.int64)

    def run(s):
        alloc, v = _place(torch, B, s)
        gok, gbad = _items_call(mode, v, doffs, wbuf)
        torch.cuda.synchronize()
        _holds(alloc, after, s)
        return gok.cpu().numpy(), gbad

    _both(("items", route, name, mode), run, s, (ok, nbad))


@pytest.mark.parametrize("s", bs.HOST_SHIFTS)
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", ["mixed", "k5"])
def test_items_page_locked(route, name, mode, s):
    fresh, stamped, offs, wbuf = bs.item_set(name)
    B = stamped if mode == "verify" else fresh
    after, ok, nbad = _items_want("items", name, mode)

    def run(s):
        with _Pinned(B, s) as pin:
            gok, gbad = _items_call(mode, pin.view, offs, wbuf)
            _holds(pin.arr, after, s)
            return gok, gbad

    _both(("items_pinned", route, name, mode), run, s, (ok, nbad))


def _pages_call(mode, v, wbuf):
    if mode == "verify":
        return mc.verify_pages(v, wbuf)
    return mc.stamp_pages(v, wbuf, keep_stamped=mode == "keep")


@pytest.mark.parametrize("s", bs.SHIFTS)
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", ["runs_1m", "runs_odd", "slots"])
def test_pages(torch, route, name, mode, s):
    """The device walk: wbuf pieces are counted from `base`, so the page as
    built lies at the shifted base and walks as it does at shift 0."""
    fresh, stamped, offs, wbuf = bs.page_set(name)
    B = stamped if mode == "verify" else fresh
    after, ok, nbad = _items_want("pages", name, mode)

    def run(s):
        alloc, v = _place(torch, B, s)
        goffs, gok, gbad = _pages_call(mode, v, wbuf)
        torch.cuda.synchronize()
        _holds(alloc, after, s)
        return _u64(goffs), gok.cpu().numpy(), gbad

    _both(("pages", route, name, mode), run, s, (offs, ok, nbad))


@pytest.mark.parametrize("s", bs.HOST_SHIFTS)
@pytest.mark.parametrize("mode", MODES)
def test_pages_page_locked(route, mode, s):
    fresh, stamped, offs, wbuf = bs.page_set("slots")
    B = stamped if mode == "verify" else fresh
    after, ok, nbad = _items_want("pages", "slots", mode)

    def run(s):
        with _Pinned(B, s) as pin:
            goffs, gok, gbad = _pages_call(mode, pin.view, wbuf)
            _holds(pin.arr, after, s)
            return np.asarray(goffs, np.uint64), gok, gbad

    _both(("pages_pinned", route, mode), run, s, (offs, ok, nbad))


# ---------------------------------------------------------------------------
# crc32c_copy_items
# ---------------------------------------------------------------------------
_COPY_WANT = []


def _copy_want():
    if not _COPY_WANT:
        src, soffs, doffs, used, damaged, dropped = copy_cases.mixed_case()
        dst_init = np.full(used, 0xa5, np.uint8)  # (exactly what the sane images need)
        _COPY_WANT.append((dst_init, copy_items_model.expected_copy(src, soffs, copy_cases.WBUF, dst_init, doffs)))
    return _COPY_WANT[0]


def _copy_run(place, host, ss, ds):
    src, soffs, doffs, used, damaged, dropped = copy_cases.mixed_case()
    dst_init, (w_dst, w_ok, w_bad, w_erange) = _copy_want()
    assert not w_erange
    (salloc, sv), (dalloc, dv), so, do = place(src, ss), place(dst_init, ds), host(soffs), host(doffs)
    ok, nbad = mc.copy_items(sv, so, dv, do, region_bytes=copy_cases.WBUF)
    _holds(salloc, src, ss)
    _holds(dalloc, w_dst, ds)
    return np.asarray(ok.cpu() if hasattr(ok, "cpu") else ok), nbad


@pytest.mark.parametrize("ss,ds", [(1, 0), (0, 1), (7, 9), (16, 131)])
def test_copy_items(torch, route, ss, ds):
    """copy_cases.py's mixed list with the source and the destination shifted apart."""
    dst_init, (w_dst, w_ok, w_bad, w_erange) = _copy_want()

    def run(s):
        got = _copy_run(lambda B, sh: _place(torch, B, sh), lambda a: _d(torch, a, np.int64), *(s or (0, 0)))
        torch.cuda.synchronize()
        return got

    _both(("copy", route), run, (ss, ds), (w_ok, w_bad))


@pytest.mark.parametrize("ss,ds", [(1, 15), (129, 1)])
def test_copy_items_page_locked(route, ss, ds):
    """Both buffers page-locked: read and written in place by the GPU."""
    dst_init, (w_dst, w_ok, w_bad, w_erange) = _copy_want()

    def run(s):
        with contextlib.ExitStack() as pins:
            def place(B, sh):
                pin = pins.enter_context(_Pinned(B, sh))
                return pin.arr, pin.view

            return _copy_run(place, lambda a: a, *(s or (0, 0)))

    _both(("copy_pinned", route), run, (ss, ds), (w_ok, w_bad))


# ---------------------------------------------------------------------------
# repair_items / repair_bytes / repair_headers
# ---------------------------------------------------------------------------
def _repair_items(v, offs, region, max_span):
    ok, bit, info = mc.repair_items(v, offs, region_bytes=region, max_span=max_span)
    return ok, bit, info["nrepaired"], info["nbad"]


def _repair_bytes(v, offs, region, max_span):
    ok, byte, mask, info = mc.repair_bytes(v, offs, region_bytes=region, max_span=max_span)
    return ok, byte, mask, info["nrepaired"], info["nbad"]


def _repair_headers(v, offs, region, max_span):
    ok, bit, lens, info = mc.repair_headers(v, offs, region_bytes=region)
    return ok, bit, lens, info["nrepaired"], info["nbad"]


# name -> (the case, the call, its model: (results..., bytes after)).  (repair_headers has no mixed case: the 42
# variants of that list's damaged images add up to more than the call's work bound, CRC32C_EWORK)
REPAIRS = {
    "items_52": (bs.repair_items_case, _repair_items, lambda b, o, r, m: rm.repair(b, o, r, 4, m)),
    "items_mixed": (bs.repair_mixed_case, _repair_items, lambda b, o, r, m: rm.repair(b, o, r, 4, m)),
    "bytes_52": (bs.repair_bytes_case, _repair_bytes, lambda b, o, r, m: bm.repair(b, o, r, 4, m)),
    "bytes_mixed": (bs.repair_mixed_case, _repair_bytes, lambda b, o, r, m: bm.repair(b, o, r, 4, m)),
    "headers_52": (bs.repair_headers_case, _repair_headers, lambda b, o, r, m: hm.repair(b, o, r, 4)),
}
_REPAIR_WANT = {}


def _repair_case(name):
    """(buffer, offsets, region, max_span, the model's results, the model's bytes after)."""
    if name not in _REPAIR_WANT:
        make, call, model = REPAIRS[name]
        buf, offs, x = make()
        region, max_span = (0, x) if name.endswith("mixed") else (x, 0)
        *want, after = model(buf, offs, region, max_span)
        want = [np.asarray(w) if isinstance(w, (list, np.ndarray)) else int(w) for w in want]
        assert want[-2] >= 1  # (something is repaired)
        _REPAIR_WANT[name] = (buf, offs, region, max_span, tuple(want), after)
    return _REPAIR_WANT[name]


def _unsigned(got, want):
    """A call's fields on the host, each array viewed as the model's dtype (device tensors are signed)."""
    got = [g.cpu().numpy() if hasattr(g, "cpu") else g for g in got]
    return tuple(g.view(w.dtype) if isinstance(w, np.ndarray) and g.dtype.itemsize == w.dtype.itemsize else g
                 for g, w in zip(got, want))


@pytest.mark.parametrize("s", bs.THIN)
@pytest.mark.parametrize("name", list(REPAIRS))
def test_repairs(torch, route, name, s):
    buf, offs, region, max_span, want, after = _repair_case(name)
    doffs = _d(torch, offs, np.int64)

    def run(s):
        alloc, v = _place(torch, buf, s)
        got = REPAIRS[name][1](v, doffs, region, max_span)
        torch.cuda.synchronize()
        _holds(alloc, after, s)
        return _unsigned(got, want)

    _both(("repair", route, name), run, s, want)


@pytest.mark.parametrize("s", bs.HOST_SHIFTS)
@pytest.mark.parametrize("name", ["items_52", "bytes_52", "headers_52"])
def test_repairs_page_locked(route, name, s):
    buf, offs, region, max_span, want, after = _repair_case(name)

    def run(s):
        with _Pinned(buf, s) as pin:
            got = REPAIRS[name][1](pin.view, offs, region, max_span)
            _holds(pin.arr, after, s)
            return _unsigned(got, want)

    _both(("repair_pinned", route, name), run, s, want)


# ---------------------------------------------------------------------------
# salvage_pages / recover_pages / triage_pages / scrub_pages (the planned path)
# ---------------------------------------------------------------------------
_SALVAGE = {}
_PAGE_MODEL = {}


def _salvage_case(name):
    if not _SALVAGE:
        _SALVAGE.update(sc.small_cases())
    return _SALVAGE[name]


def _page_model(kind, name):
    key = (kind, name)
    if key not in _PAGE_MODEL:
        buf, W, cfl = _salvage_case(name)
        if kind == "salvage":
            walked, ok = sc.walk_lists(buf, W, cfl)
            m = {"walk": (walked, ok)}
            for with_lists in (True, False):
                found, scanned, ncand, work = sm.salvage_fast(buf, W, *((walked, ok) if with_lists else (None, None)), cfl)
                m[with_lists] = (np.array(found, np.uint64), scanned, ncand)
        elif kind == "recover":
            m = recover_model.recover(buf, W, cfl)
        else:
            m = tm.triage_fast(buf, W, cfl)
        _PAGE_MODEL[key] = m
    return _PAGE_MODEL[key]


@pytest.mark.parametrize("s", bs.THIN)
@pytest.mark.parametrize("name", SALVAGE_NAMES)
def test_salvage_pages(torch, planned, name, s):
    """With the walk's lists (verify_pages over the same view, checked against
    the sequential walk) and without them."""
    buf, W, cfl = _salvage_case(name)
    m = _page_model("salvage", name)
    for with_lists in (True, False):
        def run(s):
            alloc, v = _place(torch, buf, s)
            walked = wok = None
            if with_lists:
                walked, wok, _ = mc.verify_pages(v, W, cflags64=cfl == 8)
                np.testing.assert_array_equal(_u64(walked), m["walk"][0])
                np.testing.assert_array_equal(wok.cpu().numpy(), m["walk"][1])
            found, info = mc.salvage_pages(v, W, walked, wok, cflags64=cfl == 8)
            torch.cuda.synchronize()
            _holds(alloc, buf, s)
            return _u64(found), info["scanned"], info["ncand"]

        _both(("salvage", name, with_lists), run, s, m[with_lists])


def _listed(entry, torch, v, buf, W, cfl, m, tag):
    """One recover or triage call over the placed view v against the model: (rc, the arrays whole, the counts)."""
    cap = m["nitems"] + 3
    got = raw.listed_pages(entry, raw.Side(torch).adopt(v), buf, W, cap=cap, cfl=cfl)
    raw.expect_unchanged(got, buf)
    raw.expect_listed(got, cap, m, raw.COUNTS[entry], tag=tag)
    return (got["rc"],) + tuple(got[name] for name, _ in raw.LISTED) + tuple(got[k] for k in raw.COUNTS[entry])


@pytest.mark.parametrize("s", bs.THIN)
@pytest.mark.parametrize("name", SALVAGE_NAMES)
def test_recover_pages(torch, planned, name, s):
    buf, W, cfl = _salvage_case(name)
    m = _page_model("recover", name)
    got = {}
    for sh in (0, s):
        alloc, v = _place(torch, buf, sh)
        got[sh] = _listed("crc32c_recover_pages", torch, v, buf, W, cfl, m, sh)
        _holds(alloc, buf, sh)
    _same(got[s], got[0], f"recover {name}: shift {s} against shift 0")


@pytest.mark.parametrize("s", bs.THIN)
@pytest.mark.parametrize("name", SALVAGE_NAMES)
def test_triage_pages(torch, planned, name, s):
    buf, W, cfl = _salvage_case(name)
    m = _page_model("triage", name)
    got = {}
    for sh in (0, s):
        alloc, v = _place(torch, buf, sh)
        got[sh] = _listed("crc32c_triage_pages", torch, v, buf, W, cfl, m, sh)
        _holds(alloc, buf, sh)
    _same(got[s], got[0], f"triage {name}: shift {s} against shift 0")


# (cases module, name, CRC32C_SCRUB_GAPS): scrub_cases' pages and scrub_gaps_cases' with their own arguments,
# scrub_cases' with the bit as well and scrub_gaps_cases' without it
SCRUBS = ([(sca, n, False) for n in sca.CASES] + [(gc, n, None) for n in gc.CASES] +
          [(sca, n, True) for n in sca.CASES] + [(gc, n, False) for n in gc.CASES if n != "behind_off"])
_SCRUB_MODEL = {}


def _scrub_model(cases, name, gaps):
    key = (cases.__name__, name, gaps)
    if key not in _SCRUB_MODEL:
        buf, W, cfl, kw, _ = cases.case(name)
        kw = dict(kw)
        if gaps is not None:
            kw["gaps"] = gaps
        on = kw.pop("gaps", False)
        _SCRUB_MODEL[key] = (gm.scrub(buf, W, cfl, gaps=True, **kw) if on else scm.scrub(buf, W, cfl, **kw), kw, on)
    return _SCRUB_MODEL[key]


@pytest.mark.parametrize("s", bs.THIN)
@pytest.mark.parametrize("cases,name,gaps", SCRUBS, ids=[f"{c.__name__.split('.')[-1]}-{n}-{g}" for c, n, g in SCRUBS])
def test_scrub_pages(torch, planned, cases, name, gaps, s):
    buf, W, cfl, _, _ = cases.case(name)
    m, kw, on = _scrub_model(cases, name, gaps)
    got = {}
    for sh in (0, s):
        alloc, v = _place(torch, buf, sh)
        got[sh] = raw.scrub_pages(raw.Side(torch).adopt(v), buf, W, cap=m["nitems"], flip_cap=m["nflips"], cfl=cfl,
                                  gaps=on, **kw)
        raw.expect_scrub(got[sh], m)
        _holds(alloc, m["after"], sh)
    a, b = got[s], got[0]
    assert {w: a[w] for w in WORDS + ("rc",)} == {w: b[w] for w in WORDS + ("rc",)}
    for n in LISTS:
        np.testing.assert_array_equal(a[n], b[n], err_msg=n)


# ---------------------------------------------------------------------------
# the submit queue
# ---------------------------------------------------------------------------
def test_two_queued_jobs_over_one_page_locked_buffer(route):
    """Two jobs whose bases are ptr + 1 and ptr + 129 of one crc32c_host_alloc
    buffer, submitted together and then waited for: the dispatcher packs them
    into one launch that reads the spans where they lie."""
    buf, offs, lens, cin, _, _, perm = bs.batch_parts()[0]
    rng = np.random.default_rng(1900)
    X = rng.integers(1, 256, 129 + buf.size + SLACK, dtype=np.uint8)
    with raw.pinned(X.size) as arr:
        p = arr.ctypes.data
        assert p % 256 == 0
        arr[:] = X
        jobs = []
        for base in (1, 129):
            o, n = np.ascontiguousarray(offs[perm]), np.ascontiguousarray(lens[perm])
            out = np.full(o.size, 0x5A5A5A5A, np.uint32)
            sp = _lib.Spans(p + base, buf.size, o.ctypes.data, 0, n.ctypes.data, 0, cin.ctypes.data, out.ctypes.data, o.size)
            job = ctypes.c_void_p()
            _lib.check(_lib.lib.crc32c_batch_submit(ctypes.byref(sp), 0, ctypes.byref(job)), "submit")
            jobs.append((base, job, out, sp, o, n))
        for base, job, out, sp, o, n in jobs:
            _lib.check(_lib.lib.crc32c_batch_wait(job), "wait")
        for base, job, out, sp, o, n in jobs:
            np.testing.assert_array_equal(out, oracle.batch(X[base:base + buf.size], o, n, cin), err_msg=f"base + {base}")
        np.testing.assert_array_equal(arr, X)

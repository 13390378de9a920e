"""crc32c_scrub_pages on the GPU: for every page of tests/scrub_cases.py,
through the device route and the host route, the return code, every count, the
list, the log, the final bytes and the words behind cap and flip_cap are
compared exactly with the rule's model (tests/scrub_model.py) and, in the same
process on a copy of the same page, with the flow written out over the
library's own crc32c_triage_pages, crc32c_repair_headers and
crc32c_repair_items."""
import ctypes

import numpy as np
import pytest

from memcached_amd import _lib
from memcached_amd import crc32c as mc
from tests import scrub_cases as sca
from tests import scrub_model as scm

pytestmark = pytest.mark.gpu
SENT = 0x5A5A5A5A5A5A5A5A
SENT32, SENT8 = SENT & 0xFFFFFFFF, SENT & 0xFF
EXTRA = 4  # sentinel words behind each array's room
LISTS = ("offsets", "lens", "kind", "flip_offsets", "flip_bits", "flip_by")
DTYPES = (np.uint64, np.uint32, np.uint8, np.uint64, np.uint64, np.uint8)
WORDS = scm.COUNTS + ("nflips", "headers_repaired", "items_repaired", "rounds", "complete")
NAMES = list(sca.CASES)
ROUTES = [pytest.param(True, id="device"), pytest.param(False, id="host")]
_MODEL = {}


def _torch():
    import torch
    return torch


def model(name, **more):
    key = (name, tuple(sorted(more.items())))
    if key not in _MODEL:
        buf, W, cfl, kw, _ = sca.case(name)
        _MODEL[key] = scm.scrub(buf, W, cfl, **dict(kw, **more))
    return _MODEL[key]


def call(buf, W, dev, cap, flip_cap, cfl=4, max_span=0, max_rounds=0, locate_only=False, null_arrays=False,
         dbuf=None):
    """One crc32c_scrub_pages over a copy of buf (host) or its device copy.
    The six arrays have cap + EXTRA / flip_cap + EXTRA words, pre-filled with
    the sentinel, and the struct's counts hold it too.  Returns the result in
    the model's shape, the arrays whole under "raw", and "after"."""
    mode = (_lib.CRC32C_DEVICE if dev else 0) | (_lib.CRC32C_CFLAGS64 if cfl == 8 else 0) | (
        _lib.CRC32C_LOCATE_ONLY if locate_only else 0)
    rooms = (cap, cap, cap, flip_cap, flip_cap, flip_cap)
    if dev:
        torch = _torch()
        kinds = ((SENT, torch.int64), (SENT32, torch.int32), (SENT8, torch.uint8), (SENT, torch.int64), (SENT, torch.int64),
                 (SENT8, torch.uint8))
        arrays = [torch.full((n + EXTRA,), s, dtype=t, device="cuda") for n, (s, t) in zip(rooms, kinds)]
        ptrs = [a.data_ptr() for a in arrays]
        page = torch.from_numpy(buf.copy()).cuda() if dbuf is None else dbuf
        base, stream = page.data_ptr(), torch.cuda.current_stream().cuda_stream
    else:
        kinds = ((SENT, np.uint64), (SENT32, np.uint32), (SENT8, np.uint8), (SENT, np.uint64), (SENT, np.uint64),
                 (SENT8, np.uint8))
        arrays = [np.full(n + EXTRA, s, t) for n, (s, t) in zip(rooms, kinds)]
        ptrs = [a.ctypes.data for a in arrays]
        page = buf.copy()
        base, stream = page.ctypes.data, None
    if null_arrays:
        ptrs = [None if room == 0 else p for p, room in zip(ptrs, rooms)]
    opts = _lib.ScrubOpts(mode, max_span, max_rounds, stream)
    out = _lib.ScrubOut(*ptrs[:3], cap, *ptrs[3:], flip_cap, *([SENT] * 9), SENT32, SENT32)
    rc = _lib.lib.crc32c_scrub_pages(base, buf.size, W, ctypes.byref(opts), ctypes.byref(out))
    if dev:
        torch.cuda.synchronize()
        raw = [a.cpu().numpy().astype(d) for a, d in zip(arrays, DTYPES)]
        after = page.cpu().numpy()
    else:
        raw, after = arrays, page
    got = {w: int(getattr(out, w)) for w in WORDS}
    got.update(rc=rc, raw=dict(zip(LISTS, raw)), after=after, rooms=dict(zip(LISTS, rooms)), ms=mc.lib.crc32c_last_kernel_ms())
    return got


def check(got, m, after=None):
    """got against the model's result m, exactly; after: the bytes expected."""
    assert got["rc"] == m["rc"]
    assert {w: got[w] for w in WORDS} == {w: m[w] for w in WORDS}
    for name in LISTS:
        total = m["nitems"] if name in LISTS[:3] else m["nflips"]
        room, raw = got["rooms"][name], got["raw"][name]
        k = min(room, total)
        assert raw[:k].tolist() == m[name][:k], name
        sent = SENT if raw.dtype == np.uint64 else SENT32 if raw.dtype == np.uint32 else SENT8
        assert (raw[k:] == sent).all(), f"{name}: written behind its first {k}"
    assert (got["after"] == (m["after"] if after is None else after)).all()


def written_out(page, W, cfl, max_span=0, max_rounds=0):
    """The contract's loop over the library's own three calls (the Python
    face's), the lists built on the host by the model's two builders: (list,
    log, rounds, complete).  page: a host array or a device tensor, repaired
    in place."""
    c64 = cfl == 8
    nbytes = page.numel() if mc._is_torch(page) else page.size
    host = (lambda a: a.cpu().numpy()) if mc._is_torch(page) else (lambda a: a)
    lst = lambda a, d: host(a).astype(d).tolist()  # noqa: E731
    dev_list = (lambda todo: _torch().tensor(todo, dtype=_torch().int64, device="cuda")) if mc._is_torch(page) else (
        lambda todo: np.array(todo, np.uint64))

    def triage():
        o, n, k, _ = mc.triage_pages(page, W, cflags64=c64)
        return lst(o, np.uint64), lst(n, np.uint32), lst(k, np.uint8)

    log, rounds, complete = [], 0, 0
    T = triage()
    while True:
        todo = scm.header_list(*T, nbytes, W)
        flips = []
        if todo:
            ok, bit, _, _ = mc.repair_headers(page, dev_list(todo), W, cflags64=c64)
            flips = [(o, b, 1) for o, s, b in zip(todo, lst(ok, np.uint8), lst(bit, np.uint64)) if s == 5]
        if not flips:
            todo = scm.item_list(*T)
            if todo:
                ok, bit, _ = mc.repair_items(page, dev_list(todo), W, max_span, cflags64=c64)
                flips = [(o, b, 2) for o, s, b in zip(todo, lst(ok, np.uint8), lst(bit, np.uint64)) if s == 5]
            if not flips:
                complete = 1
                break
        log += flips
        rounds += 1
        T = triage()
        if rounds == (max_rounds or 64):
            break
    return T, log, rounds, complete


@pytest.mark.parametrize("dev", ROUTES)
@pytest.mark.parametrize("name", NAMES)
def test_scrub_matches_the_model_and_the_written_out_flow(name, dev):
    buf, W, cfl, kw, notes = sca.case(name)
    m = model(name)
    got = call(buf, W, dev, m["nitems"], m["nflips"], cfl, **kw)
    check(got, m)
    assert got["ms"] >= 0.0
    if m["rc"] != 0:
        return  # (the Python face raises past the work bound: the written-out flow ends there too)
    page = _torch().from_numpy(buf.copy()).cuda() if dev else buf.copy()
    T, log, rounds, complete = written_out(page, W, cfl, **kw)
    assert [list(x) for x in T] == [m["offsets"], m["lens"], m["kind"]]
    assert log == list(zip(m["flip_offsets"], m["flip_bits"], m["flip_by"]))
    assert (rounds, complete) == (m["rounds"], m["complete"])
    assert ((page.cpu().numpy() if dev else page) == got["after"]).all()


@pytest.mark.parametrize("dev", ROUTES)
@pytest.mark.parametrize("name", ["second_pass", "suspect_promotion", "entries_per_piece"])
def test_small_outputs(name, dev):
    """cap and flip_cap each at 0 (the arrays NULL), one less than needed and
    two more: the counts stay exact and the page is fully repaired."""
    buf, W, cfl, kw, _ = sca.case(name)
    m = model(name)
    for cap in (0, m["nitems"] - 1, m["nitems"] + 2):
        for flip_cap in (0, m["nflips"] - 1, m["nflips"] + 2):
            check(call(buf, W, dev, cap, flip_cap, cfl, null_arrays=True, **kw), m)


@pytest.mark.parametrize("name", ["second_pass", "suspect_promotion_cflags64"])
def test_host_locate_only(name):
    buf, W, cfl, kw, _ = sca.case(name)
    m = model(name)
    got = call(buf, W, False, m["nitems"], m["nflips"], cfl, locate_only=True, **kw)
    check(got, m, after=buf)
    replayed = scm.replay(buf, {k: got["raw"][k][:m["nflips"]].tolist() for k in ("flip_offsets", "flip_bits")})
    assert (replayed == call(buf, W, False, m["nitems"], m["nflips"], cfl, **kw)["after"]).all()


def _untouched(got, buf):
    assert all(got[w] == (SENT32 if w in ("rounds", "complete") else SENT) for w in WORDS)
    assert all((got["raw"][k] == got["raw"][k][-1]).all() for k in LISTS)
    assert (got["after"] == buf).all()


def test_device_locate_only_is_refused():
    buf, W, cfl, kw, _ = sca.case("second_pass")
    got = call(buf, W, True, 8, 8, cfl, locate_only=True)
    assert got["rc"] == _lib.CRC32C_EINVAL
    _untouched(got, buf)


@pytest.mark.parametrize("dev", ROUTES)
def test_invalid_arguments_write_nothing(dev):
    buf, W, cfl, kw, _ = sca.case("second_pass")
    got = call(buf, 0, dev, 8, 8)
    assert got["rc"] == _lib.CRC32C_EINVAL
    _untouched(got, buf)
    got = call(buf, W, dev, 8, 8, max_span=_lib.CRC32C_REPAIR_SPAN_MAX + 1)
    assert got["rc"] == _lib.CRC32C_EINVAL
    _untouched(got, buf)
    out = _lib.ScrubOut(None, None, None, 1, None, None, None, 0)
    page = buf.copy()
    assert _lib.lib.crc32c_scrub_pages(page.ctypes.data, buf.size, W, None, ctypes.byref(out)) == _lib.CRC32C_EINVAL
    out = _lib.ScrubOut(None, None, None, 0, None, None, None, 1)
    assert _lib.lib.crc32c_scrub_pages(page.ctypes.data, buf.size, W, None, ctypes.byref(out)) == _lib.CRC32C_EINVAL
    assert _lib.lib.crc32c_scrub_pages(None, buf.size, W, None, ctypes.byref(out)) == _lib.CRC32C_EINVAL
    assert _lib.lib.crc32c_scrub_pages(page.ctypes.data, buf.size, W, None, None) == _lib.CRC32C_EINVAL
    assert _lib.lib.crc32c_scrub_pages(page.ctypes.data, (2**31 - 1) * 64, 64, None,
                                       ctypes.byref(_lib.ScrubOut())) == _lib.CRC32C_EINVAL
    assert (page == buf).all()


@pytest.mark.parametrize("dev", ROUTES)
def test_empty_page_and_null_opts(dev):
    buf, W, cfl, kw, _ = sca.case("kind0_entry")
    got = call(buf[:0], W, dev, 0, 0, dbuf=_torch().zeros(16, dtype=_torch().uint8, device="cuda") if dev else None)
    if not dev:  # (a host array of no bytes has an address all the same)
        assert got["rc"] == 0 and got["complete"] == 1
        assert all(got[w] == 0 for w in WORDS if w != "complete")
    else:
        assert got["rc"] == 0 and got["complete"] == 1 and got["nitems"] == 0 and got["nflips"] == 0
    # opts NULL: a host call with every default
    m = model("kind0_entry")
    page = buf.copy()
    out = _lib.ScrubOut()
    assert _lib.lib.crc32c_scrub_pages(page.ctypes.data, buf.size, W, None, ctypes.byref(out)) == 0
    assert (out.nitems, out.nflips, out.rounds, out.complete) == (m["nitems"], 1, 1, 1)
    assert (page == m["after"]).all()


@pytest.mark.parametrize("dev", ROUTES)
def test_second_call_changes_nothing(dev):
    buf, W, cfl, kw, _ = sca.case("dropped_lookalike")
    m = model("dropped_lookalike")
    again = call(m["after"], W, dev, m["nitems"], 4, cfl)
    assert again["nflips"] == 0 and again["rounds"] == 0 and again["complete"] == 1 and again["rc"] == 0
    assert again["raw"]["offsets"][:m["nitems"]].tolist() == m["offsets"]
    assert again["raw"]["kind"][:m["nitems"]].tolist() == m["kind"]
    assert (again["after"] == m["after"]).all()


@pytest.mark.parametrize("dev", ROUTES)
def test_python_face(dev):
    buf, W, cfl, kw, _ = sca.case("second_pass")
    m = model("second_pass")
    page = _torch().from_numpy(buf.copy()).cuda() if dev else buf.copy()
    *arrays, info = mc.scrub_pages(page, W)
    host = [(a.cpu().numpy() if dev else a) for a in arrays]
    for a, name, d in zip(host, LISTS, DTYPES):
        assert a.astype(d).tolist() == m[name], name
    assert info == dict({w: m[w] for w in WORDS if w != "nitems"}, rc=0)
    assert ((page.cpu().numpy() if dev else page) == m["after"]).all()
    if not dev:
        keep = buf.copy()
        *arrays, info2 = mc.scrub_pages(keep, W, locate_only=True)
        assert info2 == info and (keep == buf).all()
        assert [a.tolist() for a in arrays] == [a.tolist() for a in host]

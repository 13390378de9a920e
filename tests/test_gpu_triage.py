"""crc32c_triage_pages on the GPU: offsets, lens, kind, the six counts and the
return code are compared exactly with the rule's model (tests/triage_model.py)
and, with the kind-6 entries taken out, with the library's own
crc32c_recover_pages on the same buffer, through the device route and the host
route; the words behind the results and the buffer itself stay untouched.  The
suspects then go to crc32c_repair_items, and a second call finds the repaired
ones as intact images."""
import ctypes

import numpy as np
import pytest

from memcached_amd import _lib
from memcached_amd import crc32c as mc
from tests import triage_cases as tc
from tests import triage_model as tm
from tests.test_gpu_salvage import SMALL

pytestmark = pytest.mark.gpu
SENT = 0x5A5A5A5A5A5A5A5A
SENT32, SENT8 = SENT & 0xFFFFFFFF, SENT & 0xFF
COUNTS = ("nitems", "nbad", "nsalvaged", "nsuspect", "scanned", "ncand")
RCOUNTS = tuple(c for c in COUNTS if c != "nsuspect")
SUSPECT = _lib.CRC32C_ITEM_SUSPECT
BUILT = ["behind_nkey0", "walked_bad_is_not_listed_twice", "suspect_inside_found", "found_inside_suspect",
         "many_rounds", "work_bound"]


def _torch():
    import torch
    return torch


def _flags(dev, cflags64):
    return (_lib.CRC32C_CFLAGS64 if cflags64 else 0) | (_lib.CRC32C_DEVICE if dev else 0)


def _call(buf, W, cap, dev, cflags64=False, null_arrays=False, dbuf=None, triage=True):
    """One call of crc32c_triage_pages (or crc32c_recover_pages) over buf (host)
    or its device copy (dbuf: one the caller placed).  Returns (rc, offsets, lens,
    kind -- cap + 4 words each, pre-filled with the sentinel -- and the counts);
    checks that the buffer is unchanged."""
    fn = _lib.lib.crc32c_triage_pages if triage else _lib.lib.crc32c_recover_pages
    names = COUNTS if triage else RCOUNTS
    counts = [ctypes.c_uint64(SENT) for _ in names]
    refs = [ctypes.byref(c) for c in counts]
    if dev:
        torch = _torch()
        if dbuf is None:
            dbuf = torch.from_numpy(buf).cuda()
        out = [torch.full((cap + 4,), s, dtype=t, device="cuda")
               for s, t in ((SENT, torch.int64), (SENT32, torch.int32), (SENT8, torch.uint8))]
        ptrs = [None] * 3 if null_arrays else [o.data_ptr() for o in out]
        rc = fn(dbuf.data_ptr(), buf.size, W, *ptrs, cap, *refs, _flags(True, cflags64),
                torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert torch.equal(dbuf.cpu(), torch.from_numpy(buf)), "base was written"
        got = [o.cpu().numpy().astype(d) for o, d in zip(out, (np.uint64, np.uint32, np.uint8))]
    else:
        keep = buf.copy()
        got = [np.full(cap + 4, s, d) for s, d in ((SENT, np.uint64), (SENT32, np.uint32), (SENT8, np.uint8))]
        ptrs = [None] * 3 if null_arrays else [g.ctypes.data for g in got]
        rc = fn(buf.ctypes.data, buf.size, W, *ptrs, cap, *refs, _flags(False, cflags64), None)
        assert np.array_equal(buf, keep), "base was written"
    return (rc, *got, dict(zip(names, (c.value for c in counts))))


def _expect(got, cap, m, tag, names=COUNTS):
    """One call's results against a model dict, cut at cap; nothing behind it."""
    grc, goffs, glens, gkind, gcounts = got
    assert grc == m["rc"], tag
    assert gcounts == {k: m[k] for k in names}, tag
    k = min(cap, len(m["offsets"]))
    assert goffs[:k].tolist() == m["offsets"][:k] and gkind[:k].tolist() == m["kind"][:k], tag
    assert glens[:k].tolist() == m["lens"][:k], tag
    assert (goffs[k:] == SENT).all() and (glens[k:] == SENT32).all() and (gkind[k:] == SENT8).all(), tag


def _as_model(got):
    rc, offs, lens, kind, counts = got
    n = counts["nitems"]
    return dict(counts, rc=rc, offsets=offs[:n].tolist(), lens=lens[:n].tolist(), kind=kind[:n].tolist())


def _check(buf, W, cfl, m, routes=(True, False)):
    """Every route of one buffer against the model, and against
    crc32c_recover_pages on the same buffer with kind 6 taken out."""
    cf64 = cfl == 8
    cap = m["nitems"] + 3
    for dev in routes:
        got = _call(buf, W, cap, dev, cf64)
        _expect(got, cap, m, dev)
        rec = _call(buf, W, cap, dev, cf64, triage=False)
        mine = tm.without_suspects(_as_model(got))
        _expect(rec, cap, mine, ("recover", dev), RCOUNTS)
        assert rec[4]["nitems"] == got[4]["nitems"] - got[4]["nsuspect"]


@pytest.fixture(scope="module")
def cases():
    out = tc.built()
    out.update(tc.reused())
    return out


@pytest.fixture(scope="module")
def models(cases):
    return {name: tm.triage_fast(buf, W, cfl) for name, (buf, W, cfl, _) in cases.items()}


@pytest.mark.parametrize("name", BUILT + SMALL + ["hand_built", "under_48_bytes"])
def test_cases_match_the_model_and_recover(cases, models, name):
    buf, W, cfl, notes = cases[name]
    m = models[name]
    _check(buf, W, cfl, m)
    tc.check_notes(m, notes)
    if name == "work_bound":
        assert m["rc"] == _lib.CRC32C_EWORK and m["nsuspect"] == 0 and m["nitems"] == len(m["walked"]) > 50
    if name == "cflags64":
        assert cfl == 8  # CRC32C_CFLAGS64


def test_config5_shape():
    buf, W, cfl, notes = tc.config5()
    m = tm.triage_fast(buf, W, cfl)
    _check(buf, W, cfl, m)
    tc.check_notes(m, notes)
    assert m["nsalvaged"] == 306 + 606 + 1000


def test_caps(cases, models):
    buf, W, cfl, _ = cases["behind_nkey0"]
    m = models["behind_nkey0"]
    n = m["nitems"]
    cut = m["kind"].index(SUSPECT) + 1  # the first suspect is written, its found neighbour is not
    assert m["kind"][cut] == _lib.CRC32C_ITEM_SALVAGED and 1 < cut < n
    for dev in (True, False):
        for cap in (1, cut, n):
            _expect(_call(buf, W, cap, dev), cap, m, (dev, cap))
        # cap == 0: everything is still computed, the arrays may be NULL
        _expect(_call(buf, W, 0, dev, null_arrays=True), 0, m, (dev, 0))
    # scanned and ncand may be NULL; nsuspect may not
    c = [ctypes.c_uint64(0) for _ in range(4)]
    rc = _lib.lib.crc32c_triage_pages(buf.ctypes.data, buf.size, W, None, None, None, 0, *map(ctypes.byref, c), None,
                                      None, 0, None)
    assert rc == _lib.CRC32C_OK and [x.value for x in c] == [m["nitems"], m["nbad"], m["nsalvaged"], m["nsuspect"]]
    rc = _lib.lib.crc32c_triage_pages(buf.ctypes.data, buf.size, W, None, None, None, 0, *map(ctypes.byref, c[:3]),
                                      None, None, None, 0, None)
    assert rc == _lib.CRC32C_EINVAL
    # cap != 0 with an array missing
    rc = _lib.lib.crc32c_triage_pages(buf.ctypes.data, buf.size, W, None, None, None, 1, *map(ctypes.byref, c), None,
                                      None, 0, None)
    assert rc == _lib.CRC32C_EINVAL
    # an empty buffer
    rc = _lib.lib.crc32c_triage_pages(buf.ctypes.data, 0, W, None, None, None, 0, *map(ctypes.byref, c), None, None,
                                      0, None)
    assert rc == _lib.CRC32C_OK and [x.value for x in c] == [0, 0, 0, 0]


def test_a_device_buffer_off_the_tile_grid(cases, models):
    """base + 1 .. base + 15: off the scan's 4 KiB tiles and off every 16-byte boundary."""
    buf, W, cfl, _ = cases["behind_nkey0"]
    m = models["behind_nkey0"]
    torch = _torch()
    dbig = torch.zeros(16 + buf.size, dtype=torch.uint8, device="cuda")
    cap = m["nitems"] + 3
    src = torch.from_numpy(buf).cuda()
    for pad in range(1, 16):
        dbig[pad:pad + buf.size] = src
        _expect(_call(buf, W, cap, True, dbuf=dbig[pad:pad + buf.size]), cap, m, pad)


def test_a_page_locked_and_a_pageable_host_buffer(cases, models):
    buf, W, cfl, _ = cases["many_rounds"]
    m = models["many_rounds"]
    cap = m["nitems"] + 3
    _expect(_call(buf.copy(), W, cap, False), cap, m, "pageable")
    p = _lib.lib.crc32c_host_alloc(buf.size)
    assert p
    try:
        pinned = np.ctypeslib.as_array(ctypes.cast(p, ctypes.POINTER(ctypes.c_uint8)), (buf.size,))
        pinned[:] = buf
        _expect(_call(pinned, W, cap, False), cap, m, "pinned")
    finally:
        _lib.lib.crc32c_host_free(p)


def test_python_face_numpy_and_torch(cases, models):
    buf, W, cfl, _ = cases["found_inside_suspect"]
    m = models["found_inside_suspect"]
    info = {k: m[k] for k in ("nbad", "nsalvaged", "nsuspect", "scanned", "ncand")}
    offs, lens, kind, got = mc.triage_pages(buf, W)
    assert (offs.dtype, lens.dtype, kind.dtype) == (np.uint64, np.uint32, np.uint8)
    assert (offs.tolist(), lens.tolist(), kind.tolist(), got) == (m["offsets"], m["lens"], m["kind"], info)
    torch = _torch()
    offs, lens, kind, got = mc.triage_pages(torch.from_numpy(buf).cuda(), W)
    assert offs.is_cuda and lens.is_cuda and kind.is_cuda
    assert (offs.cpu().tolist(), lens.cpu().tolist(), kind.cpu().tolist(), got) == (m["offsets"], m["lens"], m["kind"],
                                                                                    info)
    # 8-byte client flags
    buf, W, cfl, _ = cases["cflags64"]
    m = models["cflags64"]
    offs, lens, kind, got = mc.triage_pages(buf, W, cflags64=True)
    assert (offs.tolist(), lens.tolist(), kind.tolist()) == (m["offsets"], m["lens"], m["kind"])
    # the work bound: the walk's part and the counts travel with the error
    buf, W, cfl, _ = cases["work_bound"]
    m = models["work_bound"]
    for src in (buf, torch.from_numpy(buf).cuda()):
        with pytest.raises(mc.Crc32cError) as e:
            mc.triage_pages(src, W)
        err = e.value
        host = (lambda x: x.cpu()) if src is not buf else (lambda x: x)
        assert err.rc == _lib.CRC32C_EWORK
        assert (err.nsalvaged, err.nsuspect, err.ncand, err.scanned) == (0, 0, m["ncand"], m["scanned"])
        assert host(err.offsets).tolist() == m["offsets"] and host(err.kind).tolist() == m["kind"]
        assert host(err.lens).tolist() == m["lens"] and err.nbad == m["nbad"]


@pytest.mark.parametrize("name", ["behind_nkey0", "many_rounds"])
def test_suspects_are_repaired_and_then_found(cases, models, name):
    """The round trip that is the point: the suspects go to
    crc32c_repair_items, the single-bit ones come back repaired, the two-bit one
    does not, and a second call lists each repaired one as an image found."""
    buf, W, cfl, notes = cases[name]
    m = models[name]
    page = buf.copy()
    offs, lens, kind, info = mc.triage_pages(page, W)
    assert (offs.tolist(), kind.tolist()) == (m["offsets"], m["kind"])
    suspects = offs[kind == SUSPECT]
    assert set(notes["suspects"]) <= set(suspects.tolist())
    ok, bit, rinfo = mc.repair_items(page, suspects, W)
    nrep, nbad = rinfo["nrepaired"], rinfo["nbad"]
    verdict = dict(zip(suspects.tolist(), ok.tolist()))
    for o in notes.get("single_bit", ()):
        assert verdict[o] == _lib.CRC32C_ITEM_REPAIRED, o
    for o in notes.get("two_bit", ()):
        assert verdict[o] == 0, o
    # a suspect that is no image of the case (a look-alike inside one) is not repaired
    assert nrep == len(notes["single_bit"]) and nbad == len(suspects) - nrep
    offs2, lens2, kind2, info2 = mc.triage_pages(page, W)
    kinds2 = dict(zip(offs2.tolist(), kind2.tolist()))
    for o in notes["single_bit"]:
        assert kinds2[o] == _lib.CRC32C_ITEM_SALVAGED, o
    for o in notes.get("two_bit", ()):
        assert kinds2[o] == SUSPECT, o
    assert info2["nsalvaged"] == info["nsalvaged"] + nrep
    # the repaired page is the model's too
    m2 = tm.triage_fast(page, W, cfl)
    assert (offs2.tolist(), lens2.tolist(), kind2.tolist()) == (m2["offsets"], m2["lens"], m2["kind"])


def test_recover_before_and_after_a_triage_call(cases, models):
    """The two entry points share their scratch: the order must not matter."""
    buf, W, cfl, _ = cases["many_rounds"]
    other, W2, _, _ = cases["behind_nkey0"]
    cap = models["many_rounds"]["nitems"] + 3
    for dev in (True, False):
        before = _call(buf, W, cap, dev, triage=False)
        _expect(_call(other, W2, models["behind_nkey0"]["nitems"] + 3, dev), models["behind_nkey0"]["nitems"] + 3,
                models["behind_nkey0"], dev)
        _expect(_call(buf, W, cap, dev), cap, models["many_rounds"], dev)
        after = _call(buf, W, cap, dev, triage=False)
        assert before[0] == after[0] == _lib.CRC32C_OK and before[4] == after[4]
        for a, b in zip(before[1:4], after[1:4]):
            assert np.array_equal(a, b)
        _expect(after, cap, tm.without_suspects(models["many_rounds"]), ("recover", dev), RCOUNTS)

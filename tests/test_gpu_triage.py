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
from tests import raw_calls as raw
from tests import triage_cases as tc
from tests import triage_model as tm
from tests.salvage_cases import SMALL

pytestmark = pytest.mark.gpu
COUNTS, RCOUNTS = raw.TRIAGE_COUNTS, raw.RECOVER_COUNTS
SUSPECT = _lib.CRC32C_ITEM_SUSPECT
BUILT = ["behind_nkey0", "walked_bad_is_not_listed_twice", "suspect_inside_found", "found_inside_suspect",
         "many_rounds", "work_bound"]


def _call(buf, W, cap, dev, cfl=4, null_arrays=False, side=None, triage=True):
    """One call of crc32c_triage_pages (or crc32c_recover_pages) over a copy of
    buf on one route (side: one that holds a buffer the caller placed); the
    buffer is unchanged."""
    got = raw.listed_pages("crc32c_triage_pages" if triage else "crc32c_recover_pages", dev if side is None else side,
                           buf, W, cap=cap, cfl=cfl, null_arrays=null_arrays)
    raw.expect_unchanged(got, buf)
    return got


def _as_model(got):
    n = got["nitems"]
    return dict(got, offsets=got["offsets"][:n].tolist(), lens=got["lens"][:n].tolist(), kind=got["kind"][:n].tolist())


def _check(buf, W, cfl, m, routes=(True, False)):
    """Every route of one buffer against the model, and against
    crc32c_recover_pages on the same buffer with kind 6 taken out."""
    cap = m["nitems"] + 3
    for dev in routes:
        got = _call(buf, W, cap, dev, cfl)
        raw.expect_listed(got, cap, m, COUNTS, tag=dev)
        rec = _call(buf, W, cap, dev, cfl, triage=False)
        mine = tm.without_suspects(_as_model(got))
        raw.expect_listed(rec, cap, mine, RCOUNTS, tag=("recover", dev))
        assert rec["nitems"] == got["nitems"] - got["nsuspect"]


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
            raw.expect_listed(_call(buf, W, cap, dev), cap, m, COUNTS, tag=(dev, cap))
        # cap == 0: everything is still computed, the arrays may be NULL
        raw.expect_listed(_call(buf, W, 0, dev, null_arrays=True), 0, m, COUNTS, tag=(dev, 0))
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
    torch = raw.need_gpu()
    dbig = torch.zeros(16 + buf.size, dtype=torch.uint8, device="cuda")
    cap = m["nitems"] + 3
    src = torch.from_numpy(buf).cuda()
    for pad in range(1, 16):
        dbig[pad:pad + buf.size] = src
        got = _call(buf, W, cap, True, side=raw.Side(torch).adopt(dbig[pad:pad + buf.size]))
        raw.expect_listed(got, cap, m, COUNTS, tag=pad)


def test_a_page_locked_and_a_pageable_host_buffer(cases, models):
    buf, W, cfl, _ = cases["many_rounds"]
    m = models["many_rounds"]
    cap = m["nitems"] + 3
    raw.expect_listed(_call(buf.copy(), W, cap, False), cap, m, COUNTS, tag="pageable")
    with raw.pinned(buf.size) as pinned:
        pinned[:] = buf
        got = _call(buf, W, cap, False, side=raw.Side(where="host").adopt(pinned))
        raw.expect_listed(got, cap, m, COUNTS, tag="pinned")


def test_python_face_numpy_and_torch(cases, models):
    buf, W, cfl, _ = cases["found_inside_suspect"]
    m = models["found_inside_suspect"]
    info = {k: m[k] for k in ("nbad", "nsalvaged", "nsuspect", "scanned", "ncand")}
    offs, lens, kind, got = mc.triage_pages(buf, W)
    assert (offs.dtype, lens.dtype, kind.dtype) == (np.uint64, np.uint32, np.uint8)
    assert (offs.tolist(), lens.tolist(), kind.tolist(), got) == (m["offsets"], m["lens"], m["kind"], info)
    torch = raw.need_gpu()
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
        cap2 = models["behind_nkey0"]["nitems"] + 3
        raw.expect_listed(_call(other, W2, cap2, dev), cap2, models["behind_nkey0"], COUNTS, tag=dev)
        raw.expect_listed(_call(buf, W, cap, dev), cap, models["many_rounds"], COUNTS, tag=dev)
        after = _call(buf, W, cap, dev, triage=False)
        assert before["rc"] == after["rc"] == _lib.CRC32C_OK and all(before[k] == after[k] for k in RCOUNTS)
        for name, _ in raw.LISTED:
            assert np.array_equal(before[name], after[name])
        raw.expect_listed(after, cap, tm.without_suspects(models["many_rounds"]), RCOUNTS, tag=("recover", dev))

"""crc32c_recover_pages on the GPU: offsets, lens, kind, the five counts and the
return code are compared exactly with the rule's model (tests/recover_model.py)
and with the library's own two calls on the same buffer (crc32c_verify_pages,
then crc32c_salvage_pages over its lists), for every buffer through the device
route and the host route, with crc32c_set_small_max at its default and at 0;
the words behind the results and the buffer itself stay untouched."""
import ctypes

import numpy as np
import pytest

from memcached_amd import _lib
from memcached_amd import crc32c as mc
from tests import raw_calls as raw
from tests import recover_model as rm
from tests import salvage_cases as sc
from tests.salvage_cases import SMALL

pytestmark = pytest.mark.gpu
ENTRY = "crc32c_recover_pages"
COUNTS = raw.RECOVER_COUNTS


def _call(buf, W, cap, dev, cfl=4, null_arrays=False, side=None):
    """One call over a copy of buf on one route (side: one that holds a buffer
    the caller placed); the buffer is unchanged."""
    got = raw.listed_pages(ENTRY, dev if side is None else side, buf, W, cap=cap, cfl=cfl,
                           null_arrays=null_arrays)
    raw.expect_unchanged(got, buf)
    return got


def _two_calls(buf, W, dev, cflags64=False):
    """The same answer from crc32c_verify_pages followed by crc32c_salvage_pages
    (offsets and kinds merged here; the lengths are the model's alone)."""
    src = raw.need_gpu().from_numpy(buf).cuda() if dev else buf
    walked, wok, nbad = mc.verify_pages(src, W, cflags64=cflags64)
    rc = _lib.CRC32C_OK
    try:
        found, info = mc.salvage_pages(src, W, walked, wok, cflags64=cflags64)
    except mc.Crc32cError as e:
        assert e.rc == _lib.CRC32C_EWORK
        rc, found, info = e.rc, walked[:0], {"scanned": e.scanned, "ncand": e.ncand}
    host = (lambda x: x.cpu().numpy()) if dev else np.asarray
    walked, wok, found = host(walked).astype(np.uint64), host(wok), host(found).astype(np.uint64)
    offs = np.concatenate((walked, found))
    kind = np.concatenate((wok, np.full(found.size, _lib.CRC32C_ITEM_SALVAGED, np.uint8)))
    order = np.argsort(offs, kind="stable")
    return dict(rc=rc, offsets=offs[order].tolist(), kind=kind[order].tolist(), nitems=offs.size, nbad=nbad,
                nsalvaged=found.size, **info)


def _check(buf, W, cfl=4, small=(None, 0), routes=(True, False), model=None):
    """Every route of one buffer against the model and the two calls."""
    cf64 = cfl == 8
    m = model or rm.recover(buf, W, cfl)
    for sm_max in small:
        with raw.small_max(sm_max):
            for dev in routes:
                tag = (sm_max, dev)
                cap = m["nitems"] + 3
                got = _call(buf, W, cap, dev, cfl)
                raw.expect_listed(got, cap, m, COUNTS, tag=tag)
                raw.expect_listed(got, cap, _two_calls(buf, W, dev, cf64), COUNTS, lens=False, tag=tag)
    return m


@pytest.fixture(scope="module")
def cases():
    out = dict(sc.small_cases())
    out["hand_built"] = sc.hand_built() + (4,)
    out["many_found"] = rm.many_found()
    return out


@pytest.mark.parametrize("name", SMALL + ["hand_built", "under_48_bytes", "many_found"])
def test_small_cases_match_the_model_and_the_two_calls(cases, name):
    buf, W, cfl = cases[name]
    m = _check(buf, W, cfl)
    if name == "many_found":
        assert m["nsalvaged"] == 267
    if name == "under_48_bytes":
        assert m["nitems"] == 0


def test_the_work_bound_leaves_the_walks_part():
    """Past the work bound the walk's entries alone are written: none for
    work_bound_case() itself, whose walk ends at its first byte, and a full
    wbuf's when one lies in front of it."""
    for (buf, W), walked in ((sc.work_bound_case(), False), (rm.work_bound_behind_a_walk(), True)):
        m = _check(buf, W)
        assert m["rc"] == _lib.CRC32C_EWORK and m["nsalvaged"] == 0 and m["nitems"] == len(m["walked"])
        assert (m["nitems"] > 50) == walked and set(m["kind"]) <= {1} and m["ncand"] > 0 and m["scanned"] > 0


def test_caps(cases):
    buf, W, cfl = cases["hdr_nbytes_b0"]
    m = rm.recover(buf, W, cfl)
    n = m["nitems"]
    assert n >= 3 and m["nsalvaged"] >= 1
    for dev in (True, False):
        for cap in (1, n - 1, n):
            raw.expect_listed(_call(buf, W, cap, dev), cap, m, COUNTS, tag=(dev, cap))
        # cap == 0: everything is still computed, the arrays may be NULL
        raw.expect_listed(_call(buf, W, 0, dev, null_arrays=True), 0, m, COUNTS, tag=(dev, 0))
    # scanned and ncand may be NULL
    c = [ctypes.c_uint64(0) for _ in range(3)]
    rc = _lib.lib.crc32c_recover_pages(buf.ctypes.data, buf.size, W, None, None, None, 0, *map(ctypes.byref, c), None,
                                       None, 0, None)
    assert rc == _lib.CRC32C_OK and [x.value for x in c] == [m["nitems"], m["nbad"], m["nsalvaged"]]
    # cap != 0 with an array missing
    rc = _lib.lib.crc32c_recover_pages(buf.ctypes.data, buf.size, W, None, None, None, 1, *map(ctypes.byref, c), None,
                                       None, 0, None)
    assert rc == _lib.CRC32C_EINVAL
    # an empty buffer
    rc = _lib.lib.crc32c_recover_pages(buf.ctypes.data, 0, W, None, None, None, 0, *map(ctypes.byref, c), None, None,
                                       0, None)
    assert rc == _lib.CRC32C_OK and [x.value for x in c] == [0, 0, 0]


def test_a_device_buffer_off_the_tile_grid(cases):
    """base + 4096 + 23: off the scan's 4 KiB tiles and off every 16-byte boundary."""
    buf, W, cfl = cases["many_found"]
    m = rm.recover(buf, W, cfl)
    torch = raw.need_gpu()
    pad = 4096 + 23
    dbig = torch.zeros(pad + buf.size, dtype=torch.uint8, device="cuda")
    dbig[pad:] = torch.from_numpy(buf).cuda()
    cap = m["nitems"] + 3
    raw.expect_listed(_call(buf, W, cap, True, side=raw.Side(torch).adopt(dbig[pad:])), cap, m, COUNTS, tag="off grid")


def test_a_page_locked_host_buffer(cases):
    buf, W, cfl = cases["hdr_cas_bit"]
    m = rm.recover(buf, W, cfl)
    with raw.pinned(buf.size) as pinned:
        pinned[:] = buf
        cap = m["nitems"] + 3
        got = _call(buf, W, cap, False, side=raw.Side(where="host").adopt(pinned))
        raw.expect_listed(got, cap, m, COUNTS, tag="pinned")


def test_config5_shape_goes_through_the_k5_verify_route():
    """8 wbufs of 4 MiB, 1007 images of 4165 B each, one header bit flipped in
    three of them: the walk's 8056 - 1912 or so images and the candidates both
    take the item kernels' large routes."""
    buf, W = sc.config5_case()
    m = _check(buf, W)
    assert m["nsalvaged"] == 306 + 606 + 1000 and m["nitems"] > 6000


def test_python_face_numpy_and_torch(cases):
    buf, W, cfl = cases["first_image"]
    m = rm.recover(buf, W, cfl)
    info = {k: m[k] for k in ("nbad", "nsalvaged", "scanned", "ncand")}
    offs, lens, kind, got = mc.recover_pages(buf, W)
    assert (offs.dtype, lens.dtype, kind.dtype) == (np.uint64, np.uint32, np.uint8)
    assert (offs.tolist(), lens.tolist(), kind.tolist(), got) == (m["offsets"], m["lens"], m["kind"], info)
    torch = raw.need_gpu()
    offs, lens, kind, got = mc.recover_pages(torch.from_numpy(buf).cuda(), W)
    assert offs.is_cuda and lens.is_cuda and kind.is_cuda
    assert (offs.cpu().tolist(), lens.cpu().tolist(), kind.cpu().tolist(), got) == (m["offsets"], m["lens"], m["kind"],
                                                                                    info)
    # 8-byte client flags
    buf, W, cfl = cases["cflags64"]
    m = rm.recover(buf, W, cfl)
    offs, lens, kind, got = mc.recover_pages(buf, W, cflags64=True)
    assert (offs.tolist(), lens.tolist(), kind.tolist()) == (m["offsets"], m["lens"], m["kind"])
    # the work bound: the walk's part and the counts travel with the error
    buf, W = rm.work_bound_behind_a_walk()
    m = rm.recover(buf, W)
    assert m["nitems"] > 50
    for src in (buf, torch.from_numpy(buf).cuda()):
        with pytest.raises(mc.Crc32cError) as e:
            mc.recover_pages(src, W)
        err = e.value
        host = (lambda x: x.cpu()) if src is not buf else (lambda x: x)
        assert err.rc == _lib.CRC32C_EWORK and (err.nsalvaged, err.ncand, err.scanned) == (0, m["ncand"], m["scanned"])
        assert host(err.offsets).tolist() == m["offsets"] and host(err.kind).tolist() == m["kind"]
        assert host(err.lens).tolist() == m["lens"] and err.nbad == m["nbad"]

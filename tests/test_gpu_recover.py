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
from tests import recover_model as rm
from tests import salvage_cases as sc
from tests.test_gpu_salvage import SMALL

pytestmark = pytest.mark.gpu
SENT = 0x5A5A5A5A5A5A5A5A
SENT32, SENT8 = SENT & 0xFFFFFFFF, SENT & 0xFF
COUNTS = ("nitems", "nbad", "nsalvaged", "scanned", "ncand")


def _torch():
    import torch
    return torch


def _flags(dev, cflags64):
    return (_lib.CRC32C_CFLAGS64 if cflags64 else 0) | (_lib.CRC32C_DEVICE if dev else 0)


def _call(buf, W, cap, dev, cflags64=False, null_arrays=False, dbuf=None):
    """One library call over buf (host) or its device copy (dbuf: one the
    caller placed).  Returns (rc, offsets, lens, kind -- cap + 4 words each,
    pre-filled with the sentinel -- and the five counts); checks that the
    buffer is unchanged."""
    counts = [ctypes.c_uint64(SENT) for _ in range(5)]
    refs = [ctypes.byref(c) for c in counts]
    if dev:
        torch = _torch()
        if dbuf is None:
            dbuf = torch.from_numpy(buf).cuda()
        out = [torch.full((cap + 4,), s, dtype=t, device="cuda")
               for s, t in ((SENT, torch.int64), (SENT32, torch.int32), (SENT8, torch.uint8))]
        ptrs = [None] * 3 if null_arrays else [o.data_ptr() for o in out]
        rc = _lib.lib.crc32c_recover_pages(dbuf.data_ptr(), buf.size, W, *ptrs, cap, *refs, _flags(True, cflags64),
                                           torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert torch.equal(dbuf.cpu(), torch.from_numpy(buf)), "base was written"
        got = [o.cpu().numpy().astype(d) for o, d in zip(out, (np.uint64, np.uint32, np.uint8))]
    else:
        keep = buf.copy()
        got = [np.full(cap + 4, s, d) for s, d in ((SENT, np.uint64), (SENT32, np.uint32), (SENT8, np.uint8))]
        ptrs = [None] * 3 if null_arrays else [g.ctypes.data for g in got]
        rc = _lib.lib.crc32c_recover_pages(buf.ctypes.data, buf.size, W, *ptrs, cap, *refs, _flags(False, cflags64),
                                           None)
        assert np.array_equal(buf, keep), "base was written"
    return (rc, *got, dict(zip(COUNTS, (c.value for c in counts))))


def _two_calls(buf, W, dev, cflags64=False):
    """The same answer from crc32c_verify_pages followed by crc32c_salvage_pages
    (offsets and kinds merged here; the lengths are the model's alone)."""
    src = _torch().from_numpy(buf).cuda() if dev else buf
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
    counts = dict(nitems=offs.size, nbad=nbad, nsalvaged=found.size, **info)
    return rc, offs[order].tolist(), kind[order].tolist(), counts


def _expect(got, cap, rc, offs, lens, kind, counts, tag):
    """One call's results against one expected answer, cut at cap."""
    grc, goffs, glens, gkind, gcounts = got
    assert grc == rc, tag
    assert gcounts == {k: counts[k] for k in COUNTS}, tag
    k = min(cap, len(offs))
    assert goffs[:k].tolist() == offs[:k] and gkind[:k].tolist() == kind[:k], tag
    if lens is not None:
        assert glens[:k].tolist() == lens[:k], tag
    assert (goffs[k:] == SENT).all() and (glens[k:] == SENT32).all() and (gkind[k:] == SENT8).all(), tag


def _check(buf, W, cfl=4, small=(None, 0), routes=(True, False), model=None):
    """Every route of one buffer against the model and the two calls."""
    cf64 = cfl == 8
    m = model or rm.recover(buf, W, cfl)
    for sm_max in small:
        prev = mc.set_small_max(sm_max) if sm_max is not None else None
        try:
            for dev in routes:
                tag = (sm_max, dev)
                cap = m["nitems"] + 3
                got = _call(buf, W, cap, dev, cf64)
                _expect(got, cap, m["rc"], m["offsets"], m["lens"], m["kind"], m, tag)
                rc2, offs2, kind2, counts2 = _two_calls(buf, W, dev, cf64)
                _expect(got, cap, rc2, offs2, None, kind2, counts2, tag)
        finally:
            if prev is not None:
                mc.set_small_max(prev)
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
            _expect(_call(buf, W, cap, dev), cap, m["rc"], m["offsets"], m["lens"], m["kind"], m, (dev, cap))
        # cap == 0: everything is still computed, the arrays may be NULL
        _expect(_call(buf, W, 0, dev, null_arrays=True), 0, m["rc"], [], [], [], m, (dev, 0))
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
    torch = _torch()
    pad = 4096 + 23
    dbig = torch.zeros(pad + buf.size, dtype=torch.uint8, device="cuda")
    dbig[pad:] = torch.from_numpy(buf).cuda()
    cap = m["nitems"] + 3
    _expect(_call(buf, W, cap, True, dbuf=dbig[pad:]), cap, m["rc"], m["offsets"], m["lens"], m["kind"], m, "off grid")


def test_a_page_locked_host_buffer(cases):
    buf, W, cfl = cases["hdr_cas_bit"]
    m = rm.recover(buf, W, cfl)
    p = _lib.lib.crc32c_host_alloc(buf.size)
    assert p
    try:
        pinned = np.ctypeslib.as_array(ctypes.cast(p, ctypes.POINTER(ctypes.c_uint8)), (buf.size,))
        pinned[:] = buf
        cap = m["nitems"] + 3
        _expect(_call(pinned, W, cap, False), cap, m["rc"], m["offsets"], m["lens"], m["kind"], m, "pinned")
    finally:
        _lib.lib.crc32c_host_free(p)


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
    torch = _torch()
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

"""crc32c_salvage_pages on the GPU against the rule's model
(tests/salvage_model.py): offsets, nfound, scanned, ncand and the return code
are compared exactly, for every buffer through the device route and the host
route, with crc32c_set_small_max at its default and at 0 (both verify routes
for the candidates), and with the walk's lists (from verify_pages on the same
buffer) and without them."""
import ctypes

import numpy as np
import pytest

from memcached_amd import _lib
from memcached_amd import crc32c as mc
from tests import raw_calls as raw
from tests import salvage_cases as sc
from tests import salvage_model as sm
from tests.salvage_cases import SMALL

pytestmark = pytest.mark.gpu
OK = _lib.CRC32C_OK


def _expect(buf, W, walked, ok, cap, dev, want, tag="", **kw):
    """One call on one route against want -- (rc, the offsets, nfound, scanned,
    ncand) -- cut at cap, nothing behind it; the buffer and the caller's lists
    are unchanged."""
    n = 0 if walked is None else len(walked)
    walked = np.ascontiguousarray(walked, np.uint64) if n else None
    ok = np.ascontiguousarray(ok, np.uint8) if n else None
    got = raw.salvage_pages(dev, buf, W, walked, ok, cap=cap, **kw)
    raw.expect_unchanged(got, buf)
    if n:
        assert np.array_equal(got["walked"], walked) and np.array_equal(got["walked_ok"], ok)
    raw.expect_listed(got, cap, dict(zip(("rc", "offsets") + raw.SALVAGE_COUNTS, want)), raw.SALVAGE_COUNTS,
                     arrays=("offsets",), tag=tag)


def _lists(buf, W, cflags64=False):
    offs, ok, _ = mc.verify_pages(buf, W, cflags64=cflags64)
    return np.asarray(offs, np.uint64), np.asarray(ok, np.uint8)


def _check(buf, W, cfl=4, lists_opts=(False, True), small=(None, 0), routes=(True, False)):
    """Every route of one buffer against the model."""
    cf64 = cfl == 8
    walk = _lists(buf, W, cf64)
    want_walk = sc.walk_lists(buf, W, cfl) if buf.size <= 1 << 20 else None
    if want_walk is not None:  # (the lists the model tests used are the library's walk)
        assert np.array_equal(walk[0], want_walk[0]) and np.array_equal(walk[1], want_walk[1])
    results = {}
    for with_lists in lists_opts:
        walked, ok = walk if with_lists else (None, None)
        found, scanned, ncand, work = sm.salvage_fast(buf, W, walked, ok, cfl)
        assert work <= sm.WORK_MAX * (scanned + W)
        for sm_max in small:
            with raw.small_max(sm_max):
                for dev in routes:
                    _expect(buf, W, walked, ok, len(found) + 3, dev, (OK, found, len(found), scanned, ncand),
                            (with_lists, sm_max, dev), cfl=cfl)
        results[with_lists] = (found, scanned, ncand)
    return results


@pytest.fixture(scope="module")
def cases():
    return sc.small_cases()


@pytest.mark.parametrize("name", SMALL)
def test_small_cases_match_the_model(cases, name):
    buf, W, cfl = cases[name]
    res = _check(buf, W, cfl)
    if name.startswith("hdr_") or name in ("first_image", "last_image", "two_adjacent", "header_then_data"):
        assert len(res[True][0]) >= (0 if name == "last_image" else 1)
    if name == "data_only":
        assert res[True][0] == []
    if name.startswith("ranges_"):
        # one piece with more uncovered entries than the region pass keeps ranges
        # for (mcrc_dev::kSvSlots = 4), and in the second case more than a round
        # of 64 of them among more than 192 entries: the emit pass goes through
        # the entries again
        walked, ok = _lists(buf, W)
        bad = np.bincount((walked[ok == 0] // W).astype(np.int64), minlength=3)
        per = np.bincount((walked // W).astype(np.int64), minlength=3)
        assert bad.max() >= (6 if name == "ranges_6" else 65)
        assert name == "ranges_6" or per[bad.argmax()] > 3 * 64
        assert max(hi - lo for lo, hi in sm.regions(buf, W, walked, ok)) > 2 * 4096


def test_hand_made_lists(cases):
    """Lists that are no walk's: an entry marked good whose header is not sane
    covers nothing, an entry inside a covered image changes nothing (the
    covered bytes end at the running maximum of the ends), and a subset of the
    walk's list leaves the images it skips to be found."""
    buf, W = sc.hand_built()
    for lst, flags in (([0, 1000, 2000], [1, 0, 1]), ([0, 500, 1000, 2000], [1, 0, 0, 1]),
                       ([0, 10, 500, 999, 1000, 1001, 3000], [1, 1, 0, 1, 1, 0, 1]), ([3000], [1]), ([4000], [0])):
        walked, ok = np.array(lst, np.uint64), np.array(flags, np.uint8)
        found, scanned, ncand, _ = sm.salvage_bytewise(buf, W, walked, ok)
        for dev in (True, False):
            _expect(buf, W, walked, ok, 8, dev, (OK, found, len(found), scanned, ncand), (lst, dev))
    assert sm.salvage_bytewise(buf, W, np.array([0, 500, 1000, 2000]), np.array([1, 0, 0, 1]))[0] == [1000, 3000, 4000]
    # more than a round of entries, every third one dropped from the walk's list of a damaged wbuf
    buf, W, cfl = cases["ranges_over_64"]
    walked, ok = _lists(buf, W)
    keep = np.arange(walked.size) % 3 != 1
    walked, ok = walked[keep], ok[keep]
    found, scanned, ncand, _ = sm.salvage_fast(buf, W, walked, ok)
    assert len(found) > 64
    for dev in (True, False):
        _expect(buf, W, walked, ok, len(found) + 2, dev, (OK, found, len(found), scanned, ncand), dev)


def test_python_face_numpy_and_torch(cases):
    buf, W, cfl = cases["hdr_nkey0"]
    offs, ok, _ = mc.verify_pages(buf, W)
    found, scanned, ncand, _ = sm.salvage_fast(buf, W, offs, ok)
    got, info = mc.salvage_pages(buf, W, offs, ok)
    assert got.tolist() == found and info == {"scanned": scanned, "ncand": ncand}
    torch = raw.need_gpu()
    dbuf = torch.from_numpy(buf).cuda()
    doffs, dok, _ = mc.verify_pages(dbuf, W)
    got, info = mc.salvage_pages(dbuf, W, doffs, dok)
    assert got.cpu().tolist() == found and info == {"scanned": scanned, "ncand": ncand}
    whole, info = mc.salvage_pages(dbuf, W)
    assert whole.cpu().tolist() == sm.salvage_fast(buf, W)[0]


def test_a_buffer_shorter_than_a_header():
    buf = sc.small_cases()["under_48_bytes"][0]
    for dev in (True, False):
        _expect(buf, sc.K16, None, None, 4, dev, (OK, [], 0, 0, 0), dev)


@pytest.fixture(scope="module")
def alignment():
    buf, W = sc.alignment_case()
    return buf, W, sm.salvage_fast(buf, W)


def test_every_alignment_and_tile_boundary(alignment):
    """4200 wbufs of 16 KiB whose survivors start at every residue mod 4096
    (the tile is 4 KiB): every lane, piece and tile edge.  The walk finds
    nothing here (each wbuf's first header is damaged), so the lists are empty."""
    buf, W, (found, scanned, ncand, work) = alignment
    assert len(found) == 2 * 4200 and {o % 4096 for o in found} == set(range(4096))
    assert work <= sm.WORK_MAX * (scanned + W)
    for sm_max in (None, 0):
        with raw.small_max(sm_max):
            for dev in (True, False):
                _expect(buf, W, None, None, len(found) + 3, dev, (OK, found, len(found), scanned, ncand), (sm_max, dev))
    walked, ok = _lists(buf, W)
    assert walked.size == 0
    # a device buffer that starts off the tile grid and off a 16-byte boundary
    torch = raw.need_gpu()
    pad = 4096 + 23
    dbig = torch.zeros(pad + 64 * W, dtype=torch.uint8, device="cuda")
    dbig[pad:] = torch.from_numpy(buf[:64 * W]).cuda()
    want = [o for o in found if o < 64 * W]
    got, info = mc.salvage_pages(dbig[pad:], W)
    assert got.cpu().tolist() == want


def test_config5_shape_goes_through_the_k5_verify_route():
    """8 wbufs of 4 MiB, 1007 images of 4165 B each, one header bit flipped in
    three of them: 306, 606 and 1000 survivors behind them.  With the walk's
    lists the 1912 candidates take the planned verify route; without them the
    whole buffer's 8053 candidates are 4096 or more, K5's share of the routes
    (host_route.h item_route), from a device buffer and from a staged host
    buffer, at both settings of crc32c_set_small_max."""
    buf, W = sc.config5_case()
    res = _check(buf, W, lists_opts=(True,))
    found = res[True][0]
    per = np.bincount(np.array(found) // W, minlength=8)
    assert sorted(per[per > 0].tolist()) == [306, 606, 1000]
    res = _check(buf, W, lists_opts=(False,))
    assert res[False][2] >= 4096 and len(res[False][0]) == 8 * 1007 - 3


def test_more_results_than_cap(cases):
    buf, W, cfl = cases["hdr_nkey0"]
    walked, ok = _lists(buf, W)
    found, scanned, ncand, _ = sm.salvage_fast(buf, W, walked, ok)
    assert len(found) >= 3
    for dev in (True, False):
        for cap in (1, len(found) - 1, len(found)):
            _expect(buf, W, walked, ok, cap, dev, (OK, found, len(found), scanned, ncand), (dev, cap))
        # cap == 0 counts only; offsets may be NULL (the CRCs are still checked: nfound is exact)
        _expect(buf, W, walked, ok, 0, dev, (OK, found, len(found), scanned, ncand), (dev, 0), null_arrays=True)
    # scanned and ncand may be NULL
    n = ctypes.c_uint64(0)
    rc = _lib.lib.crc32c_salvage_pages(buf.ctypes.data, buf.size, W, None, None, 0, None, 0, ctypes.byref(n), None,
                                       None, 0, None)
    assert rc == _lib.CRC32C_OK and n.value == len(sm.salvage_fast(buf, W)[0])


def test_the_work_bound():
    buf, W = sc.work_bound_case()
    walked, ok = _lists(buf, W)
    found, scanned, ncand, work = sm.salvage_fast(buf, W, walked, ok)
    assert work > sm.WORK_MAX * (scanned + W)
    for dev in (True, False):
        _expect(buf, W, walked, ok, 16, dev, (_lib.CRC32C_EWORK, [], 0, scanned, ncand), dev)
    with pytest.raises(mc.Crc32cError) as e:
        mc.salvage_pages(buf, W, walked, ok)
    assert e.value.rc == _lib.CRC32C_EWORK and e.value.ncand == ncand and e.value.scanned == scanned


def test_bad_lists_are_refused(cases):
    buf, W, cfl = cases["hdr_nkey0"]
    walked, ok = _lists(buf, W)
    assert walked.size >= 4
    bad = {
        "descending": walked[::-1].copy(),
        "equal": np.concatenate((walked[:2], walked[1:])),
        "at_base_bytes": np.concatenate((walked, [buf.size])).astype(np.uint64),
    }
    for name, lst in bad.items():
        flags = np.ones(lst.size, np.uint8)
        for dev in (True, False):
            _expect(buf, W, lst, flags, 8, dev, (_lib.CRC32C_EINVAL, []) + (raw.SENT64,) * 3, (name, dev))
    # and the call still works afterwards
    found, scanned, ncand, _ = sm.salvage_fast(buf, W, walked, ok)
    _expect(buf, W, walked, ok, 64, True, (OK, found, len(found), scanned, ncand))

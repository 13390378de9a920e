"""crc32c_recover_pages without a GPU: the facts about the library's own walk
that its kernels rely on (memcached_amd/csrc/k_recover.h) hold in the model for
every small test buffer, the buffers reach the hard parts of the merge, and
the C ABI carries the call."""
import ctypes

import numpy as np
import pytest

from memcached_amd import _lib
from tests import recover_model as rm
from tests import salvage_cases as sc
from tests import salvage_model as sm


@pytest.fixture(scope="module")
def models():
    cases = dict(sc.small_cases())
    cases["hand_built"] = sc.hand_built() + (4,)
    cases["many_found"] = rm.many_found()
    return {name: (case, rm.recover(*case)) for name, case in cases.items()}


def test_the_walk_has_what_the_kernels_rely_on(models):
    for name, ((buf, W, cfl), m) in models.items():
        walked, wok, found = m["walked"].tolist(), m["wok"].tolist(), m["found"]
        assert all(a < b for a, b in zip(walked, walked[1:])), name
        assert not set(walked) & set(found), name
        for i, (o, ok) in enumerate(zip(walked, wok)):
            # a verdict means a sane header ...
            assert not ok or sm.sane(buf, W, o, cfl), (name, o)
            # ... and inside a piece the next entry starts where this one's ITEM_ntotal ends
            if i + 1 < len(walked) and walked[i + 1] // W == o // W:
                assert walked[i + 1] == o + sm.ntotal_at(buf, o, cfl)[0], (name, o)
        # every piece's walk starts at its first byte
        for w in {o // W for o in walked}:
            assert w * W in walked, (name, w)


def test_the_merged_list(models):
    for name, (_, m) in models.items():
        assert m["rc"] == rm.OK, name
        offs = m["offsets"]
        assert all(a < b for a, b in zip(offs, offs[1:])), name
        assert m["nitems"] == len(m["walked"]) + m["nsalvaged"] == len(offs), name
        assert m["kind"].count(rm.SALVAGED) == m["nsalvaged"] and m["kind"].count(0) == m["nbad"], name
        # what the salvage found and what the walk verified is sane: its length is its ITEM_ntotal
        assert all(n > 0 for n, k in zip(m["lens"], m["kind"]) if k), name


def test_the_cases_reach_the_hard_parts(models):
    interleaved, not_sane = set(), set()
    for name, ((buf, W, cfl), m) in models.items():
        walked = m["walked"].tolist()
        if any(f < o and f // W == o // W for f in m["found"] for o in walked):
            interleaved.add(name)
        if any(not sm.sane(buf, W, o, cfl) for o in walked):
            not_sane.add(name)
    # an image found in front of a later walked entry of the same piece: the merge interleaves
    assert {"hdr_nbytes_b0", "hdr_nbytes_b1", "hdr_cas_bit", "first_image", "cflags64", "many_found"} <= interleaved
    # a walked entry whose header is not sane: lens = 0 from a header read
    assert len(not_sane) >= 7, sorted(not_sane)


def test_many_found_is_more_than_four_rounds_in_one_piece(models):
    (buf, W, cfl), m = models["many_found"]
    walked, wok = m["walked"], m["wok"]
    piece = walked // W == 1
    assert wok[piece].tolist() == [1, 1, 0, 0]
    assert m["nsalvaged"] == 267 and all(o // W == 1 for o in m["found"])
    assert int((walked[piece] > m["found"][0]).sum()) == 1
    assert m["nsalvaged"] > 4 * 64


def test_the_work_bound_keeps_the_walks_part():
    for (buf, W), walked in ((sc.work_bound_case(), False), (rm.work_bound_behind_a_walk(), True)):
        m = rm.recover(buf, W)
        assert m["rc"] == rm.EWORK and m["nsalvaged"] == 0 and m["ncand"] > 0
        assert m["offsets"] == m["walked"].tolist() and m["kind"] == m["wok"].tolist()
        assert (m["nitems"] > 50) == walked


def _call(*args):
    return _lib.lib.crc32c_recover_pages(*args)


def test_the_abi_carries_the_call_and_refuses_bad_arguments():
    """The argument checks come before the device lookup, so they run here."""
    assert "crc32c_recover_pages" in _lib.EXPORTED and _lib.CRC32C_ITEM_SALVAGED == rm.SALVAGED
    buf = np.zeros(256, np.uint8)
    offs, lens, kind = np.full(4, 7, np.uint64), np.full(4, 7, np.uint32), np.full(4, 7, np.uint8)
    n = [ctypes.c_uint64(9) for _ in range(5)]
    ptr = [ctypes.byref(x) for x in n]
    arrays = [offs.ctypes.data, lens.ctypes.data, kind.ctypes.data]
    good = [buf.ctypes.data, buf.size, 64, *arrays, 4, *ptr, 0, None]
    for at, bad in ((0, None), (2, 0), (3, None), (4, None), (5, None), (7, None), (8, None), (9, None)):
        args = list(good)
        args[at] = bad
        assert _call(*args) == _lib.CRC32C_EINVAL, at
    # scanned and ncand are optional, and with cap == 0 so are the arrays
    rc = _call(buf.ctypes.data, buf.size, 64, None, None, None, 0, *ptr[:3], None, None, 0, None)
    assert rc in (_lib.CRC32C_OK, _lib.CRC32C_ENODEV)
    if _lib.lib.crc32c_gpu_count() == 0:
        assert _call(*good) == _lib.CRC32C_ENODEV
        assert all(x.value == 9 for x in n) and (offs == 7).all() and (lens == 7).all() and (kind == 7).all()

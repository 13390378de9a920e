"""crc32c_repair_items on the GPU: ok, bit, the two counts and the whole buffer
afterwards are compared exactly with the rule's model (tests/repair_model.py),
for device tensors and host arrays, with crc32c_set_small_max at its default
and at 0 (k_small and the planned path compute the CRCs)."""
import numpy as np
import pytest

from memcached_amd import _lib
from memcached_amd import crc32c as mc
from tests import raw_calls as raw
from tests import repair_model as rm
from tests import salvage_cases as sc
from tests.repair_cases import flip as _flip
from tests.repair_cases import mixed as _mixed
from tests.repair_cases import place as _place

pytestmark = pytest.mark.gpu
NO_BIT, REPAIRED = rm.NO_BIT, rm.REPAIRED


def _run(buf, offs, dev, **kw):
    """mc.repair_items over a copy of buf: (ok, bit, info, the copy afterwards)."""
    side = raw.Side(where=dev)
    page = side.data(buf)
    ok, bit, info = mc.repair_items(page, side.desc(np.asarray(offs, np.uint64)), **kw)
    return side.host(ok, np.uint8), side.host(bit, np.uint64), info, side.host(page, np.uint8)


def _check(buf, offs, small=(None,), region=0, cfl=4, max_span=0, locate_only=False, verify=True):
    """Every route of one list against the model; returns the model's (ok, bit)."""
    offs = np.asarray(offs, np.uint64)
    ok, bit, nrep, nbad, after = rm.repair(buf, offs, region, cfl, max_span, locate_only)
    for sm_max in small:
        with raw.small_max(sm_max):
            for dev in (True, False):
                tag = (sm_max, dev)
                gok, gbit, info, gafter = _run(buf, offs, dev, region_bytes=region, max_span=max_span,
                                               locate_only=locate_only, cflags64=cfl == 8)
                assert gok.tolist() == ok.tolist(), tag
                assert gbit.tolist() == bit.tolist(), tag
                assert info == {"nrepaired": nrep, "nbad": nbad}, tag
                assert np.array_equal(gafter, after), tag
                if verify and not locate_only:  # what the call accepted, and only that, now verifies
                    vok, vbad = mc.verify_items(gafter, offs, region_bytes=region, cflags64=cfl == 8)
                    assert (np.asarray(vok) != 0).tolist() == (ok != 0).tolist(), tag
                    assert vbad == nbad, tag
    return ok, bit


def test_every_position_of_a_52_byte_image_at_every_alignment():
    rng = np.random.default_rng(1)
    img = sc.image_nt(rng, 52)
    bits = list(range(224, 416))
    # (a copy per 128-byte region: a flipped length bit then cannot make an image that lies over its neighbours,
    # which the work bound would refuse)
    buf = np.zeros(16 * len(bits) * 128, np.uint8)
    offs, flipped = [], []
    for a in range(16):
        for k in bits:
            o = (a * len(bits) + (k - 224)) * 128 + a
            buf[o:o + 52] = np.frombuffer(bytes(img), np.uint8)
            _flip(buf, o, k)
            offs.append(o)
            flipped.append(k)
    pristine = buf.copy()
    for o, k in zip(offs, flipped):
        _flip(pristine, o, k)
    ok, bit = _check(buf, offs, small=(None, 0), region=128)
    for o, k, v, b in zip(offs, flipped, ok.tolist(), bit.tolist()):
        assert (v, b) == ((0, NO_BIT) if rm.length_bit(k) else (REPAIRED, k)), (o, k)
    # (the model's buffer: every copy pristine again but the length bits')
    after = rm.repair(buf, offs, 128)[4]
    for o, k in zip(offs, flipped):
        want = buf if rm.length_bit(k) else pristine
        assert np.array_equal(after[o:o + 52], want[o:o + 52])


def _boundary_images(rng, cfl):
    nts = list(range(52, 81)) + [4164, 4165, 4166]
    # the search's chunk: 4 + L = CHUNK and 2 CHUNK byte steps, +- 1 byte
    nts += [rm.CHUNK + 28 + d for d in (-1, 0, 1)] + [2 * rm.CHUNK + 28 + d for d in (-1, 0, 1)]
    images, flips = [], []
    for i, nt in enumerate(nts):
        cas, cflags = bool(i & 1) and nt >= 61 + cfl, (0x01020304 if i % 3 == 0 and nt >= 61 + cfl else 0)
        img = sc.image_nt(rng, nt, cas=cas, cflags=cflags, cfl=cfl)
        for k in rm.boundary_bits(nt):
            images.append(img)
            flips.append(k)
        images.append(img)  # and an intact copy
        flips.append(None)
    return images, flips


@pytest.mark.parametrize("cfl", [4, 8])
def test_boundaries_of_the_search_and_of_the_image(cfl):
    rng = np.random.default_rng(2 + cfl)
    images, flips = _boundary_images(rng, cfl)
    buf, offs = _place(images, align=1, lead=3)
    for o, k in zip(offs.tolist(), flips):
        if k is not None:
            _flip(buf, o, k)
    ok, bit = _check(buf, offs, small=(None, 0), cfl=cfl)
    for k, v, b in zip(flips, ok.tolist(), bit.tolist()):
        if k is None:
            assert (v, b) == (1, NO_BIT)
        elif not rm.length_bit(k):
            assert (v, b) == (REPAIRED, k)
    assert sum(k is not None and not rm.length_bit(k) for k in flips) > 300


def test_one_long_image():
    rng = np.random.default_rng(3)
    nt = (1 << 20) + 77
    img = sc.image_nt(rng, nt, cas=True)
    buf, offs = _place([img] * 16, align=1, lead=5)
    ks = [224, 255, 8 * 48, 8 * nt - 1, 8 * nt - 16] + rng.integers(8 * 48, 8 * nt, 10).tolist() + [None]
    for o, k in zip(offs.tolist(), ks):
        if k is not None:
            _flip(buf, o, k)
    ok, bit = _check(buf, offs)
    assert ok.tolist() == [REPAIRED] * 15 + [1] and bit.tolist() == ks[:15] + [NO_BIT]
    # over max_span: left alone
    ok, bit = _check(buf, offs[:2], max_span=1 << 20)
    assert ok.tolist() == [0, 0]


def test_mixed_list_of_ten_thousand():
    rng = np.random.default_rng(4)
    n, max_span = 10240, 3000
    buf, offs, kinds = _mixed(rng, n, max_span)
    ok, bit = _check(buf, offs, small=(None, 0), max_span=max_span)
    assert (ok[kinds == 4] == 0).all() and (ok[kinds == 6] == 1).all() and (ok[kinds == 8] == 0).all()
    intact = np.isin(kinds, (0, 1, 2))
    intact[[n // 3, n // 2]] = False
    assert (ok[intact] == 1).all()
    assert ok[n // 3] == 0 and ok[n // 2] == REPAIRED
    one = np.isin(kinds, (3, 9))
    one[n // 3] = False
    assert (ok[one] == REPAIRED).all()
    # a short list of the same buffer in an order of its own, through k_small
    pick = rng.permutation(n)[:3000]
    _check(buf, offs[pick], small=(None,), max_span=max_span)
    # with a region the images do not cross
    _check(buf, offs[:2000], region=1 << 20, max_span=max_span)


def test_locate_only_leaves_the_buffer_alone():
    rng = np.random.default_rng(5)
    buf, offs, kinds = _mixed(rng, 2000, 1000)
    a = _check(buf, offs, small=(None, 0), max_span=1000, locate_only=True)
    b = rm.repair(buf, offs, max_span=1000)
    assert a[0].tolist() == b[0].tolist() and a[1].tolist() == b[1].tolist()
    assert int((a[0] == REPAIRED).sum()) > 300
    # a read-only host buffer is accepted so
    ok, bit, info = mc.repair_items(bytes(buf), offs, max_span=1000, locate_only=True)
    assert ok.tolist() == b[0].tolist() and info["nrepaired"] == b[2]


def test_bounds_and_arguments():
    rng = np.random.default_rng(6)
    nt = 100000
    img = sc.image_nt(rng, nt)
    buf, offs = _place([sc.image_nt(rng, 300), img, sc.image_nt(rng, 120000), sc.image_nt(rng, 300)])
    _flip(buf, int(offs[1]), 8 * 5000 + 2)
    assert 3 * (nt - 32) > buf.size > 2 * (nt - 32)
    three = np.array([offs[1]] * 3 + [offs[0]], np.uint64)
    for dev in (False, True):
        # the spans of the one image named three times pass base_bytes
        got = raw.repair_items(dev, buf, three)
        assert (got["rc"], got["nrepaired"]) == (_lib.CRC32C_EWORK, 0)
        raw.expect_unchanged(got, buf)
        # twice stays below it: the call works (that image's content is unspecified; the other is intact)
        got = raw.repair_items(dev, buf, three[1:], locate_only=True)
        assert got["rc"] == _lib.CRC32C_OK
        raw.expect_unchanged(got, buf)
        # n == 0
        got = raw.repair_items(dev, buf, three, n=0)
        assert (got["rc"], got["nrepaired"], got["nbad"]) == (_lib.CRC32C_OK, 0, 0)
        # each NULL argument, max_span over the limit
        refused = [raw.repair_items(dev, buf, three, null=(name,))
                   for name in ("buf", "offsets", "ok", "bit", "nrepaired", "nbad")]
        refused.append(raw.repair_items(dev, buf, three, max_span=_lib.CRC32C_REPAIR_SPAN_MAX + 1))
        for got in refused:
            assert got["rc"] == _lib.CRC32C_EINVAL
            raw.expect_unchanged(got, buf)
    with pytest.raises(mc.Crc32cError) as e:
        mc.repair_items(buf.copy(), three)
    assert e.value.rc == _lib.CRC32C_EWORK
    # the limit itself is accepted
    ok, bit, info = mc.repair_items(buf.copy(), offs, max_span=_lib.CRC32C_REPAIR_SPAN_MAX)
    assert ok.tolist() == [1, REPAIRED, 1, 1] and bit[1] == 8 * 5000 + 2 and mc.lib.crc32c_last_kernel_ms() > 0


@pytest.mark.parametrize("name", ["data_only", "ranges_6", "ranges_over_64", "config5_small"])
def test_the_flow_behind_recover_pages(name):
    buf, W, cfl = sc.small_cases()[name]
    if name == "config5_small":  # (its damage is to headers alone: add a data bit)
        buf = buf.copy()
        _flip(buf, W + 4165 * 5, 8 * 2000 + 6)
    for dev in (True, False):
        src = raw.need_gpu().from_numpy(buf.copy()).cuda() if dev else buf.copy()
        offs, lens, kind, info = mc.recover_pages(src, W, cflags64=cfl == 8)
        host = (lambda x: x.cpu().numpy()) if dev else np.asarray
        sel = (host(kind) == 0) & (host(lens) != 0)
        bad = host(offs).astype(np.uint64)[sel]
        assert bad.size >= 1
        want = rm.repair(buf, bad, W, cfl)
        todo = raw.need_gpu().from_numpy(bad.astype(np.int64)).cuda() if dev else bad
        ok, bit, rinfo = mc.repair_items(src, todo, region_bytes=W, cflags64=cfl == 8)
        assert host(ok).tolist() == want[0].tolist() and host(bit).view(np.uint64).tolist() == want[1].tolist()
        assert rinfo == {"nrepaired": want[2], "nbad": want[3]} and want[2] >= 1
        assert np.array_equal(host(src), want[4])

"""crc32c_repair_bytes on the GPU: ok, byte, mask, the two counts and the whole
buffer afterwards are compared exactly with the rule's model
(tests/repair_bytes_model.py), for device tensors and pageable host arrays, and
every image the call repaired then passes verify_items."""
import numpy as np
import pytest

from memcached_amd import _lib
from memcached_amd import crc32c as mc
from tests import repair_bytes_cases as bc
from tests import raw_calls as raw
from tests import repair_bytes_model as bm
from tests import repair_cases as rc
from tests import repair_model as rm
from tests import salvage_cases as sc
from tests import scrub_model as scm
from tests import triage_model as tm

pytestmark = pytest.mark.gpu
NO_BIT, REPAIRED = bm.NO_BIT, bm.REPAIRED


def _run(buf, offs, dev, **kw):
    """mc.repair_bytes over a copy of buf: (ok, byte, mask, info, the copy afterwards)."""
    side = raw.Side(where=dev)
    page = side.data(buf)
    ok, byte, mask, info = mc.repair_bytes(page, side.desc(np.asarray(offs, np.uint64)), **kw)
    return (side.host(ok, np.uint8), side.host(byte, np.uint64), side.host(mask, np.uint8), info,
            side.host(page, np.uint8))


def _check(buf, offs, region=0, cfl=4, max_span=0, locate_only=False, routes=(True, False)):
    """Every route of one list against the model; returns the model's (ok, byte, mask)."""
    offs = np.asarray(offs, np.uint64)
    ok, byte, mask, nrep, nbad, after = bm.repair(buf, offs, region, cfl, max_span, locate_only)
    changed = np.flatnonzero(after != buf)
    if not locate_only:  # (the model's buffer differs in exactly the accepted bytes)
        assert changed.tolist() == sorted(int(o) + int(p) for o, p, v in zip(offs, byte, ok) if v == REPAIRED)
    for dev in routes:
        gok, gbyte, gmask, info, gafter = _run(buf, offs, dev, region_bytes=region, max_span=max_span,
                                               locate_only=locate_only, cflags64=cfl == 8)
        assert gok.tolist() == ok.tolist(), dev
        assert gbyte.tolist() == byte.tolist(), dev
        assert gmask.tolist() == mask.tolist(), dev
        assert info == {"nrepaired": nrep, "nbad": nbad}, dev
        assert np.array_equal(gafter, after), dev
        if not locate_only:  # what the call accepted, and only that, now verifies
            vok, vbad = mc.verify_items(gafter, offs, region_bytes=region, cflags64=cfl == 8)
            assert (np.asarray(vok) != 0).tolist() == (ok != 0).tolist(), dev
            assert vbad == nbad, dev
    return ok, byte, mask


@pytest.mark.parametrize("p", [36, 28, 31])
def test_all_255_masks_at_eight_alignments(p):
    rng = np.random.default_rng(p)
    img = sc.image_nt(rng, 52)
    buf = np.zeros(8 * 255 * 64 + 64, np.uint8)
    offs = []
    for a in range(8):
        for m in range(1, 256):
            o = (a * 255 + m - 1) * 64 + a
            buf[o:o + 52] = np.frombuffer(bytes(img), np.uint8)
            bc.xor_byte(buf, o, p, m)
            offs.append(o)
    ok, byte, mask = _check(buf, offs)
    assert ok.tolist() == [REPAIRED] * len(offs) and byte.tolist() == [p] * len(offs)
    assert mask.tolist() == list(range(1, 256)) * 8


@pytest.mark.parametrize("cfl", [4, 8])
def test_edges_of_the_search_and_of_the_image(cfl):
    """4 + L = 255, 256, 257, 512, 513; damage at steps 0, 3, 4, 5, 255, 256
    and steps - 1: the last and first stored-CRC byte, '\\n' and '\\r' (the CRLF
    is tested with the mask applied), both sides of a chunk edge, and image
    byte 32, the low byte of nbytes: a length byte, rejected and left alone."""
    rng = np.random.default_rng(20 + cfl)
    images, hits = [], []
    for i, steps in enumerate((255, 256, 257, 512, 513)):
        L = steps - 4
        img = sc.image_nt(rng, L + 32, cas=bool(i & 1), cflags=0x01020304 if i % 3 == 0 else 0, cfl=cfl)
        for j in bc.edge_steps(L):
            for m in (0x01, 0x80, 0x03, 0xff, 0x5a):
                images.append(img)
                hits.append((28 + bm.byte_of_step(j, L), m, L + 32))
        images.append(img)  # and an intact copy
        hits.append(None)
    # (a region per image: a damaged nbytes byte makes an image of up to 64 KiB more, which may not lie over
    # its neighbours -- the work bound would refuse the list)
    buf = np.zeros(len(images) * 1024, np.uint8)
    offs = [i * 1024 + i % 8 for i in range(len(images))]
    for o, img, h in zip(offs, images, hits):
        buf[o:o + len(img)] = np.frombuffer(bytes(img), np.uint8)
        if h is not None:
            bc.xor_byte(buf, o, h[0], h[1])
    ok, byte, mask = _check(buf, offs, region=1024, cfl=cfl)
    seen = set()
    for h, v, p, m in zip(hits, ok.tolist(), byte.tolist(), mask.tolist()):
        if h is None:
            assert (v, p, m) == (1, NO_BIT, 0)
        elif 32 <= h[0] <= 35:  # (step 255 of 257 is nbytes' second byte)
            assert (v, p, m) == (0, NO_BIT, 0)
            seen |= {"nbytes"} if h[0] == 32 else set()
        else:
            assert (v, p, m) == (REPAIRED, h[0], h[1]), h
            seen |= {"lf"} if h[0] == h[2] - 1 else {"cr"} if h[0] == h[2] - 2 else set()
            seen |= {"crc3"} if h[0] == 31 else {"crc0"} if h[0] == 28 else set()
    assert seen == {"nbytes", "lf", "cr", "crc3", "crc0"}


def test_length_bit_masks():
    rng = np.random.default_rng(30)
    img = sc.image_nt(rng, 300, cas=True)
    cases = [(38, 0x02, False), (38, 0x05, True), (39, 0x01, False), (39, 0xfe, True)]
    cases += [(41, m, False) for m in (0x01, 0x06, 0x80, 0xff)]
    # (a region per image: one with a damaged length may not lie over its neighbour)
    buf = np.zeros(len(cases) * 1024, np.uint8)
    offs = [i * 1024 + 5 for i in range(len(cases))]
    for o, (p, m, _) in zip(offs, cases):
        buf[o:o + 300] = np.frombuffer(bytes(img), np.uint8)
        bc.xor_byte(buf, o, p, m)
    ok, byte, mask = _check(buf, offs, region=1024)
    for (p, m, accepted), v, gp, gm in zip(cases, ok.tolist(), byte.tolist(), mask.tolist()):
        assert (v, gp, gm) == ((REPAIRED, p, m) if accepted else (0, NO_BIT, 0)), (p, m)


def test_the_span_limit():
    rng = np.random.default_rng(40)
    L = bm.SPAN_MAX
    img = sc.image_nt(rng, L + 32)
    over = sc.image_nt(rng, L + 33)
    buf, offs = rc.place([img, img, over], align=1, lead=7)
    bc.xor_byte(buf, int(offs[0]), 36, 0xc3)
    bc.xor_byte(buf, int(offs[1]), L + 32 - 3, 0x7e)
    bc.xor_byte(buf, int(offs[2]), 36, 0xc3)
    ok, byte, mask = _check(buf, offs, max_span=bm.SPAN_MAX)
    assert ok.tolist() == [REPAIRED, REPAIRED, 0]
    assert byte.tolist() == [36, L + 32 - 3, NO_BIT] and mask.tolist() == [0xc3, 0x7e, 0]
    with pytest.raises(mc.Crc32cError) as e:
        mc.repair_bytes(buf.copy(), offs, max_span=bm.SPAN_MAX + 1)
    assert e.value.rc == _lib.CRC32C_EINVAL
    # the default: L = 0x10000 is searched, L = 0x10001 is not
    a, b = sc.image_nt(rng, 0x10000 + 32), sc.image_nt(rng, 0x10001 + 32)
    buf, offs = rc.place([a, b], align=1, lead=2)
    bc.xor_byte(buf, int(offs[0]), 5000, 0x18)
    bc.xor_byte(buf, int(offs[1]), 5000, 0x18)
    ok, byte, mask = _check(buf, offs)
    assert ok.tolist() == [REPAIRED, 0] and byte.tolist() == [5000, NO_BIT] and mask.tolist() == [0x18, 0]


def test_superset_of_the_one_bit_call():
    """tests/repair_cases.py's mixed page: where repair_items reports bit k,
    this call reports (k // 8, 1 << k % 8); where it reports 1, so does this;
    where it reports 0, this reports 0 or a mask of two or more bits, as the
    model says."""
    rng = np.random.default_rng(4)
    buf, offs, kinds = rc.mixed(rng, 2000, 3000)
    ok, byte, mask = _check(buf, offs, max_span=3000)
    for dev in (True, False):
        src = raw.need_gpu().from_numpy(buf).cuda() if dev else buf
        todo = raw.need_gpu().from_numpy(offs.astype(np.int64)).cuda() if dev else offs
        iok, ibit, _ = mc.repair_items(src, todo, max_span=3000, locate_only=True)
        if dev:
            iok, ibit = iok.cpu().numpy(), ibit.cpu().numpy().view(np.uint64)
        assert int((iok == REPAIRED).sum()) > 300
        for v, k, bv, bp, bmask in zip(iok.tolist(), ibit.tolist(), ok.tolist(), byte.tolist(), mask.tolist()):
            if v == REPAIRED:
                assert (bv, bp, bmask) == (REPAIRED, k // 8, 1 << (k % 8))
            elif v == 1:
                assert (bv, bp, bmask) == (1, NO_BIT, 0)
            else:
                assert bv == 0 or (bv == REPAIRED and bmask & (bmask - 1))


def test_what_the_one_bit_call_cannot_do():
    """10 000 images of 52..4200 bytes (52: the smallest image there is), 1 %
    with one byte XORed by a mask of weight >= 2: repair_items repairs none of
    them, repair_bytes exactly the ones the model accepts -- all but those whose
    mask inverts a length bit.  The pinned two-byte damage: ok 0 and untouched."""
    rng = np.random.default_rng(60)
    buf, offs, damaged = bc.mixed(rng, 10000)
    hit = np.array([d is not None for d in damaged])
    assert hit.sum() == 100
    iok, _, iinfo = mc.repair_items(buf.copy(), offs)
    assert (iok[hit] == 0).all() and (iok[~hit] == 1).all() and iinfo == {"nrepaired": 0, "nbad": 100}
    ok, byte, mask = _check(buf, offs)
    assert (ok[~hit] == 1).all()
    for i in np.flatnonzero(hit).tolist():
        p, m = damaged[i]
        want = (0, NO_BIT, 0) if bm.length_mask(p, m) else (REPAIRED, p, m)
        assert (ok[i], byte[i], mask[i]) == want, (i, p, m)
    assert int((ok == REPAIRED).sum()) >= 90
    buf, offs = bc.two_bytes()
    ok, byte, mask = _check(buf, offs)
    assert ok.tolist() == [0] * len(offs)


def test_locate_only_leaves_the_buffer_alone():
    rng = np.random.default_rng(70)
    buf, offs, damaged = bc.mixed(rng, 1500, percent=20)
    a = _check(buf, offs, locate_only=True)
    b = bm.repair(buf, offs)
    assert all(x.tolist() == y.tolist() for x, y in zip(a, b[:3])) and b[3] > 250
    # a read-only host buffer is accepted so
    ok, byte, mask, info = mc.repair_bytes(bytes(buf), offs, locate_only=True)
    assert ok.tolist() == b[0].tolist() and mask.tolist() == b[2].tolist() and info["nrepaired"] == b[3]


def test_bounds_and_arguments():
    rng = np.random.default_rng(80)
    nt = 100000
    buf, offs = rc.place([sc.image_nt(rng, 300), sc.image_nt(rng, nt), sc.image_nt(rng, 120000), sc.image_nt(rng, 300)])
    bc.xor_byte(buf, int(offs[1]), 5000, 0x66)
    assert 3 * (nt - 32) > buf.size > 2 * (nt - 32)
    three = np.array([offs[1]] * 3 + [offs[0]], np.uint64)
    span = bm.SPAN_MAX
    OK, EINVAL, UNSET = _lib.CRC32C_OK, _lib.CRC32C_EINVAL, raw.SENT64  # (UNSET: a count word the call left alone)
    words = lambda got: (got["rc"], got["nrepaired"], got["nbad"])  # noqa: E731
    for dev in (False, True):
        # the spans of the one image named three times pass base_bytes
        got = raw.repair_bytes(dev, buf, three, max_span=span)
        assert words(got) == (_lib.CRC32C_EWORK, 0, 0)
        raw.expect_unchanged(got, buf)
        # twice stays below it: the call works
        got = raw.repair_bytes(dev, buf, three[1:], max_span=span, locate_only=True)
        assert got["rc"] == OK
        raw.expect_unchanged(got, buf)
        # n == 0
        assert words(raw.repair_bytes(dev, buf, three, n=0, max_span=span)) == (OK, 0, 0)
        # each NULL argument, max_span over the limit
        refused = [raw.repair_bytes(dev, buf, three, max_span=span, null=(name,))
                   for name in ("buf", "offsets", "ok", "byte", "mask")]
        refused.append(raw.repair_bytes(dev, buf, three, max_span=span + 1))
        for got in refused:
            assert words(got) == (EINVAL, UNSET, UNSET)
            raw.expect_unchanged(got, buf)
        side = raw.Side(where=dev)
        page, lst = side.data(buf), side.desc(three)
        assert _lib.lib.crc32c_repair_bytes(raw.ptr(page), buf.size, 0, raw.ptr(lst), 4, None, None) == EINVAL
        # flags this call does not know are ignored (CRC32C_ASYNC has no effect: the counts are there)
        got = raw.repair_bytes(dev, buf, three[2:], max_span=span, asynchronous=True, locate_only=True)
        assert words(got) == (OK, 1, 0)
        raw.expect_unchanged(got, buf)
    with pytest.raises(mc.Crc32cError) as e:
        mc.repair_bytes(buf.copy(), three, max_span=span)
    assert e.value.rc == _lib.CRC32C_EWORK
    ok, byte, mask, info = mc.repair_bytes(buf.copy(), offs, max_span=span)
    assert ok.tolist() == [1, REPAIRED, 1, 1] and (byte[1], mask[1]) == (5000, 0x66)
    assert mc.lib.crc32c_last_kernel_ms() > 0
    # the Python face with an empty list
    ok, byte, mask, info = mc.repair_bytes(buf.copy(), np.zeros(0, np.uint64))
    assert len(ok) == len(byte) == len(mask) == 0 and info == {"nrepaired": 0, "nbad": 0}


def test_a_page_locked_buffer_and_a_stream_of_its_own():
    torch = raw.need_gpu()
    rng = np.random.default_rng(90)
    buf, offs, _ = bc.mixed(rng, 400, percent=25)
    want = bm.repair(buf, offs)
    assert want[3] > 60
    # page-locked host memory, repaired in place by the host route
    with raw.pinned(buf.size) as pinned:
        pinned[:] = buf
        ok, byte, mask, info = mc.repair_bytes(pinned, offs)
        assert ok.tolist() == want[0].tolist() and byte.tolist() == want[1].tolist()
        assert mask.tolist() == want[2].tolist() and info == {"nrepaired": want[3], "nbad": want[4]}
        assert np.array_equal(pinned, want[5])
    # a device buffer on a stream that is not the current one
    st = torch.cuda.Stream()
    t = torch.from_numpy(buf.copy()).cuda()
    o = torch.from_numpy(offs.astype(np.int64)).cuda()
    torch.cuda.synchronize()
    ok, byte, mask, info = mc.repair_bytes(t, o, stream=st.cuda_stream)
    st.synchronize()
    assert ok.cpu().numpy().tolist() == want[0].tolist() and mask.cpu().numpy().tolist() == want[2].tolist()
    assert info == {"nrepaired": want[3], "nbad": want[4]} and np.array_equal(t.cpu().numpy(), want[5])


def test_the_flow_behind_triage_pages():
    """A page of a few wbufs with byte damage in images the walk reaches and in
    images behind a header that ended a walk: triage_pages, the item list of
    INTEGRATION.md section 4g, repair_bytes -- against the models composed the
    same way."""
    rng = np.random.default_rng(100)
    W = sc.K16
    wbufs = [sc.mixed(rng, W) for _ in range(4)]
    buf, offs = sc.pack(wbufs, W)
    buf[offs[1][1] + 41] = 0                     # a header that ends wbuf 1's walk ...
    bc.xor_byte(buf, offs[1][3], len(wbufs[1][3]) - 9, 0x3c)  # ... and a damaged byte behind it (a suspect)
    bc.xor_byte(buf, offs[0][2], len(wbufs[0][2]) - 4, 0xf0)  # reached by the walk: kind 0
    bc.xor_byte(buf, offs[2][0], 29, 0x81)       # in a stored CRC
    bc.xor_byte(buf, offs[3][1], 33, 0x11)       # a length byte: the walk derails, nothing to repair by this rule
    T = tm.triage_fast(buf, W)
    todo = np.array(scm.item_list(T["offsets"], T["lens"], T["kind"]), np.uint64)
    want = bm.repair(buf, todo, W)
    assert want[3] >= 3 and offs[1][3] in todo.tolist()
    for dev in (True, False):
        src = raw.need_gpu().from_numpy(buf.copy()).cuda() if dev else buf.copy()
        host = (lambda x: x.cpu().numpy()) if dev else np.asarray
        o, lens, kind, _ = mc.triage_pages(src, W)
        mine = np.array(scm.item_list(host(o).astype(np.uint64).tolist(), host(lens).tolist(), host(kind).tolist()),
                        np.uint64)
        assert mine.tolist() == todo.tolist()
        lst = raw.need_gpu().from_numpy(mine.astype(np.int64)).cuda() if dev else mine
        ok, byte, mask, info = mc.repair_bytes(src, lst, region_bytes=W)
        assert host(ok).tolist() == want[0].tolist() and host(byte).view(np.uint64).tolist() == want[1].tolist()
        assert host(mask).tolist() == want[2].tolist() and info == {"nrepaired": want[3], "nbad": want[4]}
        assert np.array_equal(host(src), want[5])

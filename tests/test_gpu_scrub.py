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
from tests import raw_calls as raw
from tests import scrub_cases as sca
from tests import scrub_model as scm

pytestmark = pytest.mark.gpu
LISTS, DTYPES = zip(*raw.SCRUB_LISTS)
WORDS = raw.SCRUB_WORDS
NAMES = list(sca.CASES)
ROUTES = [pytest.param(True, id="device"), pytest.param(False, id="host")]
_MODEL = {}


def model(name, **more):
    key = (name, tuple(sorted(more.items())))
    if key not in _MODEL:
        buf, W, cfl, kw, _ = sca.case(name)
        _MODEL[key] = scm.scrub(buf, W, cfl, **dict(kw, **more))
    return _MODEL[key]


def written_out(page, W, cfl, max_span=0, max_rounds=0):
    """The contract's loop over the library's own three calls (the Python
    face's), the lists built on the host by the model's two builders: (list,
    log, rounds, complete).  page: a host array or a device tensor, repaired
    in place."""
    c64 = cfl == 8
    nbytes = page.numel() if mc._is_torch(page) else page.size
    host = (lambda a: a.cpu().numpy()) if mc._is_torch(page) else (lambda a: a)
    lst = lambda a, d: host(a).astype(d).tolist()  # noqa: E731
    torch = raw.need_gpu() if mc._is_torch(page) else None
    dev_list = (lambda todo: torch.tensor(todo, dtype=torch.int64, device="cuda")) if torch else (
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
    got = raw.scrub_pages(dev, buf, W, cap=m["nitems"], flip_cap=m["nflips"], cfl=cfl, **kw)
    raw.expect_scrub(got, m)
    assert got["ms"] >= 0.0
    if m["rc"] != 0:
        return  # (the Python face raises past the work bound: the written-out flow ends there too)
    page = raw.need_gpu().from_numpy(buf.copy()).cuda() if dev else buf.copy()
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
            got = raw.scrub_pages(dev, buf, W, cap=cap, flip_cap=flip_cap, cfl=cfl, null_arrays=True, **kw)
            raw.expect_scrub(got, m)


@pytest.mark.parametrize("name", ["second_pass", "suspect_promotion_cflags64"])
def test_host_locate_only(name):
    buf, W, cfl, kw, _ = sca.case(name)
    m = model(name)
    caps = dict(cap=m["nitems"], flip_cap=m["nflips"], cfl=cfl)
    got = raw.scrub_pages(False, buf, W, locate_only=True, **caps, **kw)
    raw.expect_scrub(got, m, after=buf)
    replayed = scm.replay(buf, {k: got[k][:m["nflips"]].tolist() for k in ("flip_offsets", "flip_bits")})
    assert (replayed == raw.scrub_pages(False, buf, W, **caps, **kw)["after"]).all()


def _untouched(got, buf):
    assert all(got[w] == (raw.SENT[4] if w in ("rounds", "complete") else raw.SENT64) for w in WORDS)
    assert all((got[k] == got[k][-1]).all() for k in LISTS)
    assert (got["after"] == buf).all()


def test_device_locate_only_is_refused():
    buf, W, cfl, kw, _ = sca.case("second_pass")
    got = raw.scrub_pages(True, buf, W, cap=8, flip_cap=8, cfl=cfl, locate_only=True)
    assert got["rc"] == _lib.CRC32C_EINVAL
    _untouched(got, buf)


@pytest.mark.parametrize("dev", ROUTES)
def test_invalid_arguments_write_nothing(dev):
    buf, W, cfl, kw, _ = sca.case("second_pass")
    got = raw.scrub_pages(dev, buf, 0, cap=8, flip_cap=8)
    assert got["rc"] == _lib.CRC32C_EINVAL
    _untouched(got, buf)
    got = raw.scrub_pages(dev, buf, W, cap=8, flip_cap=8, max_span=_lib.CRC32C_REPAIR_SPAN_MAX + 1)
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
    side = raw.Side(where=dev)
    if dev:
        side.adopt(side.torch.zeros(16, dtype=side.torch.uint8, device="cuda"))
    got = raw.scrub_pages(side, buf[:0], W, cap=0, flip_cap=0)
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
    again = raw.scrub_pages(dev, m["after"], W, cap=m["nitems"], flip_cap=4, cfl=cfl)
    assert again["nflips"] == 0 and again["rounds"] == 0 and again["complete"] == 1 and again["rc"] == 0
    assert again["offsets"][:m["nitems"]].tolist() == m["offsets"]
    assert again["kind"][:m["nitems"]].tolist() == m["kind"]
    assert (again["after"] == m["after"]).all()


@pytest.mark.parametrize("dev", ROUTES)
def test_python_face(dev):
    buf, W, cfl, kw, _ = sca.case("second_pass")
    m = model("second_pass")
    page = raw.need_gpu().from_numpy(buf.copy()).cuda() if dev else buf.copy()
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

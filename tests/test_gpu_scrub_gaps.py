"""crc32c_scrub_pages with CRC32C_SCRUB_GAPS on the GPU: every page of
tests/scrub_gaps_cases.py and of tests/scrub_cases.py with the bit, through
the device route and the host route, against the rule's model
(tests/scrub_gaps_model.py) exactly -- the return code, every count, the list,
the log in order, the final bytes and the words behind cap and flip_cap -- and
every new page without the bit against tests/scrub_model.py."""
import ctypes

import numpy as np
import pytest

from memcached_amd import _lib
from memcached_amd import crc32c as mc
from tests import scrub_cases as sca
from tests import scrub_gaps_cases as gc
from tests import scrub_gaps_model as gm
from tests import scrub_model as scm
from tests.test_gpu_scrub import DTYPES, EXTRA, LISTS, ROUTES, SENT, SENT8, SENT32, WORDS, check

pytestmark = pytest.mark.gpu
NAMES = list(gc.CASES)
_MODEL = {}


def _torch():
    import torch
    return torch


def model(cases, name, **more):
    """The model's result of a case with its own arguments and ``more``, computed once."""
    key = (cases.__name__, name, tuple(sorted(more.items())))
    if key not in _MODEL:
        buf, W, cfl, kw, _ = cases.case(name)
        _MODEL[key] = gm.scrub(buf, W, cfl, **dict(kw, **more))
    return _MODEL[key]


def call(buf, W, dev, cap, flip_cap, cfl=4, max_span=0, max_rounds=0, locate_only=False, gaps=False):
    """tests/test_gpu_scrub.py's call with the mode bit: one crc32c_scrub_pages
    over a copy of buf (host) or its device copy, the six arrays with EXTRA
    sentinel words behind their room."""
    mode = (_lib.CRC32C_DEVICE if dev else 0) | (_lib.CRC32C_CFLAGS64 if cfl == 8 else 0) | (
        _lib.CRC32C_LOCATE_ONLY if locate_only else 0) | (_lib.CRC32C_SCRUB_GAPS if gaps else 0)
    rooms = (cap, cap, cap, flip_cap, flip_cap, flip_cap)
    sents = (SENT, SENT32, SENT8, SENT, SENT, SENT8)
    if dev:
        torch = _torch()
        types = (torch.int64, torch.int32, torch.uint8, torch.int64, torch.int64, torch.uint8)
        arrays = [torch.full((n + EXTRA,), s, dtype=t, device="cuda") for n, s, t in zip(rooms, sents, types)]
        ptrs = [a.data_ptr() for a in arrays]
        page = torch.from_numpy(buf.copy()).cuda()
        base, stream = page.data_ptr(), torch.cuda.current_stream().cuda_stream
    else:
        arrays = [np.full(n + EXTRA, s, t) for n, s, t in zip(rooms, sents, DTYPES)]
        ptrs = [a.ctypes.data for a in arrays]
        page = buf.copy()
        base, stream = page.ctypes.data, None
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
    got.update(rc=rc, raw=dict(zip(LISTS, raw)), after=after, rooms=dict(zip(LISTS, rooms)))
    return got


@pytest.mark.parametrize("dev", ROUTES)
@pytest.mark.parametrize("name", NAMES)
def test_new_pages_match_the_model(name, dev):
    """(``behind`` fails where the bit is ignored: images 3 and 5 stay lost.)"""
    buf, W, cfl, kw, notes = gc.case(name)
    m = model(gc, name)
    got = call(buf, W, dev, m["nitems"], m["nflips"], cfl, **kw)
    check(got, m)
    for o, nt in notes["back"]:
        assert (got["after"][o + 28:o + nt] == notes["pristine"][o + 28:o + nt]).all()


@pytest.mark.parametrize("dev", ROUTES)
@pytest.mark.parametrize("name", ["behind", "overlap", "rounds_of_64"])
def test_small_outputs(name, dev):
    """cap and flip_cap one less than needed and two more: the counts stay exact."""
    buf, W, cfl, kw, _ = gc.case(name)
    m = model(gc, name)
    for cap, flip_cap in ((m["nitems"] - 1, m["nflips"] + 2), (m["nitems"] + 2, m["nflips"] - 1)):
        check(call(buf, W, dev, cap, flip_cap, cfl, **kw), m)


@pytest.mark.parametrize("name", ["behind", "cflags64", "chain"])
def test_host_locate_only_leaves_the_callers_bytes(name):
    buf, W, cfl, kw, _ = gc.case(name)
    m = model(gc, name)
    got = call(buf, W, False, m["nitems"], m["nflips"], cfl, locate_only=True, **kw)
    check(got, m, after=buf)
    replayed = scm.replay(buf, {k: got["raw"][k][:m["nflips"]].tolist() for k in ("flip_offsets", "flip_bits")})
    assert (replayed == m["after"]).all()


@pytest.mark.parametrize("dev", ROUTES)
@pytest.mark.parametrize("name", list(sca.CASES))
def test_older_pages_with_the_bit(name, dev):
    buf, W, cfl, kw, _ = sca.case(name)
    m = model(sca, name, gaps=True)
    check(call(buf, W, dev, m["nitems"], m["nflips"], cfl, gaps=True, **kw), m)


@pytest.mark.parametrize("dev", ROUTES)
@pytest.mark.parametrize("name", NAMES)
def test_new_pages_without_the_bit(name, dev):
    buf, W, cfl, kw, _ = gc.case(name)
    kw = {k: v for k, v in kw.items() if k != "gaps"}
    key = ("off", name)
    if key not in _MODEL:
        _MODEL[key] = scm.scrub(buf, W, cfl, **kw)
    m = _MODEL[key]
    check(call(buf, W, dev, m["nitems"], m["nflips"], cfl, **kw), m)


@pytest.mark.parametrize("dev", ROUTES)
def test_second_call_changes_nothing(dev):
    for name in ("behind", "chain", "entry_inside"):
        buf, W, cfl, kw, _ = gc.case(name)
        m = model(gc, name)
        again = call(m["after"], W, dev, m["nitems"], 4, cfl, **kw)
        assert again["nflips"] == 0 and again["rounds"] == 0 and again["complete"] == 1 and again["rc"] == 0
        assert again["raw"]["offsets"][:m["nitems"]].tolist() == m["offsets"]
        assert again["raw"]["kind"][:m["nitems"]].tolist() == m["kind"]
        assert (again["after"] == m["after"]).all()


@pytest.mark.parametrize("dev", ROUTES)
def test_python_face(dev):
    buf, W, cfl, kw, _ = gc.case("behind")
    m = model(gc, "behind")
    page = _torch().from_numpy(buf.copy()).cuda() if dev else buf.copy()
    *arrays, info = mc.scrub_pages(page, W, gaps=True)
    host = [(a.cpu().numpy() if dev else a) for a in arrays]
    for a, name, d in zip(host, LISTS, DTYPES):
        assert a.astype(d).tolist() == m[name], name
    assert info == dict({w: m[w] for w in WORDS if w != "nitems"}, rc=0)
    assert ((page.cpu().numpy() if dev else page) == m["after"]).all()

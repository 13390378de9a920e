"""crc32c_scrub_pages with CRC32C_SCRUB_GAPS on the GPU: every page of
tests/scrub_gaps_cases.py and of tests/scrub_cases.py with the bit, through
the device route and the host route, against the rule's model
(tests/scrub_gaps_model.py) exactly -- the return code, every count, the list,
the log in order, the final bytes and the words behind cap and flip_cap -- and
every new page without the bit against tests/scrub_model.py."""
import pytest

from memcached_amd import crc32c as mc
from tests import raw_calls as raw
from tests import scrub_cases as sca
from tests import scrub_gaps_cases as gc
from tests import scrub_gaps_model as gm
from tests import scrub_model as scm

pytestmark = pytest.mark.gpu
LISTS, DTYPES = zip(*raw.SCRUB_LISTS)
WORDS = raw.SCRUB_WORDS
ROUTES = [pytest.param(True, id="device"), pytest.param(False, id="host")]
NAMES = list(gc.CASES)
_MODEL = {}


def model(cases, name, **more):
    """The model's result of a case with its own arguments and ``more``, computed once."""
    key = (cases.__name__, name, tuple(sorted(more.items())))
    if key not in _MODEL:
        buf, W, cfl, kw, _ = cases.case(name)
        _MODEL[key] = gm.scrub(buf, W, cfl, **dict(kw, **more))
    return _MODEL[key]


@pytest.mark.parametrize("dev", ROUTES)
@pytest.mark.parametrize("name", NAMES)
def test_new_pages_match_the_model(name, dev):
    """(``behind`` fails where the bit is ignored: images 3 and 5 stay lost.)"""
    buf, W, cfl, kw, notes = gc.case(name)
    m = model(gc, name)
    got = raw.scrub_pages(dev, buf, W, cap=m["nitems"], flip_cap=m["nflips"], cfl=cfl, **kw)
    raw.expect_scrub(got, m)
    for o, nt in notes["back"]:
        assert (got["after"][o + 28:o + nt] == notes["pristine"][o + 28:o + nt]).all()


@pytest.mark.parametrize("dev", ROUTES)
@pytest.mark.parametrize("name", ["behind", "overlap", "rounds_of_64"])
def test_small_outputs(name, dev):
    """cap and flip_cap one less than needed and two more: the counts stay exact."""
    buf, W, cfl, kw, _ = gc.case(name)
    m = model(gc, name)
    for cap, flip_cap in ((m["nitems"] - 1, m["nflips"] + 2), (m["nitems"] + 2, m["nflips"] - 1)):
        raw.expect_scrub(raw.scrub_pages(dev, buf, W, cap=cap, flip_cap=flip_cap, cfl=cfl, **kw), m)


@pytest.mark.parametrize("name", ["behind", "cflags64", "chain"])
def test_host_locate_only_leaves_the_callers_bytes(name):
    buf, W, cfl, kw, _ = gc.case(name)
    m = model(gc, name)
    got = raw.scrub_pages(False, buf, W, cap=m["nitems"], flip_cap=m["nflips"], cfl=cfl, locate_only=True, **kw)
    raw.expect_scrub(got, m, after=buf)
    replayed = scm.replay(buf, {k: got[k][:m["nflips"]].tolist() for k in ("flip_offsets", "flip_bits")})
    assert (replayed == m["after"]).all()


@pytest.mark.parametrize("dev", ROUTES)
@pytest.mark.parametrize("name", list(sca.CASES))
def test_older_pages_with_the_bit(name, dev):
    buf, W, cfl, kw, _ = sca.case(name)
    m = model(sca, name, gaps=True)
    raw.expect_scrub(raw.scrub_pages(dev, buf, W, cap=m["nitems"], flip_cap=m["nflips"], cfl=cfl, gaps=True, **kw), m)


@pytest.mark.parametrize("dev", ROUTES)
@pytest.mark.parametrize("name", NAMES)
def test_new_pages_without_the_bit(name, dev):
    buf, W, cfl, kw, _ = gc.case(name)
    kw = {k: v for k, v in kw.items() if k != "gaps"}
    key = ("off", name)
    if key not in _MODEL:
        _MODEL[key] = scm.scrub(buf, W, cfl, **kw)
    m = _MODEL[key]
    raw.expect_scrub(raw.scrub_pages(dev, buf, W, cap=m["nitems"], flip_cap=m["nflips"], cfl=cfl, **kw), m)


@pytest.mark.parametrize("dev", ROUTES)
def test_second_call_changes_nothing(dev):
    for name in ("behind", "chain", "entry_inside"):
        buf, W, cfl, kw, _ = gc.case(name)
        m = model(gc, name)
        again = raw.scrub_pages(dev, m["after"], W, cap=m["nitems"], flip_cap=4, cfl=cfl, **kw)
        assert again["nflips"] == 0 and again["rounds"] == 0 and again["complete"] == 1 and again["rc"] == 0
        assert again["offsets"][:m["nitems"]].tolist() == m["offsets"]
        assert again["kind"][:m["nitems"]].tolist() == m["kind"]
        assert (again["after"] == m["after"]).all()


@pytest.mark.parametrize("dev", ROUTES)
def test_python_face(dev):
    buf, W, cfl, kw, _ = gc.case("behind")
    m = model(gc, "behind")
    page = raw.need_gpu().from_numpy(buf.copy()).cuda() if dev else buf.copy()
    *arrays, info = mc.scrub_pages(page, W, gaps=True)
    host = [(a.cpu().numpy() if dev else a) for a in arrays]
    for a, name, d in zip(host, LISTS, DTYPES):
        assert a.astype(d).tolist() == m[name], name
    assert info == dict({w: m[w] for w in WORDS if w != "nitems"}, rc=0)
    assert ((page.cpu().numpy() if dev else page) == m["after"]).all()

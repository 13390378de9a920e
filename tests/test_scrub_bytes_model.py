"""The model of CRC32C_SCRUB_BYTES (tests/scrub_bytes_model.py) on the pages of
tests/scrub_bytes_cases.py, tests/scrub_gaps_cases.py and tests/scrub_cases.py
(no GPU, no library call): each case's own notes with CRC32C_SCRUB_GAPS and
without, the log replayed, the fixpoint, the shape of the byte stage's log
entries, the meaning of items_repaired, and the loop with the rule off against
tests/scrub_gaps_model.py."""
import pytest

from tests import scrub_bytes_cases as bc
from tests import scrub_bytes_model as sbm
from tests import scrub_cases as sca
from tests import scrub_gaps_cases as gc
from tests import scrub_gaps_model as gm
from tests import scrub_model as scm
from tests.test_scrub_gaps_model import same

NAMES = list(bc.CASES)
GAPS = [pytest.param(False, id="plain"), pytest.param(True, id="gaps")]
OLDER = [(sca, n) for n in sca.CASES] + [(gc, n) for n in gc.CASES]
_RESULTS = {}


def result(name, gaps):
    """The model's result of a case, computed once."""
    if (name, gaps) not in _RESULTS:
        buf, W, cfl, kw, _ = bc.case(name)
        _RESULTS[name, gaps] = sbm.scrub(buf, W, cfl, gaps=gaps, **kw)
    return _RESULTS[name, gaps]


@pytest.mark.parametrize("gaps", GAPS)
@pytest.mark.parametrize("name", NAMES)
def test_case_notes(name, gaps):
    buf, W, cfl, kw, notes = bc.case(name)
    m = result(name, gaps)
    bc.check_notes(m, gm.first_lists(buf, W, cfl, gaps)[:3], notes, buf, gaps)


@pytest.mark.parametrize("gaps", GAPS)
@pytest.mark.parametrize("name", NAMES)
def test_log_replays_and_counts_add_up(name, gaps):
    buf, W, cfl, kw, notes = bc.case(name)
    m = result(name, gaps)
    assert (scm.replay(buf, m) == m["after"]).all()
    assert m["nflips"] == len(m["flip_by"]) == len(m["flip_bits"]) == len(m["flip_offsets"])
    runs = sbm.byte_runs(m)
    for o, p, bits in runs:  # ascending bits of one byte of one image
        assert bits == sorted(set(bits)) and 28 <= p
    assert len({(o, p) for o, p, _ in runs}) == len(runs) == len({o for o, _, _ in runs}), "an image, a byte, one run"
    assert sum(len(b) for _, _, b in runs) == m["flip_by"].count(sbm.BY_BYTE)
    by_item = m["flip_by"].count(scm.BY_ITEM)
    by_byte = {o for o, by in zip(m["flip_offsets"], m["flip_by"]) if by == sbm.BY_BYTE}
    assert m["items_repaired"] == by_item + len(by_byte)
    assert m["headers_repaired"] == m["flip_by"].count(scm.BY_HEADER)
    if not kw.get("byte_rule"):
        assert not runs and m["nflips"] == m["headers_repaired"] + m["items_repaired"]


@pytest.mark.parametrize("gaps", GAPS)
@pytest.mark.parametrize("name", NAMES)
def test_complete_is_a_fixpoint(name, gaps):
    buf, W, cfl, kw, notes = bc.case(name)
    m = result(name, gaps)
    if m["complete"] != 1:
        assert name == "stage_order_three_rounds"
        return
    again = sbm.scrub(m["after"], W, cfl, gaps=gaps, **kw)
    assert again["nflips"] == 0 and again["rounds"] == 0 and again["complete"] == 1
    assert all(again[k] == m[k] for k in ("rc", "offsets", "lens", "kind") + scm.COUNTS)
    assert (again["after"] == m["after"]).all()


def test_max_rounds_inside_a_byte_round_goes_on_from_there():
    buf, W, cfl, kw, notes = bc.case("stage_order_three_rounds")
    m = result("stage_order_three_rounds", False)
    assert m["flip_by"][-1] == sbm.BY_BYTE and m["complete"] == 0
    rest = sbm.scrub(m["after"], W, cfl, byte_rule=True)
    whole = result("stage_order", False)
    assert rest["rounds"] == 1 and rest["complete"] == 1 and (rest["after"] == whole["after"]).all()


@pytest.mark.parametrize("gaps", GAPS)
@pytest.mark.parametrize("name", [n for n in NAMES if n not in ("reached_off", "log_rounds")])
def test_rule_off_loses_what_the_rule_is_for(name, gaps):
    """With the bit clear the result is scrub_gaps_model's, and no image the
    byte stage repaired is back."""
    buf, W, cfl, kw, notes = bc.case(name)
    kw = {k: v for k, v in kw.items() if k != "byte_rule"}
    off = sbm.scrub(buf, W, cfl, gaps=gaps, byte_rule=False, **kw)
    same(off, gm.scrub(buf, W, cfl, gaps=gaps, **kw))
    on = result(name, gaps)
    for o, p, _ in sbm.byte_runs(on):
        assert off["after"][o + p] != notes["pristine"][o + p]


@pytest.mark.parametrize("gaps", GAPS)
@pytest.mark.parametrize("cases,name", OLDER, ids=[f"{c.__name__.split('.')[-1]}-{n}" for c, n in OLDER])
def test_rule_off_is_the_scrub_gaps_model(cases, name, gaps):
    buf, W, cfl, kw, notes = cases.case(name)
    kw = dict(kw, gaps=gaps or kw.get("gaps", False))
    same(sbm.scrub(buf, W, cfl, byte_rule=False, **kw), gm.scrub(buf, W, cfl, **kw))


def test_span_limit_resolution():
    assert sbm.bspan(0) == 0x10000 and sbm.bspan(300) == 300 and sbm.bspan(1 << 20) == 0x10000
    assert sbm.bspan(0x10000) == sbm.bspan(0x10001) == 0x10000


def test_a_mask_becomes_its_bits_ascending():
    assert sbm.bits([(700, 55, 0x81), (900, 28, 0x10)]) == [(700, 440, ), (700, 447), (900, 228)]
    assert sbm.bits([(0, 30, 0xFF)]) == [(0, 240 + b) for b in range(8)]


def test_edges():
    import numpy as np
    assert sbm.scrub(np.zeros(0, np.uint8), 4096, byte_rule=True)["complete"] == 1
    assert sbm.scrub(np.zeros(64, np.uint8), 64, max_span=scm.rm.SPAN_MAX + 1, byte_rule=True)["rc"] == scm.EINVAL

"""The model of crc32c_scrub_pages (tests/scrub_model.py) held to what it is
made of, on the pages of tests/scrub_cases.py (no GPU, no library call): its
two list builders against header_cases.breaks and against triage_sim.c's loops
transcribed line by line, each case's own notes, the fixpoint, the log replayed
and the final list against the triage's model of the final bytes."""
import numpy as np
import pytest

from tests import header_cases as hc
from tests import scrub_cases as sca
from tests import scrub_model as scm
from tests import triage_cases as tc
from tests import triage_model as tm

NAMES = list(sca.CASES)
_RESULTS = {}


def _result(name):
    """(case, the first triage, the model's result), computed once."""
    if name not in _RESULTS:
        buf, W, cfl, kw, notes = sca.case(name)
        _RESULTS[name] = (tm.triage_fast(buf, W, cfl), scm.scrub(buf, W, cfl, **kw))
    return sca.case(name) + _RESULTS[name]


def sim_header_todo(offs, lens, kind, n, PAGE, WBUF):
    """tests/integration/triage_sim.c, play(), stage 2's list."""
    todo = []
    k = 0
    w = 0
    while w * WBUF < PAGE:
        ps = w * WBUF
        pe = ps + WBUF if ps + WBUF < PAGE else PAGE
        end = ps
        last = -1
        while k < n and offs[k] < pe:
            if kind[k] == 4 or kind[k] == 6:
                k += 1
                continue
            if kind[k] == 0:
                todo.append(offs[k])
            last = kind[k]
            end = offs[k] + lens[k]
            k += 1
        if last != 0 and end >= ps and end <= pe and pe - end >= 48:
            todo.append(end)
        w += 1
    return todo


def sim_item_todo(offs, lens, kind, n):
    """tests/integration/triage_sim.c, play(), stage 3's list."""
    todo = []
    j = 0
    kept_end = 0
    for k in range(n):
        if kind[k] == 0 and lens[k] != 0:
            todo.append(offs[k])
        if kind[k] != 6:
            continue
        if j <= k:
            j = k + 1
        while j < n and kind[j] != 1 and kind[j] != 4:
            j += 1
        nxt = offs[j] if j < n else (1 << 64) - 1
        end = offs[k] + lens[k]
        if end > nxt or offs[k] < kept_end:
            continue
        todo.append(offs[k])
        kept_end = end
    return todo


def _pages():
    """Every scrub case's damaged page and the triage's own built cases."""
    for name in NAMES:
        buf, W, cfl, _, _ = sca.case(name)
        yield name, buf, W, cfl
    for name, (buf, W, cfl, _) in tc.built().items():
        yield "triage:" + name, buf, W, cfl


def test_list_builders_against_breaks_and_the_sim():
    for name, buf, W, cfl in _pages():
        T = tm.triage_fast(buf, W, cfl)
        args = T["offsets"], T["lens"], T["kind"]
        headers = scm.header_list(*args, len(buf), W)
        assert headers == sim_header_todo(*args, T["nitems"], len(buf), W), name
        assert headers == sorted(set(headers)), name
        assert headers == hc.breaks(buf, W, cfl).tolist(), name
        assert scm.item_list(*args) == sim_item_todo(*args, T["nitems"]), name


def test_item_list_is_piece_local():
    """A piece's part of the item list is the item list of that piece's
    entries alone (what lets a wave take a piece)."""
    for name, buf, W, cfl in _pages():
        T = tm.triage_fast(buf, W, cfl)
        whole = scm.item_list(T["offsets"], T["lens"], T["kind"])
        parts = []
        for ps in range(0, len(buf), W):
            keep = [i for i, o in enumerate(T["offsets"]) if ps <= o < ps + W]
            parts += scm.item_list(*([T[k][i] for i in keep] for k in ("offsets", "lens", "kind")))
        assert parts == whole, name


@pytest.mark.parametrize("name", NAMES)
def test_case_notes(name):
    buf, W, cfl, kw, notes, T, m = _result(name)
    args = T["offsets"], T["lens"], T["kind"]
    sca.check_notes(m, (scm.header_list(*args, len(buf), W), scm.item_list(*args), T["suspects"]), notes)
    if name == "clean":
        assert all(m[k] == T[k] for k in ("offsets", "lens", "kind") + scm.COUNTS)
    if name == "work_bound":
        assert all(m[k] == T[k] for k in ("offsets", "lens", "kind") + scm.COUNTS) and (m["after"] == buf).all()


@pytest.mark.parametrize("name", NAMES)
def test_log_replayed_gives_the_final_bytes(name):
    buf, W, cfl, kw, notes, T, m = _result(name)
    assert (scm.replay(buf, m) == m["after"]).all()
    assert m["nflips"] == m["headers_repaired"] + m["items_repaired"] == len(m["flip_by"])
    assert m["flip_by"].count(scm.BY_HEADER) == m["headers_repaired"]


@pytest.mark.parametrize("name", NAMES)
def test_final_list_is_the_triage_of_the_final_bytes(name):
    buf, W, cfl, kw, notes, T, m = _result(name)
    final = tm.triage_fast(m["after"], W, cfl)
    assert all(m[k] == final[k] for k in ("rc", "offsets", "lens", "kind") + scm.COUNTS)


@pytest.mark.parametrize("name", ["two_rounds", "suspect_promotion", "dropped_lookalike", "second_pass", "geometry"])
def test_final_list_bytewise(name):
    buf, W, cfl, kw, notes, T, m = _result(name)
    final = tm.triage_bytewise(m["after"], W, cfl)
    assert all(m[k] == final[k] for k in ("rc", "offsets", "lens", "kind") + scm.COUNTS)


@pytest.mark.parametrize("name", [n for n in NAMES if n not in ("two_rounds_one_allowed", "work_bound")])
def test_complete_is_a_fixpoint(name):
    buf, W, cfl, kw, notes, T, m = _result(name)
    assert m["complete"] == 1
    again = scm.scrub(m["after"], W, cfl, **kw)
    assert again["nflips"] == 0 and again["rounds"] == 0 and again["complete"] == 1
    assert all(again[k] == m[k] for k in ("rc", "offsets", "lens", "kind") + scm.COUNTS)
    assert (again["after"] == m["after"]).all()


def test_second_pass_is_what_the_written_out_flow_leaves():
    buf, W, cfl, kw, notes, T, m = _result("second_pass")
    once = scm.scrub(buf, W, cfl, single_pass=True)
    left, = notes["single_pass_leaves"]
    assert once["headers_repaired"] == 0 and once["items_repaired"] == 1
    assert dict(zip(once["offsets"], once["kind"])).get(left) not in (1, 4)
    assert dict(zip(m["offsets"], m["kind"]))[left] == 1


def test_no_proven_byte_changes():
    """dropped_lookalike: every flip lies in the one image kept."""
    buf, W, cfl, kw, notes, T, m = _result("dropped_lookalike")
    (o, k, by), = notes["log"]
    changed = np.flatnonzero(m["after"] != buf)
    assert changed.tolist() == [o + k // 8]


def test_edges():
    assert scm.scrub(np.zeros(0, np.uint8), 4096)["complete"] == 1
    assert scm.scrub(np.zeros(64, np.uint8), 64, max_span=scm.rm.SPAN_MAX + 1)["rc"] == scm.EINVAL

"""The model of CRC32C_SCRUB_GAPS (tests/scrub_gaps_model.py) on the pages of
tests/scrub_gaps_cases.py and tests/scrub_cases.py (no GPU, no library call):
each case's own notes, the fixpoint, the images that came back against the
pristine bytes, the lists' order, and the loop with the rule off against
tests/scrub_model.py."""
import pytest

from tests import scrub_cases as sca
from tests import scrub_gaps_cases as gc
from tests import scrub_gaps_model as gm
from tests import scrub_model as scm
from tests import triage_model as tm

NAMES = list(gc.CASES)
OLD = list(sca.CASES)
KEYS = ("rc", "offsets", "lens", "kind", "flip_offsets", "flip_bits", "flip_by", "nflips", "headers_repaired",
        "items_repaired", "rounds", "complete") + scm.COUNTS
_RESULTS = {}


def same(a, b):
    assert all(a[k] == b[k] for k in KEYS), [k for k in KEYS if a[k] != b[k]]
    assert (a["after"] == b["after"]).all()


def _result(name):
    """(case, the first triage, the model's result), computed once."""
    if name not in _RESULTS:
        buf, W, cfl, kw, notes = gc.case(name)
        _RESULTS[name] = (tm.triage_fast(buf, W, cfl), gm.scrub(buf, W, cfl, **kw))
    return gc.case(name) + _RESULTS[name]


@pytest.mark.parametrize("name", NAMES)
def test_case_notes(name):
    buf, W, cfl, kw, notes, T, m = _result(name)
    first = gm.first_lists(buf, W, cfl, kw.get("gaps", False))
    gc.check_notes(m, first, notes, dict(zip(T["offsets"], T["kind"])))
    assert (scm.replay(buf, m) == m["after"]).all()
    assert m["nflips"] == m["headers_repaired"] + m["items_repaired"] == len(m["flip_by"])


@pytest.mark.parametrize("name", NAMES)
def test_first_lists_ascend_and_name_nothing_twice(name):
    buf, W, cfl, kw, notes, T, m = _result(name)
    headers, items, _, gaps = gm.first_lists(buf, W, cfl, True)
    assert gaps == sorted(set(gaps)) and not set(gaps) & set(T["offsets"])
    assert headers == sorted(set(headers)) and items == sorted(set(items))
    assert set(gaps) <= set(headers)
    ends = {o + n for o, n, k in zip(T["offsets"], T["lens"], T["kind"]) if k == tm.SALVAGED}
    assert set(gaps) <= ends and len(gaps) <= T["nsalvaged"]


@pytest.mark.parametrize("name", NAMES)
def test_item_list_is_piece_local(name):
    """A piece's part of item_list' is item_list' of that piece's entries alone."""
    buf, W, cfl, kw, notes, T, m = _result(name)
    whole = gm.item_list(T["offsets"], T["lens"], T["kind"], buf, W, cfl)
    parts = []
    for ps in range(0, len(buf), W):
        keep = [i for i, o in enumerate(T["offsets"]) if ps <= o < ps + W]
        parts += gm.item_list(*([T[k][i] for i in keep] for k in ("offsets", "lens", "kind")), buf, W, cfl)
    assert parts == whole


@pytest.mark.parametrize("name", [n for n in NAMES if n != "chain_two_rounds"])
def test_complete_is_a_fixpoint(name):
    buf, W, cfl, kw, notes, T, m = _result(name)
    assert m["complete"] == 1
    again = gm.scrub(m["after"], W, cfl, **kw)
    assert again["nflips"] == 0 and again["rounds"] == 0 and again["complete"] == 1
    assert all(again[k] == m[k] for k in ("rc", "offsets", "lens", "kind") + scm.COUNTS)
    assert (again["after"] == m["after"]).all()


@pytest.mark.parametrize("name", NAMES)
def test_final_list_is_the_triage_of_the_final_bytes(name):
    buf, W, cfl, kw, notes, T, m = _result(name)
    final = tm.triage_fast(m["after"], W, cfl)
    assert all(m[k] == final[k] for k in ("rc", "offsets", "lens", "kind") + scm.COUNTS)


def test_chain_stops_at_max_rounds_and_goes_on_from_there():
    buf, W, cfl, kw, notes, T, m = _result("chain_two_rounds")
    rest = gm.scrub(m["after"], W, cfl, gaps=True)
    whole = _result("chain")[-1]
    assert rest["rounds"] == 1 and rest["complete"] == 1 and (rest["after"] == whole["after"]).all()


def _old(name):
    """scrub_model's result of a scrub_cases page, computed once."""
    if ("old", name) not in _RESULTS:
        buf, W, cfl, kw, notes = sca.case(name)
        _RESULTS["old", name] = scm.scrub(buf, W, cfl, **kw)
    return _RESULTS["old", name]


@pytest.mark.parametrize("name", OLD)
def test_rule_off_is_the_scrub_model(name):
    buf, W, cfl, kw, notes = sca.case(name)
    same(gm.scrub(buf, W, cfl, gaps=False, **kw), _old(name))


@pytest.mark.parametrize("name", NAMES)
def test_rule_off_is_the_scrub_model_on_the_new_pages(name):
    buf, W, cfl, kw, notes = gc.case(name)
    kw = {k: v for k, v in kw.items() if k != "gaps"}
    off = gm.scrub(buf, W, cfl, gaps=False, **kw)
    same(off, scm.scrub(buf, W, cfl, **kw))
    kinds = dict(zip(off["offsets"], off["kind"]))
    if name in ("behind", "cflags64"):  # (what the rule is for)
        assert all(kinds.get(o) not in (1, 4) for o, _ in notes["back"])


@pytest.mark.parametrize("name", [n for n in OLD if sca.case(n)[2] == 4 and not sca.case(n)[3]])
def test_rule_on_changes_no_older_page(name):
    """The single-call pages of scrub_cases.py with 4-byte client flags: the
    same result with the rule and without."""
    buf, W, cfl, kw, notes = sca.case(name)
    same(gm.scrub(buf, W, cfl, gaps=True), _old(name))


def doc_lists(offs, lens, kind, n, buf, size, W, cfl, hdr):
    """INTEGRATION.md section 4i's three loops, transcribed line by line
    (hdr: section 4f's list): (gap, hdr2, the gap starts kept for the items)."""
    gap = []
    for k in range(n):
        if kind[k] != 4:
            continue
        e = offs[k] + lens[k]
        pe = (offs[k] // W + 1) * W
        if pe > size:
            pe = size
        if e > pe or pe - e < 48:
            continue
        lo, hi = k + 1, n
        while lo < hi:
            mid = lo + (hi - lo) // 2
            if offs[mid] < e:
                lo = mid + 1
            else:
                hi = mid
        if lo < n and offs[lo] == e:
            continue
        gap.append(e)
    ng, m = len(gap), len(hdr)
    a = b = 0
    hdr2 = []
    while a < m or b < ng:
        o = hdr[a] if b == ng or (a < m and hdr[a] <= gap[b]) else gap[b]
        if a < m and hdr[a] == o:
            a += 1
        if b < ng and gap[b] == o:
            b += 1
        hdr2.append(o)
    todo, j, kept_end, g = [], 0, 0, 0
    for k in range(n + 1):
        while g < ng and (k == n or gap[g] < offs[k]):
            nt = gm.sm.sane(buf, W, gap[g], cfl)
            g += 1
            if nt == 0:
                continue
            if j < k:
                j = k
            while j < n and kind[j] != 1 and kind[j] != 4:
                j += 1
            nxt = offs[j] if j < n else (1 << 64) - 1
            end = gap[g - 1] + nt
            if end > nxt or gap[g - 1] < kept_end:
                continue
            todo.append(gap[g - 1])
            kept_end = end
        if k == n:
            break
        # section 4g's body for entry k
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
    return gap, hdr2, todo


def test_the_documents_loops_build_the_models_lists():
    pages = [gc.case(n)[:3] for n in NAMES] + [sca.case(n)[:3] for n in OLD if not n.startswith("log_")]
    for buf, W, cfl in pages:
        T = tm.triage_fast(buf, W, cfl)
        args = T["offsets"], T["lens"], T["kind"]
        gap, hdr2, todo = doc_lists(*args, T["nitems"], gm.sm._u8(buf), len(buf), W, cfl,
                                    scm.header_list(*args, len(buf), W))
        assert gap == gm.gap_starts(*args, len(buf), W)
        assert hdr2 == gm.header_list(*args, len(buf), W)
        assert todo == gm.item_list(*args, buf, W, cfl)


def test_edges():
    import numpy as np
    assert gm.scrub(np.zeros(0, np.uint8), 4096, gaps=True)["complete"] == 1
    assert gm.scrub(np.zeros(64, np.uint8), 64, max_span=scm.rm.SPAN_MAX + 1, gaps=True)["rc"] == scm.EINVAL
    assert gm.gap_starts([], [], [], 0, 4096) == []

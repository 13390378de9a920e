"""crc32c_triage_pages without a GPU: the rule's two models agree, the result
with the suspects taken out is recover_pages' (tests/recover_model.py), every
case shows what it was built to show, and the library exports the entry point
with its argument checks."""
import ctypes

import numpy as np
import pytest

from memcached_amd import _lib
from memcached_amd import crc32c as mc
from tests import recover_model as rm
from tests import triage_cases as tc
from tests import triage_model as tm

KEYS = ("rc", "offsets", "lens", "kind", "nitems", "nbad", "nsalvaged", "nsuspect", "scanned", "ncand", "suspects")


@pytest.fixture(scope="module")
def cases():
    out = tc.built()
    out.update(tc.reused())
    return out


@pytest.fixture(scope="module")
def fast(cases):
    return {name: tm.triage_fast(buf, W, cfl) for name, (buf, W, cfl, _) in cases.items()}


BUILT = ["behind_nkey0", "walked_bad_is_not_listed_twice", "suspect_inside_found", "found_inside_suspect",
         "many_rounds", "work_bound"]


def test_the_case_list_is_complete(cases):
    assert set(BUILT) == set(tc.built()) and len(cases) >= len(BUILT) + 20


@pytest.mark.parametrize("name", BUILT)
def test_bytewise_and_fast_agree_on_the_built_cases(cases, fast, name):
    buf, W, cfl, _ = cases[name]
    slow = tm.triage_bytewise(buf, W, cfl)
    assert {k: slow[k] for k in KEYS} == {k: fast[name][k] for k in KEYS}


def test_bytewise_and_fast_agree_on_the_reused_cases(cases, fast):
    """(config5_case(8), 32 MiB, is left to the fast form: one offset at a time
    in Python it takes minutes.)"""
    for name in tc.reused():
        buf, W, cfl, _ = cases[name]
        slow = tm.triage_bytewise(buf, W, cfl)
        assert {k: slow[k] for k in KEYS} == {k: fast[name][k] for k in KEYS}, name


def _invariant(m, buf, W, cfl):
    want = rm.recover(buf, W, cfl)
    got = tm.without_suspects(m)
    assert got == {k: want[k] for k in got}
    assert m["nitems"] == want["nitems"] + m["nsuspect"]


def test_without_the_suspects_it_is_recover(cases, fast):
    for name, (buf, W, cfl, _) in cases.items():
        _invariant(fast[name], buf, W, cfl)


def test_each_case_shows_what_it_was_built_for(cases, fast):
    for name, (buf, W, cfl, notes) in cases.items():
        m = fast[name]
        tc.check_notes(m, notes)
        # a suspect is a candidate (its length is never 0), outside the other two lists
        others = set(m["walked"].tolist()) | set(m["found"])
        for o, n, k in zip(m["offsets"], m["lens"], m["kind"]):
            assert k != tm.SUSPECT or (n != 0 and o not in others), (name, o)
    assert fast["behind_nkey0"]["nsuspect"] == 4
    assert fast["found_inside_suspect"]["nsuspect"] == 1
    # (38 damaged images behind the header, and one look-alike 9 bytes into one of them: triage_cases.check_notes)
    assert fast["many_rounds"]["nsuspect"] == 38 + 1 and fast["many_rounds"]["ncand"] > 4 * 64
    m = fast["work_bound"]
    assert m["rc"] == tm.EWORK and m["nsuspect"] == m["nsalvaged"] == 0 and m["nitems"] == len(m["walked"]) > 50
    # the suspect of found_inside_suspect spans images that are found all the same
    m = fast["found_inside_suspect"]
    p, = m["suspects"]
    n = m["lens"][m["offsets"].index(p)]
    assert sum(1 for o in m["found"] if p < o < p + n) == 2


def test_config5_has_no_suspects_and_is_recover():
    buf, W, cfl, notes = tc.config5()
    m = tm.triage_fast(buf, W, cfl)
    tc.check_notes(m, notes)
    _invariant(m, buf, W, cfl)
    assert m["nsalvaged"] == 306 + 606 + 1000


def test_the_out_of_order_ops_are_self_consistent():
    """tests/triage_interleave_cases.py: counts match arrays, sentinels in place,
    the early return leaves the walk's part."""
    from tests import interleave_cases as ic
    from tests import triage_interleave_cases as tic
    for op in tic.table():
        w, cap = op.want, op.inputs["cap"]
        for key, size in (("offsets", 8), ("lens", 4), ("kind", 1)):
            assert w[key].size == cap + 1 and w[key][-1] == ic.SENT[size] and not w[key].flags.writeable
        k = min(cap, w["nitems"])
        kind = w["kind"][:k]
        assert (np.diff(w["offsets"][:k].astype(np.int64)) > 0).all() and set(kind.tolist()) <= {0, 1, 4, 6}
        assert (w["kind"][k:] == ic.SENT[1]).all() and np.array_equal(w["buf"], op.inputs["buf"])
        if cap >= w["nitems"]:
            assert ((kind == 4).sum(), (kind == 6).sum(), (kind == 0).sum()) == (w["nsalvaged"], w["nsuspect"],
                                                                                 w["nbad"])
        assert (w["lens"][:k][kind == 6] != 0).all()
        if op.error:
            assert w["rc"] == ic.EWORK and w["nsuspect"] == w["nsalvaged"] == 0 and set(kind.tolist()) <= {0, 1}
    assert any(op.inputs["cap"] < op.want["nitems"] for op in tic.table())


def _abi_call(buf, *, base=True, nitems=True, nbad=True, nsalvaged=True, nsuspect=True, W=4096, cap=0, arrays=None):
    c = [ctypes.c_uint64(7) for _ in range(6)]
    ref = [ctypes.byref(x) if on else None for x, on in zip(c, (nitems, nbad, nsalvaged, nsuspect, True, True))]
    rc = _lib.lib.crc32c_triage_pages(buf.ctypes.data if base else None, buf.size, W, *(arrays or (None, None, None)),
                                      cap, *ref, 0, None)
    return rc, [x.value for x in c]


def test_the_library_exports_triage_pages_with_its_argument_checks():
    assert "crc32c_triage_pages" in _lib.EXPORTED and _lib.CRC32C_ITEM_SUSPECT == 6
    buf, W, cfl, _ = tc.behind_nkey0()
    for null in ("base", "nitems", "nbad", "nsalvaged", "nsuspect"):
        rc, counts = _abi_call(buf, **{null: False})
        assert rc == _lib.CRC32C_EINVAL and counts == [7] * 6, null
    assert _abi_call(buf, W=0)[0] == _lib.CRC32C_EINVAL
    offs = np.zeros(4, np.uint64)
    assert _abi_call(buf, cap=4, arrays=(offs.ctypes.data, None, None))[0] == _lib.CRC32C_EINVAL
    # a good call: no device, no answer (and no CPU fallback); with one, the model's counts
    rc, counts = _abi_call(buf, W=W)
    if _lib.lib.crc32c_gpu_count() > 0:
        m = tm.triage_fast(buf, W, cfl)
        assert rc == _lib.CRC32C_OK
        assert counts == [m[k] for k in ("nitems", "nbad", "nsalvaged", "nsuspect", "scanned", "ncand")]
    else:
        assert rc == _lib.CRC32C_ENODEV and counts == [7] * 6


def test_the_python_face_raises_without_a_device():
    buf, W, cfl, _ = tc.behind_nkey0()
    if _lib.lib.crc32c_gpu_count() > 0:
        assert mc.triage_pages(buf, W)[3]["nsuspect"] == 4
        return
    with pytest.raises(mc.Crc32cError) as e:
        mc.triage_pages(buf, W)
    assert e.value.rc == _lib.CRC32C_ENODEV
    with pytest.raises(ValueError):
        mc.triage_pages(buf, 0)

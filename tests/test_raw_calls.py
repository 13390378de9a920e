"""The checkers of tests/raw_calls.py are where a weakened assertion of the
page-recovery GPU tests would hide, so each is shown a hand-made result that
matches a hand-made model, and then the same result with one thing wrong at a
time: every deviation must raise.  Also the padding of Side.out and the
expected-array builders, on the host side.  No GPU and no library."""
import copy

import numpy as np
import pytest

from . import raw_calls as raw

PAD = raw.EXTRA
NAMES = raw.TRIAGE_COUNTS
LISTED = dict(raw.LISTED)
SCRUB = dict(raw.SCRUB_LISTS)
CAPS = [0, 1, 2, 3, 4, 6]  # below, at (3) and above the model's length, and none


def _model():
    """Three listed entries and two flips."""
    m = dict(rc=0, offsets=[48, 1000, 70000], lens=[52, 4165, 300], kind=[1, 4, 6], nitems=3, nbad=1, nsalvaged=1,
             nsuspect=1, scanned=9000, ncand=7, flip_offsets=[1000, 70000], flip_bits=[259, 8 * 100 + 3],
             flip_by=[1, 2], nflips=2, headers_repaired=1, items_repaired=1, rounds=2, complete=1)
    m["after"] = np.arange(64, dtype=np.uint8)
    return m


def _filled(values, room, dtype):
    """What a call leaves in an array of room + PAD words."""
    a = np.full(room + PAD, raw.SENT[np.dtype(dtype).itemsize], dtype)
    k = min(room, len(values))
    a[:k] = values[:k]
    return a


def _listed(cap, m):
    got = {"rc": m["rc"], "after": m["after"].copy()}
    got.update((k, m[k]) for k in NAMES)
    got.update((name, _filled(m[name], cap, dtype)) for name, dtype in LISTED.items())
    return got


def _scrubbed(cap, flip_cap, m):
    got = {"rc": m["rc"], "after": m["after"].copy(), "rooms": {}}
    got.update((w, m[w]) for w in raw.SCRUB_WORDS)
    for k, (name, dtype) in enumerate(SCRUB.items()):
        got["rooms"][name] = cap if k < 3 else flip_cap
        got[name] = _filled(m[name], got["rooms"][name], dtype)
    return got


def _deviations(got, arrays, words, rooms, lengths):
    """(what, the result with that one thing wrong) for every kind of deviation."""
    def changed(key, value=None, at=None):
        bad = copy.deepcopy(got)
        if at is None:
            bad[key] = value
        else:
            bad[key][at] ^= 1
        return bad

    yield "rc", changed("rc", got["rc"] - 1)
    for w in words:
        yield w, changed(w, got[w] + 1)
    for name in arrays:
        k = min(rooms[name], lengths[name])
        if k:
            yield f"{name}[{k - 1}]", changed(name, at=k - 1)
            yield f"{name}[0]", changed(name, at=0)
        yield f"{name} behind {k}", changed(name, at=k)
        yield f"{name} last word", changed(name, at=-1)


@pytest.mark.parametrize("cap", CAPS)
def test_expect_listed(cap):
    m = _model()
    got = _listed(cap, m)
    raw.expect_listed(got, cap, m, NAMES)
    raw.expect_unchanged(got, m["after"])
    n = 0
    for what, bad in _deviations(got, LISTED, NAMES, dict.fromkeys(LISTED, cap), dict.fromkeys(LISTED, 3)):
        with pytest.raises(AssertionError):
            raw.expect_listed(bad, cap, m, NAMES, tag=what)
            pytest.fail(f"cap {cap}: {what} wrong, and the checker passed")
        n += 1
    assert n == 1 + len(NAMES) + 3 * (4 if cap else 2)


@pytest.mark.parametrize("cap", CAPS)
def test_expect_listed_without_lens(cap):
    """lens=False takes the expected answer without its lengths, and lets go of
    nothing else: the words behind the lengths are still checked."""
    m = _model()
    got = _listed(cap, m)
    k = min(cap, 3)
    if k:
        got["lens"][k - 1] ^= 1
        with pytest.raises(AssertionError):
            raw.expect_listed(got, cap, m, NAMES)
    del m["lens"]
    raw.expect_listed(got, cap, m, NAMES, lens=False)
    for what, bad in _deviations(got, LISTED, NAMES, dict.fromkeys(LISTED, cap), dict.fromkeys(LISTED, 3)):
        if what in ("lens[0]", f"lens[{k - 1}]"):
            continue
        with pytest.raises(AssertionError):
            raw.expect_listed(bad, cap, m, NAMES, lens=False, tag=what)
            pytest.fail(f"cap {cap}: {what} wrong, and the checker passed")


def test_expect_listed_one_array_and_fewer_counts():
    """The salvage call's shape: offsets alone and three counts."""
    m = dict(rc=raw.EINVAL, offsets=[], nfound=raw.SENT64, scanned=raw.SENT64, ncand=raw.SENT64)
    got = dict(m, offsets=_filled([], 8, np.uint64))
    raw.expect_listed(got, 8, m, raw.SALVAGE_COUNTS, arrays=("offsets",))
    for what, bad in _deviations(got, ("offsets",), raw.SALVAGE_COUNTS, {"offsets": 8}, {"offsets": 0}):
        with pytest.raises(AssertionError):
            raw.expect_listed(bad, 8, m, raw.SALVAGE_COUNTS, arrays=("offsets",), tag=what)
            pytest.fail(f"{what} wrong, and the checker passed")


def test_an_array_without_a_word_behind_its_room_is_refused():
    m = _model()
    got = _listed(3, m)
    got["kind"] = got["kind"][:3]
    with pytest.raises(AssertionError):
        raw.expect_listed(got, 3, m, NAMES)
    got = _scrubbed(3, 2, m)
    got["flip_by"] = got["flip_by"][:2]
    with pytest.raises(AssertionError):
        raw.expect_scrub(got, m)


@pytest.mark.parametrize("flip_cap", [0, 1, 2, 4])
@pytest.mark.parametrize("cap", [0, 2, 3, 5])
def test_expect_scrub(cap, flip_cap):
    m = _model()
    got = _scrubbed(cap, flip_cap, m)
    raw.expect_scrub(got, m)
    lengths = {name: 3 if k < 3 else 2 for k, name in enumerate(SCRUB)}
    for what, bad in _deviations(got, SCRUB, raw.SCRUB_WORDS, got["rooms"], lengths):
        with pytest.raises(AssertionError):
            raw.expect_scrub(bad, m)
            pytest.fail(f"caps {cap}, {flip_cap}: {what} wrong, and the checker passed")
    bad = copy.deepcopy(got)
    bad["after"][17] ^= 0x40
    with pytest.raises(AssertionError):
        raw.expect_scrub(bad, m)
    # after: the bytes expected in place of the model's
    raw.expect_scrub(bad, m, after=bad["after"])
    with pytest.raises(AssertionError):
        raw.expect_scrub(got, m, after=bad["after"])


def test_expect_unchanged():
    buf = np.arange(300, dtype=np.uint8)
    raw.expect_unchanged({"after": buf.copy()}, buf)
    for at in (0, 150, 299):
        after = buf.copy()
        after[at] ^= 0x01
        with pytest.raises(AssertionError):
            raw.expect_unchanged({"after": after}, buf)
    with pytest.raises(AssertionError):
        raw.expect_unchanged({"after": buf[:-1].copy()}, buf)


@pytest.mark.parametrize("dtype", [np.uint8, np.uint32, np.uint64])
def test_out_ended_and_capped(dtype):
    size = np.dtype(dtype).itemsize
    sent = raw.SENT[size]
    assert sent == int.from_bytes(b"\x5a" * size, "little")
    side = raw.Side(where="host")
    for n in (0, 1, 5):
        a = side.out(n, dtype)
        assert a.dtype == dtype and a.size == n + raw.EXTRA == n + 4 and (a == sent).all()
        assert side.out(n, dtype, pad=1).size == n + 1
        assert raw.Side(where=False, pad=1).out(n, dtype).size == n + 1
    values = [3, 1, 4, 1, 5]
    e = raw.ended(values, dtype)
    assert e.dtype == dtype and e.tolist() == values + [sent] and not e.flags.writeable
    for cap in (0, 3, 5, 8):
        c = raw._capped(values, cap, dtype)
        k = min(cap, 5)
        assert c.dtype == dtype and c.size == cap + 1 and not c.flags.writeable
        assert c[:k].tolist() == values[:k] and (c[k:] == sent).all()
        # what a call leaves in a one-word-padded array of this room is what _capped expects
        got = side.out(cap, dtype, pad=1)
        got[:k] = values[:k]
        assert np.array_equal(side.host(got, dtype), c)
    assert np.array_equal(raw._capped(values, 5, dtype), raw.ended(values, dtype))


def test_a_host_side_needs_no_gpu_and_copies():
    side = raw.Side(where=False)
    assert (side.dev, side.where, side.handle, side.flags(), side.flags(True, locate_only=True, gaps=False)) == (
        False, "host", None, 0, raw.CFLAGS64 | raw.LOCATE_ONLY)
    buf = np.arange(16, dtype=np.uint8)
    page = side.data(buf)
    assert page is not buf and np.array_equal(page, buf) and side.desc(None) is None
    view = np.zeros(16, np.uint8)
    assert raw.Side(where="host").adopt(view).data(buf) is view
    assert raw.ptr(None) is None and raw.ptr(view) == view.ctypes.data


def test_the_repair_callers_hold_the_copies_whose_addresses_they_pass():
    """The library gets bare addresses: the copy of the list must be alive when the call is made."""
    buf, offs = np.arange(64, dtype=np.uint8), np.array([0, 8, 16], np.uint64)
    side, keep, spec, arrays, ptrs, args = raw._list_call(False, buf, offs, None, (("ok", np.uint8),), ())
    assert args == [keep[0].ctypes.data, 64, keep[1].ctypes.data, 3]
    assert np.array_equal(keep[1], offs) and keep[1] is not offs and ptrs == [arrays["ok"].ctypes.data]
    assert raw._list_call(side, buf, offs, 2, (("ok", np.uint8),), ("buf", "offsets", "ok"))[4:] == ([None], [None, 64, None, 2])

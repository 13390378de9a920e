"""crc32c_salvage_pages without a GPU: the rule's two restatements
(tests/salvage_model.py) agree on every test buffer, hand-built buffers have
the answers written out by hand, the HIP-free arithmetic the kernels share
(memcached_amd/csrc/salvage_geom.h) matches the model when a stand-alone
program runs it, and the C ABI carries the new call."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from memcached_amd import _lib
from tests import salvage_cases as sc
from tests import salvage_model as sm

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


@pytest.fixture(scope="module")
def cases():
    out = dict(sc.small_cases())
    out["hand_built"] = sc.hand_built() + (4,)
    # the large GPU cases, cut down to what the byte-by-byte model can cross
    out["alignment_40_wbufs"] = sc.alignment_case(40) + (4,)
    return out


@pytest.fixture(scope="module")
def geom_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("salvage_geom") / "salvage_geom_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-I", os.path.join(ROOT, "memcached_amd", "csrc"),
                    os.path.join(HERE, "integration", "salvage_geom_check.cpp"), "-o", exe], check=True)
    return exe


def _both(buf, W, cfl):
    lists = sc.walk_lists(buf, W, cfl)
    return [(None, None), lists]


def test_the_two_models_agree_and_stay_within_the_work_bound(cases):
    for name, (buf, W, cfl) in cases.items():
        for walked, ok in _both(buf, W, cfl):
            slow = sm.salvage_bytewise(buf, W, walked, ok, cfl)
            fast = sm.salvage_fast(buf, W, walked, ok, cfl)
            assert slow == fast, name
            found, scanned, ncand, work = fast
            # the bound never hides a miss in the GPU tests
            assert work <= sm.WORK_MAX * (scanned + W), name
            assert ncand >= len(found), name
            assert all(a < b for a, b in zip(found, found[1:])), name


def test_the_large_cases_stay_within_the_work_bound():
    for buf, W in (sc.alignment_case(300), sc.config5_case(2)):
        found, scanned, ncand, work = sm.salvage_fast(buf, W)
        assert work <= sm.WORK_MAX * (scanned + W)
        assert len(found) >= 2


def test_hand_built_answers():
    buf, W = sc.hand_built()
    walked, ok = sc.walk_lists(buf, W)
    assert walked.tolist() == [0, 1000] and ok.tolist() == [1, 1]  # the walk stops at image 2
    # with the lists: [0, 2000) is covered; offsets 2000 .. 16384 - 48 are eligible
    found, scanned, ncand, work = sm.salvage_bytewise(buf, W, walked, ok)
    assert found == [3000, 4000]
    assert scanned == 16384 - 47 - 2000 == 14337
    assert ncand == 2 and work == 2 * (1000 - 32)
    # without them every intact image is found from scratch
    found, scanned, ncand, work = sm.salvage_bytewise(buf, W)
    assert found == [0, 1000, 3000, 4000]
    assert scanned == 16384 - 47 == 16337
    assert ncand == 4
    # an entry marked good whose header is not sane covers nothing
    found, scanned, _, _ = sm.salvage_bytewise(buf, W, np.array([0, 1000, 2000], np.uint64), np.array([1, 0, 1]))
    assert found == [1000, 3000, 4000] and scanned == 16337 - 1000


def test_outcomes_of_the_named_cases(cases):
    def run(name, lists=True):
        buf, W, cfl = cases[name]
        walked, ok = sc.walk_lists(buf, W, cfl) if lists else (None, None)
        return sm.salvage_fast(buf, W, walked, ok, cfl), (walked, ok)
    # header damage of every kind: everything the walk lost behind it comes back
    for name in sc.HEADER_DAMAGE:
        (found, *_), (walked, ok) = run("hdr_" + name)
        (whole, *_), _ = run("hdr_" + name, lists=False)
        assert len(found) >= 3, name
        good = set(walked[ok != 0].tolist())
        assert set(whole) == good | set(found), name
    # data damage only: nothing to find, the damaged images' bytes are scanned
    (found, scanned, _, _), (walked, ok) = run("data_only")
    assert found == [] and int((ok == 0).sum()) == 2
    buf, W, _ = cases["data_only"]
    tails = sum(max(0, (W - 47) - (int(o) % W + sm.ntotal_at(buf, int(o))[0]))
                for o in walked.tolist() if int(o) == max(walked[walked // W == int(o) // W].tolist()))
    bad = sum(sm.ntotal_at(buf, int(o))[0] for o in walked[ok == 0].tolist())
    assert scanned == bad + tails
    # the look-alike inside an intact image is covered; inside the damaged one it is reported
    (found, *_), _ = run("lookalike_in_intact")
    (inside, *_), _ = run("lookalike_in_damaged")
    buf, W, _ = cases["lookalike_in_damaged"]
    assert any(sm.intact(buf, W, o) == 1777 for o in inside)
    buf, W, _ = cases["lookalike_in_intact"]
    assert not any(sm.intact(buf, W, o) == 1777 for o in found)
    # one byte short of fitting: not reported
    (a, *_), _ = run("ends_exact")
    (b, *_), _ = run("ends_one_short")
    assert len(a) == len(b) + 1 and a[:-1] == b
    assert run("under_48_bytes")[0] == ([], 0, 0, 0)


def test_the_work_bound_case_is_over_the_bound():
    buf, W = sc.work_bound_case()
    found, scanned, ncand, work = sm.salvage_fast(buf, W, *sc.walk_lists(buf, W))
    assert work > sm.WORK_MAX * (scanned + W) and found == [] and ncand > 800
    assert sm.salvage_bytewise(buf, W, *sc.walk_lists(buf, W)) == (found, scanned, ncand, work)


def test_region_cuts_and_tiles_of_the_shared_header(cases, geom_exe):
    """The header's cuts, run as k_salvage_regions runs them, give the model's
    eligible ranges for every case and base alignment, and the tiles partition
    them inside aligned 4 KiB blocks (the program checks that itself)."""
    for name, (buf, W, cfl) in cases.items():
        for walked, ok in _both(buf, W, cfl):
            want = sm.regions(buf, W, walked, ok, cfl)
            lines = []
            if walked is not None:
                for o, good in zip(walked.tolist(), ok.tolist()):
                    nt = sm.sane(buf, W, o, cfl) if good else 0
                    lines.append(f"{o} {o + nt}")
            for ba in (0, 16, 4095, 1001):
                r = subprocess.run([geom_exe, "regions", str(W), str(len(buf)), str(ba)], input="\n".join(lines),
                                   capture_output=True, text=True, timeout=120)
                assert r.returncode == 0 and "salvage_geom ok" in r.stdout, (name, r.stderr)
                got, ntiles = [], 0
                for ln in r.stdout.splitlines():
                    t = ln.split()
                    if t[0] == "r":
                        lo, hi, pe = map(int, t[1:])
                        assert pe == sm.piece_end(lo, W, len(buf))
                        # ranges of one piece that touch are one run of the model's
                        if got and got[-1][1] == lo and lo % W != 0:
                            got[-1][1] = hi
                        else:
                            got.append([lo, hi])
                    elif t[0] == "t":
                        ntiles += 1
                assert [tuple(x) for x in got] == want, (name, ba)
                assert ntiles >= sum((ba + hi - 1) // 4096 - (ba + lo) // 4096 + 1 for lo, hi in want)


def test_region_cuts_of_hand_made_lists(geom_exe):
    """Lists that are no walk's: a covering image that reaches past later
    entries (the running maximum of the ends), entries that cover nothing."""
    buf, W = sc.hand_built()
    for lst, flags in (([0, 500, 1000, 2000], [1, 0, 0, 1]), ([0, 10, 500, 999, 1000, 1001, 3000], [1, 1, 0, 1, 1, 0, 1]),
                       ([3000], [1]), ([4000], [0])):
        want = sm.regions(buf, W, np.array(lst), np.array(flags))
        assert sm.salvage_bytewise(buf, W, np.array(lst), np.array(flags)) == \
            sm.salvage_fast(buf, W, np.array(lst), np.array(flags))
        lines = [f"{o} {o + (sm.sane(buf, W, o) if good else 0)}" for o, good in zip(lst, flags)]
        r = subprocess.run([geom_exe, "regions", str(W), str(len(buf)), "48"], input="\n".join(lines),
                           capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        got = []
        for t in (ln.split() for ln in r.stdout.splitlines()):
            if t[0] == "r":
                lo, hi = int(t[1]), int(t[2])
                if got and got[-1][1] == lo:
                    got[-1][1] = hi
                else:
                    got.append([lo, hi])
        assert [tuple(x) for x in got] == want, lst
    assert sm.regions(buf, W, np.array([0, 500, 1000, 2000]), np.array([1, 0, 0, 1]))[0][0] == 1000


def test_header_test_and_work_bound_of_the_shared_header(geom_exe):
    rng = np.random.default_rng(5)
    rows = []
    for _ in range(4000):
        nbytes = int(rng.choice([0, 1, 2, 50, 4100, (1 << 31) - 1, 1 << 31, 0x7FFF0000, 0x7FFEFFF0,
                                 int(rng.integers(0, 1 << 32))]))
        flags = int(rng.choice([0, 2, 256, 258, 0xFFFF, int(rng.integers(0, 1 << 16))]))
        nkey = int(rng.choice([0, 1, 255, int(rng.integers(0, 256))]))
        room = int(rng.choice([48, 60, 4165, 1 << 22, 1 << 33, 49 + nkey + nbytes, 49 + nkey + nbytes + 12]))
        rows.append((nbytes, flags, nkey, int(rng.choice([4, 8])), room))
    r = subprocess.run([geom_exe, "span"], input="\n".join(" ".join(map(str, x)) for x in rows),
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    for (nbytes, flags, nkey, cfl, room), got in zip(rows, map(int, r.stdout.split())):
        nt = 48 + nkey + 1 + nbytes + (cfl if flags & 256 else 0) + (8 if flags & 2 else 0)
        ok = nkey != 0 and nbytes < 1 << 31 and nt - 32 <= sm.MAX_SPAN and nt <= room
        assert got == (nt if ok else 0), (nbytes, flags, nkey, cfl, room)
    rows = [(w, s, W) for W in (1, 4096, 1 << 22) for s in (0, 1, 12345, 1 << 40)
            for w in (0, 64 * (s + W) - 1, 64 * (s + W), 64 * (s + W) + 1, (1 << 64) - 1)]
    r = subprocess.run([geom_exe, "work"], input="\n".join(" ".join(map(str, x)) for x in rows),
                       capture_output=True, text=True, timeout=120)
    assert [int(x) for x in r.stdout.split()] == [int(w > sm.WORK_MAX * (s + W)) for w, s, W in rows]


def test_abi_symbol_constants_and_enodev():
    assert "crc32c_salvage_pages" in _lib.EXPORTED and hasattr(_lib.lib, "crc32c_salvage_pages")
    assert _lib.CRC32C_EWORK == -7 and _lib.CRC32C_SALVAGE_WORK_MAX == sm.WORK_MAX == 64
    assert b"work bound" in _lib.lib.crc32c_strerror(_lib.CRC32C_EWORK)
    buf, W = sc.hand_built()
    offs = np.full(8, 0xAB, np.uint64)
    counts = [ctypes.c_uint64(0x5A5A) for _ in range(3)]
    call = _lib.lib.crc32c_salvage_pages
    # bad arguments are refused before anything else
    refs = [ctypes.byref(c) for c in counts]
    assert call(None, buf.size, W, None, None, 0, offs.ctypes.data, 8, *refs, 0, None) == _lib.CRC32C_EINVAL
    assert call(buf.ctypes.data, buf.size, 0, None, None, 0, offs.ctypes.data, 8, *refs, 0, None) == _lib.CRC32C_EINVAL
    assert call(buf.ctypes.data, buf.size, W, None, None, 0, None, 8, *refs, 0, None) == _lib.CRC32C_EINVAL
    assert call(buf.ctypes.data, buf.size, W, offs.ctypes.data, None, 2, offs.ctypes.data, 8, *refs, 0,
                None) == _lib.CRC32C_EINVAL
    assert call(buf.ctypes.data, buf.size, W, None, None, 0, offs.ctypes.data, 8, None, refs[1], refs[2], 0,
                None) == _lib.CRC32C_EINVAL
    if _lib.lib.crc32c_gpu_count() == 0:
        rc = call(buf.ctypes.data, buf.size, W, None, None, 0, offs.ctypes.data, 8, *refs, 0, None)
        assert rc == _lib.CRC32C_ENODEV
    assert (offs == 0xAB).all() and all(c.value == 0x5A5A for c in counts)

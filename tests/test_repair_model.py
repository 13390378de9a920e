"""crc32c_repair_items without a GPU: the rule's two statements
(tests/repair_model.py: every bit inverted and the CRC recomputed through the
oracle; the syndrome sequence g(t)) agree, two inverted bits are never taken
for one, the host scalar crc32c_locate_bit of the built library gives the
model's answers, the HIP-free arithmetic the kernels share
(memcached_amd/csrc/repair_geom.h) passes its stand-alone check under the
sanitizers, and the C ABI refuses to work without a device."""
import ctypes
import itertools
import os
import subprocess

import numpy as np
import pytest

from memcached_amd import _lib
from memcached_amd import crc32c as mc
from tests import repair_model as rm
from tests import salvage_cases as sc

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def _flip(img, k):
    out = np.frombuffer(bytes(img), np.uint8).copy()
    out[k // 8] ^= 1 << (k % 8)
    return out


def _explains(img, k):
    """The rule as written, for one bit: with bit k inverted, stored == computed."""
    return rm.syndrome(_flip(img, k))[0] == 0


@pytest.fixture(scope="module")
def geom_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("repair_geom") / "repair_geom_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-I", os.path.join(ROOT, "memcached_amd", "csrc"),
                    os.path.join(HERE, "integration", "repair_geom_check.cpp"),
                    os.path.join(ROOT, "memcached_amd", "csrc", "crc32c_host.cpp"), "-o", exe], check=True)
    return exe


def test_the_two_statements_agree_on_every_bit_of_short_images():
    rng = np.random.default_rng(52)
    for nt in range(52, 81):
        img = sc.image_nt(rng, nt, cas=nt >= 60 and bool(nt & 1))
        assert rm.located_brute(img) == rm.located_syndrome(img) == []
        g = [rm.ONE]
        for _ in range(32 + 8 * (nt - 32)):
            g.append(rm.step(g[-1]))
        for k in range(224, 8 * nt):
            bad = _flip(img, k)
            assert rm.located_brute(bad) == rm.located_syndrome(bad) == [k], (nt, k)
            assert rm.t_of_k(k, nt) < 32 + 8 * (nt - 32) and rm.k_of_t(rm.t_of_k(k, nt), nt) == k
            assert g[rm.t_of_k(k, nt)] == rm.syndrome(bad)[0]
        assert rm.xpow(len(g) - 1) == g[-1]


@pytest.mark.parametrize("nt", [4165, (1 << 20) + 77])
def test_the_two_statements_agree_on_sampled_bits_of_long_images(nt):
    rng = np.random.default_rng(nt)
    img = sc.image_nt(rng, nt, cas=True)
    ks = set(rm.boundary_bits(nt)) | set(rng.integers(224, 8 * nt, 24).tolist())
    for k in sorted(ks):
        bad = _flip(img, k)
        assert rm.located_syndrome(bad) == [k], (nt, k)
        assert _explains(bad, k)
        other = int(rng.integers(224, 8 * nt))
        assert _explains(bad, other) == (other == k)


def test_every_two_bit_pattern_of_a_52_byte_image_is_not_located():
    rng = np.random.default_rng(2)
    img = sc.image_nt(rng, 52)
    pairs = list(itertools.combinations(range(224, 8 * 52), 2))
    assert len(pairs) == 192 * 191 // 2
    for a, b in pairs:
        assert rm.located_syndrome(_flip(_flip(img, a), b)) == [], (a, b)
    for a, b in pairs[::997]:
        bad = _flip(_flip(img, a), b)
        assert rm.located_brute(bad) == []
        assert rm.repair_one(bad, 0) == (0, rm.NO_BIT) == rm.repair_one(bad, 0, brute=True)


def test_verdicts_of_one_image():
    rng = np.random.default_rng(3)
    img = sc.image_nt(rng, 77, cas=True)
    assert rm.repair_one(img, 0) == (1, rm.NO_BIT)
    for k in range(224, 8 * 77):
        want = (0, rm.NO_BIT) if rm.length_bit(k) else (rm.REPAIRED, k)
        bad = _flip(img, k)
        if rm.length_bit(k):  # (the image is then judged by its new length: pad so that it can still be sane)
            bad = np.concatenate([bad, np.zeros(1 << 16, np.uint8)])
            nt = rm.sm.sane(bad, 1 << 62, 0)
            if nt and nt - 32 <= rm.SPAN_DEFAULT:
                assert rm.repair_one(bad, 0) == rm.repair_one(bad, 0, brute=nt < 400)
            continue
        assert rm.repair_one(bad, 0) == rm.repair_one(bad, 0, brute=True) == want, k
    # bytes 0..27 are not covered: intact
    assert rm.repair_one(_flip(img, 100), 0) == (1, rm.NO_BIT)
    # no CRLF at the end (and the stored CRC stamped over that): a located bit is not accepted
    raw = np.frombuffer(bytes(sc.raw_image(rng, 300, b"xy")), np.uint8)
    assert rm.repair_one(raw, 0) == (1, rm.NO_BIT)
    assert rm.repair_one(_flip(raw, 8 * 100 + 3), 0) == (0, rm.NO_BIT)
    # a bit of the CRLF itself is repaired: the test is made after the flip
    assert rm.repair_one(_flip(img, 8 * 76 + 1), 0) == (rm.REPAIRED, 8 * 76 + 1)
    # longer than max_span; not sane
    assert rm.repair_one(_flip(img, 300), 0, max_span=44) == (0, rm.NO_BIT)
    assert rm.repair_one(_flip(img, 300), 0, max_span=45) == (rm.REPAIRED, 300)
    assert rm.repair_one(img[:60], 0) == (0, rm.NO_BIT)


def _locate_cases():
    rng = np.random.default_rng(4)
    cases = [(5, 5, 100), (0, 0, 0), (rm.ONE, 0, 0), (1, 0, 0), (rm.ONE, 0, rm.SPAN_MAX + 1), (3, 0, 20)]
    for length in (0, 1, 2, 20, 251, 252, 253, 4133):
        npos = 32 + 8 * length
        for t in sorted({0, 7, 8, 31, 32, npos - 1, npos} | set(rng.integers(0, npos, 12).tolist())):
            e = int(rng.integers(0, 1 << 32))
            cases.append((rm.xpow(t) ^ e, e, length))
        a, b = rng.integers(0, npos, 2).tolist()
        if a != b:
            cases.append((rm.xpow(a) ^ rm.xpow(b), 0, length))
    length = (1 << 20) + 45
    for t in (0, 32 + 8 * length - 1, 8 * 256 * 1000 - 1, 8 * 256 * 1000, 5555555):
        cases.append((rm.xpow(t), 0, length))
    cases.append((rm.xpow(32 + 8 * length), 0, length))
    return cases


def test_locate_bit_of_the_built_library_equals_the_model(geom_exe):
    cases = _locate_cases()
    want = [rm.locate_bit(*c) for c in cases]
    assert rm.NO_BIT in want and 0 in want and 31 in want and sum(w != rm.NO_BIT for w in want) > 80
    assert [mc.locate_bit(*c) for c in cases] == want
    assert _lib.CRC32C_NO_BIT == rm.NO_BIT and _lib.CRC32C_REPAIR_SPAN_MAX == rm.SPAN_MAX
    # the same source, compiled with the sanitizers
    r = subprocess.run([geom_exe, "locate"], input="\n".join(" ".join(map(str, c)) for c in cases),
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert [int(x) for x in r.stdout.split()] == want


def test_locate_bit_finds_real_damage():
    """From CRCs of real bytes, not of powers of x: one inverted bit of a span or of its stored CRC."""
    from tests import oracle
    rng = np.random.default_rng(5)
    for length in (1, 20, 4133):
        span = rng.integers(0, 256, length, dtype=np.uint8)
        stored = oracle.crc32c(0, span)
        for q in sorted({0, 31, 32, 32 + 8 * length - 1} | set(rng.integers(0, 32 + 8 * length, 8).tolist())):
            if q < 32:
                assert mc.locate_bit(stored, stored ^ (1 << q), length) == q
            else:
                bad = span.copy()
                bad[(q - 32) // 8] ^= 1 << ((q - 32) % 8)
                assert mc.locate_bit(oracle.crc32c(0, bad), stored, length) == q


def test_the_shared_header_passes_its_stand_alone_check(geom_exe):
    r = subprocess.run([geom_exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "repair_geom ok" in r.stdout, r.stdout + r.stderr


def test_the_models_geometry_is_the_headers():
    src = open(os.path.join(ROOT, "memcached_amd", "csrc", "repair_geom.h")).read()
    assert f"kRepairChunk = {rm.CHUNK};" in src
    hdr = open(os.path.join(ROOT, "include", "crc32c_batch.h")).read()
    assert "#define CRC32C_REPAIR_SPAN_MAX 0x0fffffc0u" in hdr and "#define CRC32C_ITEM_REPAIRED 5" in hdr
    assert _lib.CRC32C_REPAIR_SPAN_DEFAULT == rm.SPAN_DEFAULT and _lib.CRC32C_ITEM_REPAIRED == rm.REPAIRED


def test_repair_items_without_a_gpu_is_enodev_and_writes_nothing():
    if _lib.lib.crc32c_gpu_count() > 0:
        pytest.skip("a gfx950 device is visible")
    rng = np.random.default_rng(6)
    buf = _flip(sc.image_nt(rng, 300), 8 * 100)
    before = buf.copy()
    offs = np.zeros(1, np.uint64)
    ok, bit = np.full(1, 77, np.uint8), np.full(1, 77, np.uint64)
    nrep, nbad = ctypes.c_uint64(77), ctypes.c_uint64(77)
    rc = _lib.lib.crc32c_repair_items(buf.ctypes.data, buf.size, 0, offs.ctypes.data, 1, 0, ok.ctypes.data,
                                      bit.ctypes.data, ctypes.byref(nrep), ctypes.byref(nbad), 0, None)
    assert rc == _lib.CRC32C_ENODEV
    assert (buf == before).all() and ok[0] == 77 and bit[0] == 77 and nrep.value == 77 and nbad.value == 77
    with pytest.raises(_lib.Crc32cError) as e:
        mc.repair_items(buf, offs)
    assert e.value.rc == _lib.CRC32C_ENODEV and (buf == before).all()
    # the argument checks come first
    assert _lib.lib.crc32c_repair_items(None, buf.size, 0, offs.ctypes.data, 1, 0, ok.ctypes.data, bit.ctypes.data,
                                        ctypes.byref(nrep), ctypes.byref(nbad), 0, None) == _lib.CRC32C_EINVAL


def test_repair_items_needs_a_writable_buffer_unless_locate_only():
    rng = np.random.default_rng(7)
    img = bytes(sc.image_nt(rng, 300))
    with pytest.raises(TypeError):
        mc.repair_items(img, np.zeros(1, np.uint64))
    try:
        mc.repair_items(img, np.zeros(1, np.uint64), locate_only=True)
    except _lib.Crc32cError as e:
        assert e.rc == _lib.CRC32C_ENODEV and _lib.lib.crc32c_gpu_count() == 0

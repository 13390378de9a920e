"""crc32c_repair_bytes without a GPU: the rule's two statements
(tests/repair_bytes_model.py: every byte XORed by every mask and the CRC
recomputed through the oracle; the byte steps of the syndrome) agree, damage in
two bytes is not located in the pinned cases, the host scalar
crc32c_locate_byte of the built library gives the model's answers and
crc32c_locate_bit's for single bits, the HIP-free arithmetic the kernels share
(memcached_amd/csrc/repair_geom.h) passes its stand-alone check under the
sanitizers -- which derives the span limit 190 231 itself -- and the C ABI
refuses to work without a device."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from memcached_amd import _lib
from memcached_amd import crc32c as mc
from tests import oracle
from tests import repair_bytes_cases as bc
from tests import repair_bytes_model as bm
from tests import repair_model as rm
from tests import salvage_cases as sc

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def _xor(img, p, m):
    out = np.frombuffer(bytes(img), np.uint8).copy()
    out[p] ^= m
    return out


@pytest.fixture(scope="module")
def check_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("repair_bytes") / "repair_bytes_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-I", os.path.join(ROOT, "memcached_amd", "csrc"),
                    os.path.join(HERE, "integration", "repair_bytes_check.cpp"),
                    os.path.join(ROOT, "memcached_amd", "csrc", "crc32c_host.cpp"), "-o", exe], check=True)
    return exe


def test_the_two_statements_agree_on_every_byte_and_mask_of_a_52_byte_image():
    rng = np.random.default_rng(52)
    img = sc.image_nt(rng, 52)
    assert bm.located_brute(img) == bm.located_syndrome(img) == []
    for p in range(28, 52):
        for m in range(1, 256):
            bad = _xor(img, p, m)
            assert bm.located_brute(bad) == bm.located_syndrome(bad) == [(p, m)], (p, m)


def test_the_two_statements_agree_on_every_byte_of_short_images():
    rng = np.random.default_rng(53)
    for nt in (53, 60, 77):
        img = sc.image_nt(rng, nt, cas=nt >= 60)
        for p in range(28, nt):
            m = bc.heavy_mask(rng)
            bad = _xor(img, p, m)
            assert bm.located_brute(bad) == bm.located_syndrome(bad) == [(p, m)], (nt, p, m)


@pytest.mark.parametrize("nt", [4165, bm.SPAN_DEFAULT + 32, bm.SPAN_MAX + 32])
def test_the_two_statements_agree_on_sampled_bytes_of_long_images(nt):
    """The rule as written for one pair: with byte p XORed by m, stored ==
    computed -- at both ends, at the search's chunk edge and at random places."""
    rng = np.random.default_rng(nt)
    img = sc.image_nt(rng, nt, cas=True)
    L = nt - 32
    ps = {28 + bm.byte_of_step(j, L) for j in (0, 3, 4, 5, 255, 256, 257, 4 + L - 1)}
    ps |= set(rng.integers(28, nt, 2 if nt > 100000 else 6).tolist())
    for p in sorted(ps):
        for m in (0x03, 0xff, bc.heavy_mask(rng)) if nt > 100000 else (0x01, 0x80, 0x03, 0xff, 0x5a, bc.heavy_mask(rng)):
            bad = _xor(img, p, m)
            assert bm.located_syndrome(bad) == [(p, m)], (nt, p, m)
            assert rm.syndrome(_xor(bad, p, m))[0] == 0
            other = int(rng.integers(28, nt))
            assert (rm.syndrome(_xor(bad, other, m))[0] == 0) == (other == p)


def test_single_bit_masks_are_the_one_bit_rules_positions():
    rng = np.random.default_rng(54)
    for nt in (52, 77, 300, 4165):
        img = sc.image_nt(rng, nt, cas=nt >= 60)
        for k in sorted(set(rm.boundary_bits(nt)) | set(rng.integers(224, 8 * nt, 16).tolist())):
            bad = _xor(img, k // 8, 1 << (k % 8))
            assert rm.located_syndrome(bad) == [k]
            assert bm.located_syndrome(bad) == [(k // 8, 1 << (k % 8))]


def test_two_damaged_bytes_are_not_located_in_the_pinned_cases():
    buf, offs = bc.two_bytes()  # (asserts it of every image itself)
    ok, byte, mask, nrep, nbad, after = bm.repair(buf, offs)
    assert ok.tolist() == [0] * len(offs) and nrep == 0 and nbad == len(offs)
    assert (byte == bm.NO_BIT).all() and (mask == 0).all() and np.array_equal(after, buf)
    # the one-bit rule refuses them too
    assert rm.repair(buf, offs)[0].tolist() == [0] * len(offs)


def test_verdicts_of_one_image():
    rng = np.random.default_rng(3)
    img = sc.image_nt(rng, 77, cas=True)
    assert bm.repair_one(img, 0) == (1, bm.NO_BIT, 0)
    pad = np.zeros(1 << 12, np.uint8)
    for p in range(28, 77):
        for m in (0x01, 0x02, 0x05, 0xfe, 0xff):
            bad = _xor(img, p, m)
            if bm.length_mask(p, m):  # (judged by its new length: padded so that it can still be sane)
                bad = np.concatenate([bad, pad])
                assert bm.repair_one(bad, 0) == (0, bm.NO_BIT, 0), (p, m)
                continue
            assert bm.repair_one(bad, 0) == bm.repair_one(bad, 0, brute=True) == (bm.REPAIRED, p, m), (p, m)
    # the length bits of a mask: byte 38 bit 1, byte 39 bit 0, every bit of 32..35 and 41
    assert bm.length_mask(38, 0x02) and not bm.length_mask(38, 0x05)
    assert bm.length_mask(39, 0x01) and not bm.length_mask(39, 0xfe)
    assert all(bm.length_mask(p, m) for p in (32, 33, 34, 35, 41) for m in range(1, 256))
    # bytes 0..27 are not covered: intact
    assert bm.repair_one(_xor(img, 12, 0xff), 0) == (1, bm.NO_BIT, 0)
    # no CRLF at the end (and the stored CRC stamped over that): a located pair is not accepted
    raw = np.frombuffer(bytes(sc.raw_image(rng, 300, b"xy")), np.uint8)
    assert bm.repair_one(raw, 0) == (1, bm.NO_BIT, 0)
    assert bm.located_syndrome(_xor(raw, 100, 0x0f)) == [(100, 0x0f)]
    assert bm.repair_one(_xor(raw, 100, 0x0f), 0) == (0, bm.NO_BIT, 0)
    # the CRLF itself: the test is made with the byte corrected
    assert bm.repair_one(_xor(img, 75, 0xff), 0) == (bm.REPAIRED, 75, 0xff)
    assert bm.repair_one(_xor(img, 76, 0x0a), 0) == (bm.REPAIRED, 76, 0x0a)
    # longer than max_span; not sane
    assert bm.repair_one(_xor(img, 50, 3), 0, max_span=44) == (0, bm.NO_BIT, 0)
    assert bm.repair_one(_xor(img, 50, 3), 0, max_span=45) == (bm.REPAIRED, 50, 3)
    assert bm.repair_one(img[:60], 0) == (0, bm.NO_BIT, 0)


def _syndrome_of(p, m, length):
    """S of codeword byte p XORed by m, from the CRCs of real bytes."""
    if p < 4:
        return m << (8 * p)
    span = np.zeros(length, np.uint8)
    span[p - 4] = m
    return oracle.crc32c(0, span) ^ oracle.crc32c(0, np.zeros(length, np.uint8))


def _locate_cases():
    """(crc_computed, crc_stored, len, want): a hit in every stored-CRC byte, in
    the first and last span byte and on both sides of step 256; the refusals."""
    rng = np.random.default_rng(4)
    cases = [(5, 5, 100, None), (0, 0, 0, None), (0x5a000000, 0, bm.SPAN_MAX + 1, None), (0x00010100, 0, 20, None)]
    for length in (0, 1, 251, 252, 253, 4133, bm.SPAN_MAX):
        steps = 4 + length
        for j in sorted({0, 1, 2, 3, 4, steps - 1, 255, 256, 257} & set(range(steps))):
            p = bm.byte_of_step(j, length)
            for m in (0x01, 0x80, 0x03, 0xff, 0x5a):
                e = int(rng.integers(0, 1 << 32))
                cases.append((_syndrome_of(p, m, length) ^ e, e, length, (p, m)))
    return cases


def test_locate_byte_of_the_built_library_equals_the_model(check_exe):
    cases = _locate_cases()
    for c, e, length, want in cases:
        assert bm.locate_byte(c, e, length) == want, (length, want)
    got = [mc.locate_byte(c, e, length) for c, e, length, _ in cases]
    assert got == [w for *_, w in cases]
    assert sum(w is not None for *_, w in cases) > 200
    # a single-bit mask: crc32c_locate_bit's position
    for c, e, length, want in cases:
        if want is not None and want[1] in (0x01, 0x80):
            assert mc.locate_bit(c, e, length) == 8 * want[0] + (0 if want[1] == 1 else 7)
    # one byte over the limit: refused, whatever the syndrome
    assert mc.locate_byte(0x5a000000, 0, bm.SPAN_MAX) == (3, 0x5a)
    assert mc.locate_byte(0x5a000000, 0, bm.SPAN_MAX + 1) is None
    assert _lib.CRC32C_REPAIR_BYTES_SPAN_MAX == bm.SPAN_MAX == 190231
    assert _lib.CRC32C_REPAIR_BYTES_SPAN_DEFAULT == bm.SPAN_DEFAULT
    # the mask pointer is optional, and zeroed when nothing is located
    assert _lib.lib.crc32c_locate_byte(0x5a000000, 0, 10, None) == 3
    m = ctypes.c_uint8(0x77)
    assert _lib.lib.crc32c_locate_byte(5, 5, 10, ctypes.byref(m)) == _lib.CRC32C_NO_BIT and m.value == 0
    # the same source, compiled with the sanitizers
    r = subprocess.run([check_exe, "locate"], input="\n".join(f"{c} {e} {n}" for c, e, n, _ in cases),
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    rows = [tuple(map(int, line.split())) for line in r.stdout.splitlines()]
    assert rows == [(bm.NO_BIT, 0) if w is None else w for *_, w in cases]


def test_the_shared_header_passes_its_stand_alone_check(check_exe):
    """The program recomputes the smallest distance at which two one-byte
    patterns share a syndrome (190 235, for 0xdf) and holds kRepairBytesSpanMax
    + 4 to it."""
    r = subprocess.run([check_exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "repair_bytes ok" in r.stdout, r.stdout + r.stderr


def test_the_models_constants_are_the_headers():
    src = open(os.path.join(ROOT, "memcached_amd", "csrc", "repair_geom.h")).read()
    assert f"kRepairBytesSpanMax = {bm.SPAN_MAX}u;" in src and "kRepairBytesSpanDefault = 0x10000u;" in src
    hdr = open(os.path.join(ROOT, "include", "crc32c_batch.h")).read()
    assert "#define CRC32C_REPAIR_BYTES_SPAN_MAX 190231u" in hdr
    assert "#define CRC32C_REPAIR_BYTES_SPAN_DEFAULT 0x10000u" in hdr
    # the evidence is stated where the guarantee is
    assert "255 (4 + L) / 2^32" in hdr and "32 times" in hdr


def test_repair_bytes_is_public_but_not_in_the_pinned_list():
    assert callable(mc.repair_bytes) and callable(mc.locate_byte)
    assert "repair_bytes" not in mc.__all__ and "locate_byte" not in mc.__all__


def _raw(buf, offs, n, ok, byte, mask, mode=0, max_span=0, out=True):
    opts = _lib.BytesOpts(mode, max_span, None)
    o = _lib.BytesOut(*(None if a is None else a.ctypes.data for a in (ok, byte, mask)), 77, 77)
    rc = _lib.lib.crc32c_repair_bytes(None if buf is None else buf.ctypes.data, 0 if buf is None else buf.size, 0,
                                      None if offs is None else offs.ctypes.data, n, ctypes.byref(opts),
                                      ctypes.byref(o) if out else None)
    return rc, o.nrepaired, o.nbad


def test_repair_bytes_without_a_gpu_is_enodev_and_writes_nothing():
    if _lib.lib.crc32c_gpu_count() > 0:
        pytest.skip("a gfx950 device is visible")
    rng = np.random.default_rng(6)
    buf = _xor(sc.image_nt(rng, 300), 100, 0x5a)
    before = buf.copy()
    offs = np.zeros(1, np.uint64)
    ok, byte, mask = np.full(1, 77, np.uint8), np.full(1, 77, np.uint64), np.full(1, 77, np.uint8)
    assert _raw(buf, offs, 1, ok, byte, mask) == (_lib.CRC32C_ENODEV, 77, 77)
    assert _raw(buf, offs, 0, ok, byte, mask) == (_lib.CRC32C_ENODEV, 77, 77)
    assert (buf == before).all() and ok[0] == 77 and byte[0] == 77 and mask[0] == 77
    # NULL opts: all zero
    o = _lib.BytesOut(ok.ctypes.data, byte.ctypes.data, mask.ctypes.data, 77, 77)
    assert _lib.lib.crc32c_repair_bytes(buf.ctypes.data, buf.size, 0, offs.ctypes.data, 1, None,
                                        ctypes.byref(o)) == _lib.CRC32C_ENODEV
    assert (o.nrepaired, o.nbad) == (77, 77)
    with pytest.raises(_lib.Crc32cError) as e:
        mc.repair_bytes(buf, offs)
    assert e.value.rc == _lib.CRC32C_ENODEV and (buf == before).all()
    # the argument checks come first
    assert _raw(None, offs, 1, ok, byte, mask)[0] == _lib.CRC32C_EINVAL
    assert _raw(buf, None, 1, ok, byte, mask)[0] == _lib.CRC32C_EINVAL
    assert _raw(buf, offs, 1, None, byte, mask)[0] == _lib.CRC32C_EINVAL
    assert _raw(buf, offs, 1, ok, None, mask)[0] == _lib.CRC32C_EINVAL
    assert _raw(buf, offs, 1, ok, byte, None)[0] == _lib.CRC32C_EINVAL
    assert _raw(buf, offs, 1, ok, byte, mask, out=False)[0] == _lib.CRC32C_EINVAL
    assert _raw(buf, offs, 1, ok, byte, mask, max_span=bm.SPAN_MAX + 1) == (_lib.CRC32C_EINVAL, 77, 77)
    assert _raw(buf, offs, 1, ok, byte, mask, max_span=bm.SPAN_MAX)[0] == _lib.CRC32C_ENODEV
    assert (buf == before).all() and ok[0] == 77 and byte[0] == 77 and mask[0] == 77


def test_repair_bytes_needs_a_writable_buffer_unless_locate_only():
    rng = np.random.default_rng(7)
    img = bytes(sc.image_nt(rng, 300))
    with pytest.raises(TypeError):
        mc.repair_bytes(img, np.zeros(1, np.uint64))
    frozen = np.frombuffer(img, np.uint8)
    with pytest.raises(TypeError):
        mc.repair_bytes(frozen, np.zeros(1, np.uint64))
    try:
        mc.repair_bytes(img, np.zeros(1, np.uint64), locate_only=True)
    except _lib.Crc32cError as e:
        assert e.rc == _lib.CRC32C_ENODEV and _lib.lib.crc32c_gpu_count() == 0

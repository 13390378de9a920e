"""crc32c_repair_headers without a GPU: the rule's two statements
(tests/header_model.py: each length bit inverted and the CRC recomputed through
the oracle; the CRC of the span as it stands XOR x^t) agree, the crafted
ambiguous header is what it claims to be, the HIP-free arithmetic the kernels
share (memcached_amd/csrc/header_geom.h) passes its stand-alone check under the
sanitizers, the symbol is declared, exported and prototyped, and the C ABI
refuses to work without a device."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from memcached_amd import _lib
from memcached_amd import crc32c as mc
from tests import header_cases as hc
from tests import header_model as hm
from tests import repair_model as rm
from tests import salvage_cases as sc
from tests.repair_cases import flip

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


@pytest.fixture(scope="module")
def geom_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("header_geom") / "header_geom_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-I", os.path.join(ROOT, "memcached_amd", "csrc"),
                    os.path.join(HERE, "integration", "header_geom_check.cpp"),
                    os.path.join(ROOT, "memcached_amd", "csrc", "crc32c_host.cpp"), "-o", exe], check=True)
    return exe


def test_the_two_statements_agree_on_every_bit_of_short_images():
    rng = np.random.default_rng(52)
    for nt in range(52, 81):
        img = sc.image_nt(rng, nt, cas=nt >= 60 and bool(nt & 1))
        # room behind the image: a variant may be longer than the image
        buf = np.concatenate([np.zeros(7, np.uint8), np.frombuffer(bytes(img), np.uint8),
                              rng.integers(0, 256, 700, dtype=np.uint8)])
        assert hm.repair_one(buf, 7) == hm.repair_one(buf, 7, flip=True) == (1, hm.NO_BIT, nt)
        for k in hm.BITS:
            flip(buf, 7, k)
            assert hm.hits_flip(buf, 7) == hm.hits_xpow(buf, 7) == [(k, nt)], (nt, k)
            assert hm.repair_one(buf, 7) == hm.repair_one(buf, 7, flip=True) == (hm.REPAIRED, k, nt)
            flip(buf, 7, k)


def test_the_identity_for_the_lengths_on_record():
    """For nt in {52, 61, 77, 300, 4165} and all 42 bits: the oracle CRC of the
    damaged span XOR xpow(t_of_k(k, nt)) equals the stored CRC."""
    from tests import oracle
    rng = np.random.default_rng(61)
    for nt in (52, 61, 77, 300, 4165):
        img = np.frombuffer(bytes(sc.image_nt(rng, nt, cas=nt >= 77)), np.uint8).copy()
        stored = int.from_bytes(bytes(img[28:32]), "little")
        for k in hm.BITS:
            flip(img, 0, k)
            assert oracle.crc32c(0, img[32:]) ^ rm.xpow(rm.t_of_k(k, nt)) == stored, (nt, k)
            flip(img, 0, k)


def test_verdicts_of_one_header():
    rng = np.random.default_rng(3)
    buf, offs, names = hc.mixed_damage()
    at = dict(zip(names, offs.tolist()))
    for name in ("data_bit", "two_length_bits", "length_and_data", "nkey0", "no_crlf"):
        assert hm.repair_one(buf, at[name]) == hm.repair_one(buf, at[name], flip=True) == (0, hm.NO_BIT, 0), name
    for name in ("decoy", "one_bit"):
        ok, bit, nt = hm.repair_one(buf, at[name])
        assert (ok, bit) == (hm.REPAIRED, 256 + 3) and nt > 300, name
    # (the decoy's CRLF makes candidates of the wrong variants that end there: nbytes bit 6 and nkey bit 6)
    assert len(hm.candidates(buf, at["decoy"])) > len(hm.candidates(buf, at["one_bit"]))
    assert hm.repair_one(buf, at["intact"])[0] == 1
    # under 48 bytes left, at and past the end: nothing is read
    img = np.frombuffer(bytes(sc.image_nt(rng, 60)), np.uint8).copy()
    for o in (13, 59, 60, 61, 1 << 40):
        assert hm.repair_one(img, o) == (0, hm.NO_BIT, 0)
    assert hm.repair_one(img, 12)[0] == 0 and hm.repair_one(img, 0) == (1, hm.NO_BIT, 60)


def test_the_crafted_header_is_ambiguous():
    buf, o = hc.ambiguous(crafted=False)
    assert hm.hits_flip(buf, o) == hm.hits_xpow(buf, o) == [(256, 77)]
    assert hm.repair_one(buf, o) == (hm.REPAIRED, 256, 77)
    buf, o = hc.ambiguous()
    hits = hm.hits_flip(buf, o)
    assert hits == hm.hits_xpow(buf, o) and [k for k, _ in hits] == [256, 261] and hits[0][1] == 77 < hits[1][1]
    assert hm.repair_one(buf, o) == hm.repair_one(buf, o, flip=True) == (0, hm.NO_BIT, 0)


def test_packed_images_are_all_repaired_below_the_work_bound():
    rng = np.random.default_rng(8)
    buf, offs, bits, nts = hc.packed(rng)
    ok, bit, lens, nrep, nbad, after = hm.repair(buf, offs)
    damaged = [k is not None for k in bits]
    assert sum(damaged) == 32 * 42 == nrep and nbad == 0
    for k, v, b, n, nt in zip(bits, ok.tolist(), bit.tolist(), lens.tolist(), nts):
        assert (v, b, n) == ((1, hm.NO_BIT, nt) if k is None else (hm.REPAIRED, k, nt))
    assert hm.ncandidates(buf, offs) >= nrep
    assert 2 * hm.work(buf, offs) < hm.WORK_MAX * buf.size  # under half the bound
    for o, nt in zip(offs.tolist(), nts):
        assert rm.syndrome(after[o:o + nt])[0] == 0


def test_breaks_lists_the_damaged_header_of_every_header_case():
    cases = sc.small_cases()
    for name in ("hdr_nbytes_b0", "hdr_cas_bit", "hdr_nkey0", "first_image", "config5_small"):
        buf, W, cfl = cases[name]
        todo = hc.breaks(buf, W, cfl)
        assert todo.size >= 1 and (np.diff(todo.astype(np.int64)) > 0).all()
        assert all(min((int(o) // W + 1) * W, buf.size) - int(o) >= 48 for o in todo)
        ok = hm.repair(buf, todo, W, cfl)[0]
        assert (ok == hm.REPAIRED).sum() == (0 if name == "hdr_nkey0" else 2 if name == "config5_small" else 1), name


def test_the_shared_header_passes_its_stand_alone_check(geom_exe):
    r = subprocess.run([geom_exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "header_geom ok" in r.stdout, r.stdout + r.stderr


def test_repair_headers_is_declared_exported_and_prototyped():
    hdr = open(os.path.join(ROOT, "include", "crc32c_batch.h")).read()
    assert "#define CRC32C_HEADER_BITS 42" in hdr and "#define CRC32C_HEADER_WORK_MAX 8" in hdr
    assert re.search(r"\bint crc32c_repair_headers\(void \*base, uint64_t base_bytes, uint64_t region_bytes,", hdr)
    assert "crc32c_repair_headers" in _lib.EXPORTED and "crc32c_repair_headers" in _lib.PROTOTYPES
    f = _lib.lib.crc32c_repair_headers
    assert f.restype == ctypes.c_int and len(f.argtypes) == 12
    assert _lib.CRC32C_HEADER_BITS == hm.HEADER_BITS == len(hm.BITS) and _lib.CRC32C_HEADER_WORK_MAX == hm.WORK_MAX
    src = open(os.path.join(ROOT, "memcached_amd", "csrc", "header_geom.h")).read()
    assert "kHeaderBits = 42;" in src and "kHeaderWorkMax = 8;" in src
    assert callable(mc.repair_headers) and "repair_headers" not in mc.__all__


def test_repair_headers_without_a_gpu_is_enodev_and_writes_nothing():
    if _lib.lib.crc32c_gpu_count() > 0:
        pytest.skip("a gfx950 device is visible")
    rng = np.random.default_rng(6)
    buf = np.frombuffer(bytes(sc.image_nt(rng, 300)), np.uint8).copy()
    flip(buf, 0, 256 + 1)
    before = buf.copy()
    offs = np.zeros(1, np.uint64)
    ok, bit, lens = np.full(1, 77, np.uint8), np.full(1, 77, np.uint64), np.full(1, 77, np.uint32)
    nrep, nbad = ctypes.c_uint64(77), ctypes.c_uint64(77)
    args = [buf.ctypes.data, buf.size, 0, offs.ctypes.data, 1, ok.ctypes.data, bit.ctypes.data, lens.ctypes.data,
            ctypes.byref(nrep), ctypes.byref(nbad), 0, None]
    assert _lib.lib.crc32c_repair_headers(*args) == _lib.CRC32C_ENODEV
    assert (buf == before).all() and ok[0] == 77 and bit[0] == 77 and lens[0] == 77
    assert nrep.value == 77 and nbad.value == 77
    with pytest.raises(_lib.Crc32cError) as e:
        mc.repair_headers(buf, offs)
    assert e.value.rc == _lib.CRC32C_ENODEV and (buf == before).all()
    # the argument checks come first
    for i in (0, 3, 5, 6, 7, 8, 9):
        bad = list(args)
        bad[i] = None
        assert _lib.lib.crc32c_repair_headers(*bad) == _lib.CRC32C_EINVAL, i
    args[4] = (2**32 - 2) // 43 + 1
    assert _lib.lib.crc32c_repair_headers(*args) == _lib.CRC32C_EINVAL


def test_repair_headers_needs_a_writable_buffer_unless_locate_only():
    rng = np.random.default_rng(7)
    img = bytes(sc.image_nt(rng, 300))
    with pytest.raises(TypeError):
        mc.repair_headers(img, np.zeros(1, np.uint64))
    try:
        mc.repair_headers(img, np.zeros(1, np.uint64), locate_only=True)
    except _lib.Crc32cError as e:
        assert e.rc == _lib.CRC32C_ENODEV and _lib.lib.crc32c_gpu_count() == 0

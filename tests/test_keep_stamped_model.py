"""CRC32C_KEEP_STAMPED and crc32c_stamp_pages without a GPU: the CPU model the
GPU tests compare against (tests/keep_stamped_model.py) on hand-built cases,
the header constants, the Python wrappers' argument checks, and the new kernel
instantiations in the built code object."""
import os
import re
import subprocess

import numpy as np
import pytest

from memcached_amd import _lib, layout
from memcached_amd import crc32c as mc

from . import keep_stamped_model as model
from . import oracle
from .test_kernel_resources import LLVM, _code_object

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _item(i, nvalue, seed=0):
    rng = np.random.default_rng(1000 * seed + i)
    return layout.make_item(b"km%05d" % i, rng.integers(0, 256, nvalue, dtype=np.uint8).tobytes(), cas=i + 1)


def _exptime(buf, o):
    return int.from_bytes(bytes(buf[int(o) + 28:int(o) + 32]), "little")


def _zero_crc_item():
    """An image whose spill CRC is 0: the last four value bytes are solved so
    that the register after the span is ~0 (crc32c is affine in them)."""
    img = layout.make_item(b"zerocrc", bytes(8), cas=7)
    at = len(img) - 6  # the four value bytes before the trailing CRLF
    buf = np.frombuffer(bytes(img), np.uint8).copy()
    base = oracle.item_crc(buf, 0)
    # columns of the linear map (bit j of the four bytes -> CRC bits)
    cols = []
    for j in range(32):
        b = buf.copy()
        b[at + j // 8] ^= 1 << (j % 8)
        cols.append(oracle.item_crc(b, 0) ^ base)
    # solve cols . x = base over GF(2)
    rows = [(cols[j], 1 << j) for j in range(32)]
    x, target = 0, base
    basis = {}
    for v, tag in rows:
        while v:
            h = v.bit_length() - 1
            if h not in basis:
                basis[h] = (v, tag)
                break
            bv, bt = basis[h]
            v ^= bv
            tag ^= bt
    while target:
        h = target.bit_length() - 1
        bv, bt = basis[h]  # (the map is a bijection on 32 bits)
        target ^= bv
        x ^= bt
    for j in range(32):
        if x >> j & 1:
            buf[at + j // 8] ^= 1 << (j % 8)
    assert oracle.item_crc(buf, 0) == 0
    return bytearray(buf.tobytes())


def test_model_on_hand_built_cases():
    wbuf = 64 << 10
    items = [_item(i, 100 + 37 * i) for i in range(6)] + [_zero_crc_item()]
    buf, offs = layout.pack_wbufs(items, wbuf)
    crcs = [oracle.item_crc(buf, o) for o in offs]
    assert all(c != 0 for c in crcs[:6]) and crcs[6] == 0
    FRESH, GOOD, BAD, MAL, BADLEN, FRESH2, ZERO = range(7)
    layout.store_crcs(buf, offs[[GOOD, BAD, MAL, BADLEN]], [crcs[GOOD], crcs[BAD], crcs[MAL], crcs[BADLEN]])
    buf[int(offs[BAD]) + 60] ^= 0x20          # carried, a data bit flipped
    buf[int(offs[MAL]) + 41] = 0              # nkey 0: malformed
    buf[int(offs[BADLEN]) + 32 + 2] ^= 0x08   # nbytes += 512 KiB: leaves its wbuf, malformed
    out, ok, nbad = model.expected_stamp(buf, offs, wbuf, keep=True)
    assert ok.tolist() == [1, 2, 0, 0, 0, 1, 1] and nbad == 3
    assert _exptime(out, offs[FRESH]) == crcs[FRESH] and _exptime(out, offs[FRESH2]) == crcs[FRESH2]
    # a stored CRC of 0 with a CRC of 0: taken for fresh, re-stamped with the same 0
    assert _exptime(out, offs[ZERO]) == 0
    changed = np.flatnonzero(out != buf)
    want = np.concatenate([np.arange(28, 32) + int(offs[k]) for k in (FRESH, FRESH2)])
    assert set(changed.tolist()) <= set(want.tolist())  # only fresh images' exptime bytes
    # carried images keep their bytes, the damaged one included
    for k in (GOOD, BAD, MAL, BADLEN):
        assert _exptime(out, offs[k]) == crcs[k]
    # the verify that follows: bad exactly the damaged carried image and the malformed ones
    assert model.expected_verify(out, offs, wbuf).tolist() == [1, 1, 0, 0, 0, 1, 1]
    # without the flag every sane image is stamped: the damage is laundered
    out2, ok2, nbad2 = model.expected_stamp(buf, offs, wbuf, keep=False)
    assert ok2.tolist() == [1, 1, 1, 0, 0, 1, 1] and nbad2 == 2
    assert model.expected_verify(out2, offs, wbuf).tolist() == [1, 1, 1, 0, 0, 1, 1]
    # a corrupt carried image whose stored CRC is 0 is laundered too (the documented 2^-32 caveat)
    z = buf.copy()
    z[int(offs[ZERO]) + 50] ^= 1
    out3, ok3, _ = model.expected_stamp(z, offs, wbuf, keep=True)
    assert ok3[ZERO] == 1 and _exptime(out3, offs[ZERO]) == oracle.item_crc(z, offs[ZERO]) != 0


def test_model_walk_stops_where_the_reference_walk_stops():
    wbuf = 16 << 10
    items = [_item(i, 900, seed=2) for i in range(40)]
    buf, offs = layout.pack_wbufs(items, wbuf)
    np.testing.assert_array_equal(model.host_walk(buf, wbuf), offs)
    per = int(np.searchsorted(offs, wbuf))
    b = buf.copy()
    b[int(offs[3]) + 41] = 0  # ends the first wbuf's walk
    np.testing.assert_array_equal(model.host_walk(b, wbuf), np.concatenate([offs[:3], offs[per:]]))
    # a walk bounded by the bytes used never looks behind them
    used = int(offs[5])
    g = buf[:used + 300].copy()
    g[used:] = 0xa5
    np.testing.assert_array_equal(model.host_walk(g[:used], wbuf), offs[:5])


def test_header_constants_match_the_binding():
    hdr = open(os.path.join(ROOT, "include", "crc32c_batch.h")).read()
    defs = dict(re.findall(r"#define (CRC32C_\w+) \(?(-?(?:0x)?[0-9a-fA-F]+)u?\)?", hdr))
    assert int(defs["CRC32C_KEEP_STAMPED"], 0) == _lib.CRC32C_KEEP_STAMPED == 0x10
    assert int(defs["CRC32C_ITEM_STAMPED"], 0) == _lib.CRC32C_ITEM_STAMPED == model.STAMPED == 1
    assert int(defs["CRC32C_ITEM_KEPT"], 0) == _lib.CRC32C_ITEM_KEPT == model.KEPT == 2
    assert "crc32c_stamp_pages" in _lib.EXPORTED and re.search(r"\bint crc32c_stamp_pages\(void \*base,", hdr)
    assert "stamp_pages" in mc.__all__ and "stamp_items" in mc.__all__
    assert _lib.lib.crc32c_stamp_pages.argtypes == _lib.lib.crc32c_verify_pages.argtypes


def test_wrappers_reject_bad_arguments_without_a_device():
    buf = np.zeros(4096, np.uint8)
    offs = np.zeros(1, np.uint64)
    ro = buf.copy()
    ro.flags.writeable = False
    for bad in (bytes(4096), ro, np.zeros(1024, np.uint32), np.zeros((64, 64), np.uint8)[:, ::2]):
        with pytest.raises(TypeError):
            mc.stamp_pages(bad, 4096, keep_stamped=True)
        with pytest.raises(TypeError):
            mc.stamp_items(bad, offs, keep_stamped=True)
    for wbuf in (0, -4096, 4096.0, None):
        with pytest.raises(ValueError):
            mc.stamp_pages(buf, wbuf)
    # the C entry point checks its pointers before it looks for a device
    n, nb = _lib.ctypes.c_uint64(0), _lib.ctypes.c_uint64(0)
    f = _lib.lib.crc32c_stamp_pages
    ref = _lib.ctypes.byref
    assert f(None, 4096, 4096, None, None, 0, ref(n), ref(nb), _lib.CRC32C_KEEP_STAMPED, None) == _lib.CRC32C_EINVAL
    assert f(buf.ctypes.data, 4096, 0, None, None, 0, ref(n), ref(nb), 0, None) == _lib.CRC32C_EINVAL
    assert f(buf.ctypes.data, 4096, 4096, None, None, 0, None, ref(nb), 0, None) == _lib.CRC32C_EINVAL
    assert f(buf.ctypes.data, 4096, 4096, None, None, 0, ref(n), None, 0, None) == _lib.CRC32C_EINVAL
    assert f(buf.ctypes.data, 4096, 4096, None, None, 8, ref(n), ref(nb), 0, None) == _lib.CRC32C_EINVAL  # cap, no arrays


def _kernel_notes(co):
    notes = subprocess.run([os.path.join(LLVM, "llvm-readobj"), "--notes", str(co)], check=True,
                           capture_output=True, text=True).stdout
    out = {}
    for blk in notes.split("  - .agpr_count")[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        out[name] = {k: int(re.search(rf"\.{k}:\s+(\d+)", blk).group(1))
                     for k in ("private_segment_fixed_size", "vgpr_count", "sgpr_count")}
    return out


def test_keep_stamped_kernels_in_the_code_object(tmp_path):
    """Every route of a stamp has its MODE 3 instantiation (the Itanium
    mangling of k<3> / k<3, true> is k ILi3E / ILi3ELb1E), and K5's costs no
    more private segment (scratch) than the plain stamp's in the same object."""
    ks = _kernel_notes(_code_object(tmp_path))

    def find(kernel, targs):
        hits = [n for n in ks if re.search(rf"\d{kernel}I{targs}E", n)]
        assert len(hits) == 1, (kernel, targs, hits)
        return ks[hits[0]]

    for kernel, targs in (("k_small", "Li3"), ("k_count", "Li3"), ("k_census", "Li3"), ("k_final", "Li3ELb1"),
                          ("k_lines", "Li3ELb1")):
        find(kernel, targs)
    plain, keep = find("k_lines", "Li2ELb1"), find("k_lines", "Li3ELb1")
    assert keep["private_segment_fixed_size"] <= plain["private_segment_fixed_size"], (plain, keep)

"""crc32c_copy_items without a GPU: the CPU model the GPU tests compare with
(tests/copy_items_model.py) against a plain per-image memcpy plus the verify
model's verdicts, the ENODEV contract of the entry point, and the kernel's
presence in the built gfx950 code object."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from memcached_amd import _lib, layout

from . import copy_items_model as model
from . import keep_stamped_model as ks
from . import oracle

LLVM = "/opt/rocm/lib/llvm/bin"
WBUF = 64 * 1024


def _case():
    """60 images with values of 0..5000 B in 64 KiB wbufs, every one carrying
    its CRC; a few damaged or malformed; destinations packed back to back from
    the headers as found, with a 7-byte gap in front of each."""
    rng = np.random.default_rng(2024)
    items = [layout.make_item(b"cp%04d" % i, rng.integers(0, 256, int(rng.integers(0, 5000)), dtype=np.uint8).tobytes(),
                              cas=i + 1 if i % 4 else None) for i in range(60)]
    src, offs = layout.pack_wbufs(items, WBUF)
    layout.store_crcs(src, offs, np.array([oracle.item_crc(src, o) for o in offs], np.uint32))
    for i in (3, 17, 40):  # a data bit
        src[int(offs[i]) + 48 + 5] ^= 0x04
    src[int(offs[8]) + 40] ^= 0x01   # slabs_clsid: inside the span, the header stays sane
    src[int(offs[21]) + 41] = 0      # nkey = 0: malformed
    src[int(offs[33]) + 34] ^= 0x10  # nbytes += 1 MiB: leaves its wbuf
    offs = np.concatenate([offs, np.array([src.size - 20], np.uint64)])  # a header cut by the buffer's end
    doffs, at = [], 0
    for o in offs.tolist():
        at += 7
        doffs.append(at)
        if ks.header_sane(src, o, WBUF):
            at += layout.ntotal_of(src, o)
    return src, offs, np.array(doffs, np.uint64), at


def test_model_is_memcpy_of_the_sane_images_plus_verify_verdicts():
    src, offs, doffs, used = _case()
    init = np.full(used + 64, 0xa5, np.uint8)
    dst, ok, nbad, erange = model.expected_copy(src, offs, WBUF, init, doffs)
    want = init.copy()
    verdict = ks.expected_verify(src, offs, WBUF)
    sane = np.array([ks.header_sane(src, o, WBUF) for o in offs])
    for so, do, s in zip(offs.tolist(), doffs.tolist(), sane):
        if s:
            nt = layout.ntotal_of(src, so)
            want[do:do + nt] = np.frombuffer(bytes(src[so:so + nt]), np.uint8)  # the memcpy of storage.c:1004-1006
    np.testing.assert_array_equal(dst, want)
    np.testing.assert_array_equal(ok, np.where(~sane, 0, np.where(verdict == 1, 1, 3)))
    assert not erange and nbad == 3 + 1 + 3
    assert sorted(np.flatnonzero(ok == 0).tolist()) == [21, 33, 60]
    assert sorted(np.flatnonzero(ok == 3).tolist()) == [3, 8, 17, 40]
    assert (dst[used:] == 0xa5).all() and (init == 0xa5).all()  # nothing behind the last image; the input is not modified
    # a destination one byte too short for the last sane image: that image is
    # dropped and reported, every other one is copied as before
    last = max(i for i in range(60) if sane[i])
    nt = layout.ntotal_of(src, int(offs[last]))
    short = np.full(int(doffs[last]) + nt - 1, 0xa5, np.uint8)
    dst2, ok2, nbad2, erange2 = model.expected_copy(src, offs, WBUF, short, doffs)
    assert erange2 and ok2[last] == 0 and nbad2 == nbad + 1
    np.testing.assert_array_equal(np.delete(ok2, last), np.delete(ok, last))
    np.testing.assert_array_equal(dst2[:int(doffs[last])], want[:int(doffs[last])])
    assert (dst2[int(doffs[last]):] == 0xa5).all()


def test_copy_items_without_a_gpu_is_enodev_and_writes_nothing():
    """CPU leg only: skipped where a gfx950 device is visible."""
    if _lib.lib.crc32c_gpu_count() > 0:
        pytest.skip("a gfx950 device is visible")
    src, offs, doffs, used = _case()
    dst = np.full(used + 64, 0xa5, np.uint8)
    ok = np.full(offs.size, 9, np.uint8)
    nbad = ctypes.c_uint64(77)
    rc = _lib.lib.crc32c_copy_items(src.ctypes.data, src.size, WBUF, offs.ctypes.data, dst.ctypes.data, dst.size,
                                    doffs.ctypes.data, offs.size, ok.ctypes.data, ctypes.byref(nbad), 0, None)
    assert rc == _lib.CRC32C_ENODEV
    assert (dst == 0xa5).all() and (ok == 9).all() and nbad.value == 77
    # the argument checks come first
    assert _lib.lib.crc32c_copy_items(None, src.size, WBUF, offs.ctypes.data, dst.ctypes.data, dst.size,
                                      doffs.ctypes.data, offs.size, ok.ctypes.data, ctypes.byref(nbad), 0,
                                      None) == _lib.CRC32C_EINVAL
    assert _lib.lib.crc32c_copy_items(src.ctypes.data, src.size, WBUF, offs.ctypes.data, src.ctypes.data + 100, 1000,
                                      doffs.ctypes.data, offs.size, ok.ctypes.data, ctypes.byref(nbad), 0,
                                      None) == _lib.CRC32C_EINVAL  # overlapping ranges


# the approach of tests/test_kernel_resources.py: the gfx950 code object out of
# the library's fat binary, and the kernel names in its metadata
def _code_object(tmp_path):
    lib = _lib.LIB_PATH
    if not os.path.exists(lib):
        pytest.skip("libmcrc32c.so not built")
    bundler = os.path.join(LLVM, "clang-offload-bundler")
    if not (shutil.which("objcopy") and os.path.exists(bundler)):
        pytest.skip("objcopy / clang-offload-bundler not available")
    fat = tmp_path / "fatbin.bin"
    co = tmp_path / "gfx950.co"
    subprocess.run(["objcopy", "-O", "binary", "--only-section=.hip_fatbin", lib, str(fat)], check=True)
    subprocess.run([bundler, "--unbundle", "--type=o", f"--input={fat}",
                    "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--output={co}"], check=True)
    return co


def test_k_copy_is_in_the_code_object(tmp_path):
    notes = subprocess.run([os.path.join(LLVM, "llvm-readobj"), "--notes", str(_code_object(tmp_path))], check=True,
                           capture_output=True, text=True).stdout
    names = re.findall(r"\.name:\s+(\S+)", notes)
    hits = [n for n in names if re.search(r"\d+k_copyE", n)]
    assert len(hits) == 1, names
    assert "mcrc_dev" in hits[0]

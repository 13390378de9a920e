"""crc32c_batch_ptrs, crc32c_ptrs_submit and crc32c_chains_ptrs without a GPU:
the argument refusals, which come before the device is looked for, the
CRC32C_ENODEV contract where none is visible, and the cases of
tests/ptr_cases.py against the cases they re-express."""
import ctypes
import os
import re

import numpy as np
import pytest

from memcached_amd import _lib
from memcached_amd import crc32c as mc

from . import chain_cases as cc
from . import ptr_cases as pc
from . import routes_cases as rc
from . import stride_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENT = 0x5A5A5A5A
lib = _lib.lib


def _batch(n=2, ptrs=True, out=True, cin=False):
    buf = np.arange(64, dtype=np.uint8)
    p = np.array([buf.ctypes.data, buf.ctypes.data + 7], np.uint64)
    lens = np.array([10, 20], np.uint32)
    o = np.full(2, SENT, np.uint32)
    c = np.zeros(2, np.uint32)
    b = _lib.PtrBatch(p.ctypes.data if ptrs else None, lens.ctypes.data, 0, c.ctypes.data if cin else None,
                      o.ctypes.data if out else None, n)
    b.keep = buf, p, lens, c
    return b, o


def test_null_arguments_are_refused_before_anything_else():
    b, o = _batch()
    job = ctypes.c_void_p()
    first = np.array([0, 2], np.uint64)
    cout = np.full(1, SENT, np.uint32)
    assert lib.crc32c_batch_ptrs(None, None) == _lib.CRC32C_EINVAL
    assert lib.crc32c_ptrs_submit(None, None, ctypes.byref(job)) == _lib.CRC32C_EINVAL
    assert lib.crc32c_ptrs_submit(ctypes.byref(b), None, None) == _lib.CRC32C_EINVAL
    for kw in (dict(ptrs=False), dict(out=False)):
        bad, o2 = _batch(**kw)
        assert lib.crc32c_batch_ptrs(ctypes.byref(bad), None) == _lib.CRC32C_EINVAL
        assert lib.crc32c_ptrs_submit(ctypes.byref(bad), None, ctypes.byref(job)) == _lib.CRC32C_EINVAL
        assert (o2 == SENT).all()
    # chains: NULL iovs, chain_first or out, and a crc_in
    assert lib.crc32c_chains_ptrs(None, first.ctypes.data, 1, cout.ctypes.data, None) == _lib.CRC32C_EINVAL
    assert lib.crc32c_chains_ptrs(ctypes.byref(b), None, 1, cout.ctypes.data, None) == _lib.CRC32C_EINVAL
    assert lib.crc32c_chains_ptrs(ctypes.byref(b), first.ctypes.data, 1, None, None) == _lib.CRC32C_EINVAL
    seeded, _ = _batch(cin=True)
    assert lib.crc32c_chains_ptrs(ctypes.byref(seeded), first.ctypes.data, 1, cout.ctypes.data, None) == \
        _lib.CRC32C_EINVAL
    # no chains: nothing to do, device or not
    assert lib.crc32c_chains_ptrs(ctypes.byref(b), first.ctypes.data, 0, None, None) == _lib.CRC32C_OK
    assert (o == SENT).all() and (cout == SENT).all() and not job.value


def test_without_a_gpu_every_call_is_enodev_and_writes_nothing():
    if lib.crc32c_gpu_count() > 0:
        pytest.skip("a gfx950 device is visible")
    b, o = _batch()
    job = ctypes.c_void_p()
    first = np.array([0, 2], np.uint64)
    cout = np.full(1, SENT, np.uint32)
    for mode in (0, _lib.CRC32C_DEVICE, _lib.CRC32C_DEVICE | _lib.CRC32C_ASYNC):
        opts = _lib.PtrOpts(mode, None)
        assert lib.crc32c_batch_ptrs(ctypes.byref(b), ctypes.byref(opts)) == _lib.CRC32C_ENODEV
        assert lib.crc32c_ptrs_submit(ctypes.byref(b), ctypes.byref(opts), ctypes.byref(job)) == _lib.CRC32C_ENODEV
        assert lib.crc32c_chains_ptrs(ctypes.byref(b), first.ctypes.data, 1, cout.ctypes.data,
                                      ctypes.byref(opts)) == _lib.CRC32C_ENODEV
    empty, _ = _batch(n=0)
    assert lib.crc32c_batch_ptrs(ctypes.byref(empty), None) == _lib.CRC32C_ENODEV  # (as crc32c_batch answers)
    assert (o == SENT).all() and (cout == SENT).all() and not job.value
    for call in (lambda: mc.batch_ptrs([b"abc", np.arange(5, dtype=np.uint8)]),
                 lambda: mc.chains_ptrs([b"abc", b"de"], [0, 2])):
        with pytest.raises(_lib.Crc32cError) as e:
            call()
        assert e.value.rc == _lib.CRC32C_ENODEV


def test_python_face_is_public_but_not_in_all():
    assert callable(mc.batch_ptrs) and callable(mc.chains_ptrs)
    assert "batch_ptrs" not in mc.__all__ and "chains_ptrs" not in mc.__all__
    with pytest.raises(ValueError):
        mc.batch_ptrs([b"abc"], crc_in=np.zeros(0, np.uint32))  # (one span, no crc_in entry: refused before the call)


def _code(text):
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def test_header_declares_the_three_calls_with_their_structs():
    hdr = open(os.path.join(ROOT, "include", "crc32c_batch.h")).read()
    for name in ("crc32c_batch_ptrs", "crc32c_ptrs_submit", "crc32c_chains_ptrs"):
        assert re.search(rf"\bint {name}\(const crc32c_ptr_batch \*", hdr), name
        assert name in _lib.EXPORTED and name in _lib.PROTOTYPES
    fields = re.search(r"typedef struct crc32c_ptr_batch \{(.*?)\} crc32c_ptr_batch;", hdr, re.S).group(1)
    assert re.findall(r"(\w+);", _code(fields)) == [f for f, _ in _lib.PtrBatch._fields_]
    fields = re.search(r"typedef struct crc32c_ptr_opts \{(.*?)\} crc32c_ptr_opts;", hdr, re.S).group(1)
    assert re.findall(r"(\w+);", _code(fields)) == [f for f, _ in _lib.PtrOpts._fields_]
    assert ctypes.sizeof(_lib.PtrBatch) == 48 and ctypes.sizeof(_lib.PtrOpts) == 16


def test_cases_re_express_every_span_and_chain_case():
    """ptr_cases covers short_spans(), every stride case and every small chain
    case, with the spans and expectations of the originals."""
    spans = pc.span_cases()
    buf, offs, lens, want = rc.short_spans()
    short = [c for c in spans if c.source == "short_spans"]
    assert {c.small_max for c in short} == {None, 0} and any(c.n == 8192 for c in short)
    whole = next(c for c in short if c.n == offs.size)
    assert np.array_equal(whole.offs, offs) and np.array_equal(whole.expected(), want)
    strides = {c.source.name: c for c in spans if isinstance(c.source, sc.Case)}
    assert set(strides) == {c.name for c in sc.cases()}
    for c in list(sc.cases())[::7]:
        p = strides[c.name]
        assert np.array_equal(p.offs, c.offsets()) and np.array_equal(p.span_lens(), c.span_lens())
        assert p.small_max == c.small_max and p.bufs[0] is c.buf
        assert np.array_equal(p.expected(), c.expected(False))
    chains = pc.chain_cases()
    assert [c.source.name for c in chains] == [c.name for c in cc.small_cases()]
    for p in chains:
        if p.n <= 100:
            assert np.array_equal(p.expected_chains(), cc.expected(p.source)), p.name


def test_scattered_case_has_the_shapes_it_is_there_for():
    c = pc.scattered()
    assert c.n == 48 and len(c.bufs) == 3 and set(c.where.tolist()) == {0, 1, 2}
    assert set(pc.SCATTER_LENS) == {0, 1, 3, 15, 16, 17, 4095, 4096, 4097, 4133} <= set(c.lens.tolist())
    assert set((c.offs % 16).tolist()) == set(range(16))
    assert (c.where[46], c.offs[46], c.lens[46]) == (c.where[5], c.offs[5], c.lens[5])
    assert c.where[47] == c.where[7] and c.offs[47] == c.offs[7] + 1 and c.lens[7] == c.lens[47] == 4096
    ends = c.offs.astype(np.int64) + c.lens
    assert all(ends[c.where == k].max() <= c.bufs[k].size for k in range(3)) and ends[c.where == 2].max() == c.bufs[2].size
    assert c.expected()[46] == c.expected()[5] and c.expected(True)[46] != c.expected(True)[5]
    counts = np.diff(c.first.astype(np.int64))
    assert (counts == 0).sum() == 3 and counts.sum() == 48

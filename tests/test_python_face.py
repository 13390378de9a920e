"""What memcached_amd/crc32c.py hands to the library, pinned without a GPU.

crc32c.py binds the library as the module global ``lib``; every test here puts
a recording stub in its place.  The stub notes each call's arguments as plain
integers (a ``crc32c_spans`` as a dict of its fields, a ``byref`` out-parameter
as the string "out"), writes scripted values through the out-parameters and
returns a scripted status.  So these tests see exactly what a host (numpy)
call marshals -- pointers, byte counts, n, cap, the flag word, the stream --
and what the wrapper makes of the library's answer: result dtypes and lengths,
the second call of the capacity retry, the attributes that travel with an
error.  The device (torch) side is covered by tests/test_gpu_python_face.py.
"""
import ctypes

import numpy as np
import pytest

from memcached_amd import _lib
from memcached_amd import crc32c as mc

SIZE = 16 << 10
W = 4096
F64, KEEP = _lib.CRC32C_CFLAGS64, _lib.CRC32C_KEEP_STAMPED


class Stub:
    """Stands in for the ctypes library object.  ``replies[name]`` is a list
    of (status, value per out-parameter ...) used up call by call (the last
    one repeats); a function without replies returns 0 and writes nothing."""

    def __init__(self, **replies):
        self.replies = {k: list(v) for k, v in replies.items()}
        self.calls = []
        self.peek = None  # called with the raw arguments while the call is in flight

    def __getattr__(self, name):
        if not name.startswith("crc32c"):
            raise AttributeError(name)

        def call(*args):
            if self.peek:
                self.peek(*args)
            seen, outs = [], []
            for a in args:
                obj = getattr(a, "_obj", None)  # what ctypes.byref() wraps
                if isinstance(obj, _lib.Spans):
                    seen.append({f: getattr(obj, f) for f, _ in _lib.Spans._fields_})
                elif obj is not None:
                    outs.append(obj)
                    seen.append("out")
                else:
                    seen.append(a)
            self.calls.append((name, seen))
            replies = self.replies.get(name)
            if not replies:
                return 0
            status, *values = replies.pop(0) if len(replies) > 1 else replies[0]
            for obj, v in zip(outs, values):
                obj.value = v
            return status

        return call


@pytest.fixture
def stub(monkeypatch):
    def install(**replies):
        s = Stub(**replies)
        monkeypatch.setattr(mc, "lib", s)
        return s
    return install


@pytest.fixture
def buf():
    return np.arange(SIZE, dtype=np.uint32).astype(np.uint8)


def p(a):
    return a.ctypes.data


OFFS = np.array([0, 100, 4096, 9000], np.uint64)
LENS = np.array([64, 3000, 1, 0], np.uint32)
CIN = np.array([0, 1, 0xFFFFFFFF, 7], np.uint32)
N = 4


def _only(s, name):
    assert [c[0] for c in s.calls] == [name]
    return s.calls[0][1]


# ---- what reaches the library -------------------------------------------------

def test_scalars(stub):
    s = stub(crc32c_sw=[(0x1234,)], crc32c_gpu_count=[(3,)])
    assert mc.crc32c(0, b"123456789") == 0xE3069283  # through the data symbol, not through `lib`
    assert mc.crc32c(mc.crc32c(0, b"1234"), bytearray(b"56789")) == 0xE3069283
    assert s.calls == []
    data = np.frombuffer(b"123456789", np.uint8)
    assert mc.crc32c_sw(-1, data) == 0x1234
    assert _only(s, "crc32c_sw") == [0xFFFFFFFF, p(data), 9]
    assert mc.gpu_count() == 3
    assert mc.Crc32cError is _lib.Crc32cError


def test_batch_offsets_and_lens(stub, buf):
    s = stub()
    out = mc.batch(buf, offsets=OFFS, lens=LENS, crc_in=CIN, stream=1234, asynchronous=True)
    sp, flags, stream = _only(s, "crc32c_batch")
    assert sp == dict(base=p(buf), base_bytes=SIZE, offsets=p(OFFS), stride=0, lens=p(LENS), len=0, crc_in=p(CIN),
                      out=p(out), n=N)
    assert flags == 0 and stream is None  # neither ASYNC nor a stream on the host
    assert out.dtype == np.uint32 and out.shape == (N,)


def test_batch_stride_and_length(stub, buf):
    s = stub()
    mine = np.zeros(6, np.int32)
    out = mc.batch(buf, stride=4096, lens=LENS, out=mine)  # n from lens
    sp, flags, stream = _only(s, "crc32c_batch")
    assert out is mine
    assert sp == dict(base=p(buf), base_bytes=SIZE, offsets=None, stride=4096, lens=p(LENS), len=0, crc_in=None,
                      out=p(mine), n=N)
    s.calls.clear()
    out = mc.batch(buf.tobytes(), offsets=OFFS, length=100)  # bytes in, n from offsets
    sp, flags, stream = _only(s, "crc32c_batch")
    assert (sp["base_bytes"], sp["offsets"], sp["lens"], sp["len"], sp["n"]) == (SIZE, p(OFFS), None, 100, N)
    assert (flags, stream) == (0, None) and out.dtype == np.uint32 and out.shape == (N,)


def test_descriptors_are_converted_to_the_abi_widths(stub, buf):
    s = stub()
    seen = {}

    def peek(spans, flags, stream):
        sp = spans._obj
        seen["offsets"] = list((ctypes.c_uint64 * sp.n).from_address(sp.offsets))
        seen["lens"] = list((ctypes.c_uint32 * sp.n).from_address(sp.lens))
        seen["crc_in"] = list((ctypes.c_uint32 * sp.n).from_address(sp.crc_in))

    s.peek = peek
    mc.batch(buf.view(np.uint32), offsets=[0, 8, 4096], lens=np.array([1, 2, 3], np.int64),
             crc_in=np.array([5, 0, 6, 0, 7, 0], np.uint32)[::2])
    assert seen == {"offsets": [0, 8, 4096], "lens": [1, 2, 3], "crc_in": [5, 6, 7]}
    assert s.calls[0][1][0]["base_bytes"] == SIZE  # bytes, whatever the element type


def test_batch_multi(stub, buf):
    s = stub()
    out = mc.batch_multi(buf, offsets=OFFS, lens=LENS, crc_in=CIN, ngpus=2)
    sp, ngpus = _only(s, "crc32c_batch_multi")
    assert sp == dict(base=p(buf), base_bytes=SIZE, offsets=p(OFFS), stride=0, lens=p(LENS), len=0, crc_in=p(CIN),
                      out=p(out), n=N)
    assert ngpus == 2 and out.dtype == np.uint32 and out.shape == (N,)
    s.calls.clear()
    out = mc.batch_multi(buf, stride=512, lens=LENS)
    sp, ngpus = _only(s, "crc32c_batch_multi")
    assert (sp["offsets"], sp["stride"], sp["lens"], sp["n"], ngpus) == (None, 512, p(LENS), N, 0)


@pytest.mark.parametrize("kw, flags", [({}, 0), ({"cflags64": True}, F64)])
def test_verify_items(stub, buf, kw, flags):
    s = stub(crc32c_verify_items=[(0, 2)])
    ok, nbad = mc.verify_items(buf, OFFS, region_bytes=W, stream=99, **kw)
    assert _only(s, "crc32c_verify_items") == [p(buf), SIZE, W, p(OFFS), N, p(ok), "out", flags, None]
    assert ok.dtype == np.uint8 and ok.shape == (N,) and nbad == 2


@pytest.mark.parametrize("kw, flags", [({}, 0), ({"cflags64": True}, F64), ({"keep_stamped": True}, KEEP),
                                       ({"cflags64": True, "keep_stamped": True}, F64 | KEEP)])
def test_stamp_items(stub, buf, kw, flags):
    s = stub(crc32c_stamp_items=[(0, 1)])
    ok, nbad = mc.stamp_items(buf, OFFS, **kw)
    assert _only(s, "crc32c_stamp_items") == [p(buf), SIZE, 0, p(OFFS), N, p(ok), "out", flags, None]
    assert ok.dtype == np.uint8 and ok.shape == (N,) and nbad == 1


@pytest.mark.parametrize("kw, flags", [({}, 0), ({"cflags64": True}, F64)])
def test_copy_items(stub, buf, kw, flags):
    s = stub(crc32c_copy_items=[(0, 3)])
    dst = np.zeros(8192, np.uint8)
    doffs = np.array([0, 64, 3000, 5000], np.uint64)
    ok, nbad = mc.copy_items(buf, OFFS, dst, doffs, region_bytes=W, stream=5, **kw)
    assert _only(s, "crc32c_copy_items") == [p(buf), SIZE, W, p(OFFS), p(dst), 8192, p(doffs), N, p(ok), "out",
                                             flags, None]
    assert ok.dtype == np.uint8 and ok.shape == (N,) and nbad == 3


def _bound(size, wbuf):
    """An image is >= 50 bytes and each wbuf's last counted image may run past its end."""
    return size // 50 + -(-size // wbuf)


@pytest.mark.parametrize("kw, flags", [({}, 0), ({"cflags64": True}, F64), ({"keep_stamped": True}, KEEP)])
def test_stamp_pages(stub, buf, kw, flags):
    s = stub(crc32c_stamp_pages=[(0, 5, 1)])
    offs, ok, nbad = mc.stamp_pages(buf, W, stream=7, **kw)
    cap = _bound(SIZE, W)
    assert cap == 327 + 4
    args = _only(s, "crc32c_stamp_pages")  # one call on the host: no count query
    assert args == [p(buf), SIZE, W, p(offs.base), p(ok.base), cap, "out", "out", flags, None]
    assert offs.dtype == np.uint64 and ok.dtype == np.uint8 and offs.shape == ok.shape == (5,) and nbad == 1
    assert offs.base.shape == ok.base.shape == (cap,)


def test_stamp_pages_trusts_its_bound(stub, buf):
    stub(crc32c_stamp_pages=[(0, _bound(SIZE, W) + 1, 0)])
    with pytest.raises(AssertionError, match="above the proven bound"):
        mc.stamp_pages(buf, W)


@pytest.mark.parametrize("wbuf", [W, 5000, SIZE, 1 << 20])
def test_verify_pages_host_bound(stub, buf, wbuf):
    s = stub(crc32c_verify_pages=[(0, 3, 2)])
    offs, ok, nbad = mc.verify_pages(buf, wbuf, stream=7, cflags64=True)
    cap = _bound(SIZE, wbuf)
    args = _only(s, "crc32c_verify_pages")
    assert args == [p(buf), SIZE, wbuf, p(offs.base), p(ok.base), cap, "out", "out", F64, None]
    assert offs.dtype == np.uint64 and ok.dtype == np.uint8 and offs.shape == ok.shape == (3,) and nbad == 2


def test_verify_pages_host_never_retries(stub, buf):
    """On the host the capacity is the proven bound: a larger count is an
    assertion, not a second call."""
    cap = _bound(SIZE, W)
    s = stub(crc32c_verify_pages=[(0, cap, 0)])
    offs, ok, nbad = mc.verify_pages(buf, W)
    assert offs.shape == (cap,) and len(s.calls) == 1
    s = stub(crc32c_verify_pages=[(0, cap + 1, 0)])
    with pytest.raises(AssertionError, match="above the proven bound"):
        mc.verify_pages(buf, W)
    assert len(s.calls) == 1


def test_salvage_pages_one_call(stub, buf):
    s = stub(crc32c_salvage_pages=[(0, 2, 900, 11)])
    walked = np.array([0, 500, 4096], np.uint64)
    walked_ok = np.array([1, 0, 1], np.uint8)
    offs, info = mc.salvage_pages(buf, W, walked, walked_ok, stream=3, cflags64=True)
    cap = SIZE // (100 * 1024) + 64
    assert _only(s, "crc32c_salvage_pages") == [p(buf), SIZE, W, p(walked), p(walked_ok), 3, p(offs.base), cap,
                                                "out", "out", "out", F64, None]
    assert offs.dtype == np.uint64 and offs.shape == (2,) and info == {"scanned": 900, "ncand": 11}


@pytest.mark.parametrize("lists", [(None, None), (np.empty(0, np.uint64), np.empty(0, np.uint8))])
def test_salvage_pages_retries_with_the_exact_count(stub, buf, lists):
    """More images than the first guess holds: the second call's capacity is
    the count the first one reported, and its results are the ones returned."""
    s = stub(crc32c_salvage_pages=[(0, 70, 100, 80), (0, 70, 101, 81)])
    offs, info = mc.salvage_pages(buf, W, *lists)
    assert [c[0] for c in s.calls] == ["crc32c_salvage_pages"] * 2
    first, second = s.calls[0][1], s.calls[1][1]
    assert first[:6] == [p(buf), SIZE, W, None, None, 0] and first[7] == 64 and first[11:] == [0, None]
    assert second[:6] == first[:6] and second[7] == 70 and second[11:] == [0, None]
    assert second[6] == p(offs.base) and offs.base.shape == (70,)
    assert offs.dtype == np.uint64 and offs.shape == (70,) and info == {"scanned": 101, "ncand": 81}


def test_batch_chains(stub, buf):
    s = stub()
    offs = np.array([0, 10, 20, 4096, 5000, 6000], np.uint64)
    lens = np.array([10, 10, 5, 100, 0, 9], np.uint32)
    first = np.array([0, 3, 6], np.uint64)
    out = mc.batch_chains(buf, offs, lens, first, stream=8)
    sp, cf, nchains, outp, flags, stream = _only(s, "crc32c_batch_chains")
    iov_out = sp.pop("out")
    assert sp == dict(base=p(buf), base_bytes=SIZE, offsets=p(offs), stride=0, lens=p(lens), len=0, crc_in=None, n=6)
    assert iov_out and iov_out != p(out)  # the iovs' own CRCs go to a scratch array
    assert (cf, nchains, outp, flags, stream) == (p(first), 2, p(out), 0, None)
    assert out.dtype == np.uint32 and out.shape == (2,)


def test_small_calls(stub):
    s = stub(crc32c_queue_stats=[(0, 1, 2, 3, 4)], crc32c_set_small_max=[(48,)],
             crc32c_set_k1_tail_min=[(2 ** 64 - 1,)])
    lens = np.array([5, 6, 7], np.uint32)
    seen = []

    def fill(lens_p, length, n, parts, cuts_p):
        seen.append((lens_p, length, n, parts))
        (ctypes.c_uint64 * (parts + 1)).from_address(cuts_p)[:] = [0, 2, 3]

    s.peek = fill
    cuts = mc.shard_cuts(lens, 2)
    assert seen == [(p(lens), 0, 3, 2)]
    assert cuts.dtype == np.int64 and cuts.tolist() == [0, 2, 3]
    s.peek = None
    assert mc.queue_stats() == (1, 2, 3, 4)
    assert s.calls[-1] == ("crc32c_queue_stats", ["out"] * 4)
    assert mc.set_small_max(16) == 48 and s.calls[-1] == ("crc32c_set_small_max", [16])
    assert mc.set_k1_tail_min(9) == 2 ** 64 - 1 and s.calls[-1] == ("crc32c_set_k1_tail_min", [9])


def test_everything_public_is_pinned_here():
    assert sorted(mc.__all__) == sorted([
        "crc32c", "crc32c_sw", "gpu_count", "Crc32cError", "batch", "batch_multi", "verify_items", "stamp_items",
        "copy_items", "stamp_pages", "verify_pages", "salvage_pages", "batch_chains", "shard_cuts", "queue_stats",
        "set_small_max", "set_k1_tail_min"])


# ---- a status other than OK ---------------------------------------------------

def test_a_status_becomes_a_named_error(stub, buf):
    stub(crc32c_batch=[(_lib.CRC32C_ENODEV,)], crc32c_verify_pages=[(_lib.CRC32C_EWALK, 0, 0)],
         crc32c_copy_items=[(_lib.CRC32C_EINVAL, 0)], crc32c_salvage_pages=[(_lib.CRC32C_ERANGE, 0, 0, 0)])
    for rc, what, call in (
            (_lib.CRC32C_ENODEV, "crc32c_batch", lambda: mc.batch(buf, offsets=OFFS, lens=LENS)),
            (_lib.CRC32C_EWALK, "crc32c_verify_pages", lambda: mc.verify_pages(buf, W)),
            (_lib.CRC32C_EINVAL, "crc32c_copy_items", lambda: mc.copy_items(buf, OFFS, np.zeros(64, np.uint8), OFFS)),
            (_lib.CRC32C_ERANGE, "crc32c_salvage_pages", lambda: mc.salvage_pages(buf, W))):
        with pytest.raises(mc.Crc32cError, match=what) as e:
            call()
        assert e.value.rc == rc and not hasattr(e.value, "ok") and not hasattr(e.value, "scanned")


def test_copy_items_erange_carries_the_verdicts(stub, buf):
    stub(crc32c_copy_items=[(_lib.CRC32C_ERANGE, 2)])
    with pytest.raises(mc.Crc32cError, match="crc32c_copy_items") as e:
        mc.copy_items(buf, OFFS, np.zeros(64, np.uint8), OFFS)
    assert e.value.rc == _lib.CRC32C_ERANGE and e.value.nbad == 2
    assert e.value.ok.dtype == np.uint8 and e.value.ok.shape == (N,)


def test_salvage_pages_ework_carries_the_counts(stub, buf):
    s = stub(crc32c_salvage_pages=[(_lib.CRC32C_EWORK, 0, 16000, 4000)])
    with pytest.raises(mc.Crc32cError, match="crc32c_salvage_pages") as e:
        mc.salvage_pages(buf, W)
    assert (e.value.rc, e.value.scanned, e.value.ncand) == (_lib.CRC32C_EWORK, 16000, 4000)
    assert len(s.calls) == 1


# ---- rejected before the library is called -----------------------------------

def _rejected(s, exc, match, call):
    with pytest.raises(exc, match=match):
        call()
    assert s.calls == []


def test_batch_rejections(stub, buf):
    s = stub()
    _rejected(s, ValueError, "need offsets or lens", lambda: mc.batch(buf, stride=64, length=64))
    _rejected(s, ValueError, "lens: 4 elements for 5 spans", lambda: mc.batch(buf, offsets=np.arange(5), lens=LENS))
    _rejected(s, ValueError, "crc_in: 4 elements for 5 spans",
              lambda: mc.batch(buf, offsets=np.arange(5), length=8, crc_in=CIN))
    _rejected(s, ValueError, "out: 3 elements for 4 spans",
              lambda: mc.batch(buf, offsets=OFFS, lens=LENS, out=np.zeros(3, np.uint32)))
    for bad in (np.zeros(4, np.uint64), np.zeros(4, np.float32), np.zeros(8, np.uint32)[::2]):
        _rejected(s, TypeError, "out: need a contiguous uint32 array",
                  lambda: mc.batch(buf, offsets=OFFS, lens=LENS, out=bad))


def _not_in_place(buf):
    ro = buf.copy()
    ro.setflags(write=False)
    return [ro, buf.view(np.uint32), buf[::2], buf.tobytes(), bytearray(buf.tobytes())]


def test_in_place_calls_need_a_writable_uint8_array(stub, buf):
    s = stub()
    need = "needs a writable contiguous uint8 numpy array"
    for bad in _not_in_place(buf):
        _rejected(s, TypeError, "stamp_items " + need, lambda: mc.stamp_items(bad, OFFS))
        _rejected(s, TypeError, "stamp_pages " + need, lambda: mc.stamp_pages(bad, W))
        _rejected(s, TypeError, "copy_items " + need + " as dst", lambda: mc.copy_items(buf, OFFS, bad, OFFS))


@pytest.mark.parametrize("wbuf", [0, -1, 1.5, None])
def test_wbuf_bytes_is_a_positive_integer(stub, buf, wbuf):
    s = stub()
    _rejected(s, ValueError, "wbuf_bytes: need a positive integer", lambda: mc.stamp_pages(buf, wbuf))
    _rejected(s, ValueError, "wbuf_bytes: need a positive integer", lambda: mc.salvage_pages(buf, wbuf))


def test_wbuf_bytes_may_be_any_integer_type(stub, buf):
    s = stub()
    mc.stamp_pages(buf, np.int64(W))
    mc.salvage_pages(buf, np.uint32(W))
    assert [c[1][2] for c in s.calls] == [W, W]


def test_salvage_pages_rejections(stub, buf):
    s = stub()
    walked = np.array([0, 500, 4096], np.uint64)
    _rejected(s, ValueError, "walked and walked_ok go together", lambda: mc.salvage_pages(buf, W, walked))
    _rejected(s, ValueError, "walked and walked_ok go together",
              lambda: mc.salvage_pages(buf, W, walked_ok=np.ones(3, np.uint8)))
    _rejected(s, ValueError, "walked_ok: 2 ", lambda: mc.salvage_pages(buf, W, walked, np.ones(2, np.uint8)))


def test_copy_items_rejections(stub, buf):
    s = stub()
    dst = np.zeros(8192, np.uint8)
    for doffs in (OFFS[:3], np.arange(5, dtype=np.uint64)):
        _rejected(s, ValueError, "dst_offsets: %d elements for 4 " % doffs.size,
                  lambda: mc.copy_items(buf, OFFS, dst, doffs))

    class NotNumpy:  # a host src goes with a numpy dst and nothing else
        is_cuda = False

    _rejected(s, TypeError, "copy_items needs a writable contiguous uint8 numpy array as dst",
              lambda: mc.copy_items(buf, OFFS, NotNumpy(), OFFS))
    _rejected(s, TypeError, "as dst", lambda: mc.copy_items(buf, OFFS, list(range(64)), OFFS))


# ---- invalid calls that used to fail by accident, or not at all ----------------
# (each is now refused as the sibling wrapper named refuses it)

@pytest.mark.parametrize("wbuf", [0, -1, 1.5, None])
def test_verify_pages_bad_wbuf_bytes(stub, buf, wbuf):
    """As stamp_pages and salvage_pages.  (Was a ZeroDivisionError for 0, numpy's
    ValueError for -1 and its TypeError for 1.5 and None, from the capacity
    arithmetic.)"""
    s = stub()
    _rejected(s, ValueError, "wbuf_bytes: need a positive integer", lambda: mc.verify_pages(buf, wbuf))


def test_batch_multi_without_offsets_and_lens(stub, buf):
    """As batch.  (Was the TypeError of len(None).)"""
    s = stub()
    _rejected(s, ValueError, "need offsets or lens", lambda: mc.batch_multi(buf, stride=64, length=64))


def test_batch_multi_short_arrays(stub, buf):
    """As batch.  (Both reached the library, which reads n elements of each.)"""
    s = stub()
    _rejected(s, ValueError, "lens: 4 elements for 5 spans",
              lambda: mc.batch_multi(buf, offsets=np.arange(5, dtype=np.uint64), lens=LENS))
    _rejected(s, ValueError, "crc_in: 2 elements for 4 spans",
              lambda: mc.batch_multi(buf, offsets=OFFS, lens=LENS, crc_in=CIN[:2]))


def test_batch_chains_short_lens(stub, buf):
    """As batch_chains on the device.  (Reached the library.)  Longer arrays
    than the iov count stay valid on both sides."""
    s = stub()
    first = np.array([0, 3, 6], np.uint64)
    _rejected(s, ValueError, "lens: 4 elements for 6 spans",
              lambda: mc.batch_chains(buf, np.arange(6, dtype=np.uint64), LENS, first))
    mc.batch_chains(buf, OFFS, np.zeros(9, np.uint32), np.array([0, 4], np.uint64))
    assert _only(s, "crc32c_batch_chains")[0]["n"] == N

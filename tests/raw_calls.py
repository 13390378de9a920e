"""The page-recovery entry points as the GPU tests call them: one raw ctypes
caller per entry point, one checker per result shape, and what they share --
the sentinels, Side (where a run's copies live), page-locked buffers and the
small-batch limit as context managers.  Nothing here needs a GPU or the
library to be imported: torch and memcached_amd._lib are loaded on first use,
so the tables of ops (tests/*interleave_cases.py) and their CPU tests import
through it.

A caller makes fresh copies of its inputs through the Side, hands the library
output arrays with sentinel words behind their room and count words that hold
the sentinel, and returns a dict: "rc", every output array whole as unsigned
numpy, every count word, and "after", the buffer's bytes after the call.  It
asserts nothing; the checkers and the test files do."""
import contextlib
import ctypes
import functools

import numpy as np

OK, EINVAL, ERANGE, EWORK = 0, -3, -5, -7
DEVICE, ASYNC, CFLAGS64, KEEP_STAMPED, LOCATE_ONLY, SCRUB_GAPS = 0x1, 0x2, 0x8, 0x10, 0x20, 0x40
MODE_BITS = {"asynchronous": ASYNC, "cflags64": CFLAGS64, "keep_stamped": KEEP_STAMPED, "locate_only": LOCATE_ONLY,
             "gaps": SCRUB_GAPS}
SENT64 = 0x5A5A5A5A5A5A5A5A
SENT = {1: SENT64 & 0xFF, 4: SENT64 & 0xFFFFFFFF, 8: SENT64}
EXTRA = 4  # sentinel words behind an output array's room

LISTED = (("offsets", np.uint64), ("lens", np.uint32), ("kind", np.uint8))
SALVAGE_COUNTS = ("nfound", "scanned", "ncand")
RECOVER_COUNTS = ("nitems", "nbad", "nsalvaged", "scanned", "ncand")
TRIAGE_COUNTS = ("nitems", "nbad", "nsalvaged", "nsuspect", "scanned", "ncand")
COUNTS = {"crc32c_recover_pages": RECOVER_COUNTS, "crc32c_triage_pages": TRIAGE_COUNTS}
SCRUB_LISTS = LISTED + (("flip_offsets", np.uint64), ("flip_bits", np.uint64), ("flip_by", np.uint8))
SCRUB_WORDS = TRIAGE_COUNTS + ("nflips", "headers_repaired", "items_repaired", "rounds", "complete")


def _lib():
    from memcached_amd import _lib as m  # (loads libmcrc32c.so: only a call gets here)
    return m


@functools.lru_cache(maxsize=None)
def need_gpu():
    """torch, once a GPU and the library's view of it are there (asserted once per process)."""
    import torch
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    assert _lib().lib.crc32c_gpu_count() >= 1, "libmcrc32c.so sees no gfx950 device"
    return torch


@contextlib.contextmanager
def pinned(nbytes):
    """nbytes of crc32c_host_alloc memory as a numpy view, freed on exit."""
    lib = _lib().lib
    p = lib.crc32c_host_alloc(max(nbytes, 1))
    assert p, "crc32c_host_alloc failed"
    try:
        yield np.ctypeslib.as_array((ctypes.c_uint8 * nbytes).from_address(p))
    finally:
        lib.crc32c_host_free(p)


@contextlib.contextmanager
def small_max(value):
    """crc32c_set_small_max for a block: None leaves it alone (k_small up to
    the default), 0 sends every batch to the planned path."""
    if value is None:
        yield
        return
    lib = _lib().lib
    prev = lib.crc32c_set_small_max(value)
    try:
        yield
    finally:
        lib.crc32c_set_small_max(prev)


def _ro(a):
    a.setflags(write=False)
    return a


def ended(a, dtype=None):
    """An expected output array: a, and the sentinel behind its end."""
    a = np.asarray(a, dtype)
    return _ro(np.concatenate((a, np.array([SENT[a.itemsize]], a.dtype))))


def _capped(values, cap, dtype):
    """An expected output array of cap entries that received min(cap, len) values."""
    a = np.full(cap, SENT[np.dtype(dtype).itemsize], dtype)
    k = min(cap, len(values))
    a[:k] = values[:k]
    return ended(a)


def ptr(x):
    if x is None:
        return None
    return x.data_ptr() if hasattr(x, "data_ptr") else x.ctypes.data


class Side:
    """Where one run's copies live -- "device" (torch tensors made and read on
    `stream`, or on the default stream), "host" (pageable numpy arrays) or
    "pinned" (the data buffers in crc32c_host_alloc memory; freed when the
    with block ends) -- and the flags and the stream handle that go with it.
    where may be a bool: True is "device", False "host".  pad: the sentinel
    words behind the room of the arrays out() makes."""

    def __init__(self, torch=None, stream=None, where="device", pad=EXTRA):
        where = {True: "device", False: "host"}.get(where, where)
        self.dev = where == "device"
        self.torch = need_gpu() if self.dev and torch is None else torch
        self.stream, self.where, self.pad = stream, where, pad
        self.handle = None
        self._adopted, self._stack = None, contextlib.ExitStack()
        if self.dev:
            self.handle = ctypes.c_void_p((self.torch.cuda.default_stream() if stream is None else stream).cuda_stream)

    def __enter__(self):
        if self.dev and self.stream is not None:
            self._stack.enter_context(self.torch.cuda.stream(self.stream))
        return self

    def __exit__(self, *exc):
        return self._stack.__exit__(*exc)

    def flags(self, cflags64=False, **mode_bits):
        """The call's flags word: CRC32C_DEVICE for a device side, and the named bits that are set."""
        on = [MODE_BITS[k] for k, v in dict(mode_bits, cflags64=cflags64).items() if v]
        return (DEVICE if self.dev else 0) | sum(on)

    def _tensor(self, a):
        signed = {"uint64": np.int64, "uint32": np.int32}.get(a.dtype.name)
        return self.torch.from_numpy(np.array(a.view(signed) if signed else a)).cuda()

    def adopt(self, view):
        """The data buffer is one the caller placed already (a device view off
        the grid, a page-locked view): data() returns it, not a copy."""
        self._adopted = view
        return self

    def data(self, a):
        """A fresh, writable copy of a data buffer (or the adopted one)."""
        if self._adopted is not None:
            return self._adopted
        if self.dev:
            return self._tensor(a)
        if self.where == "pinned":
            arr = self._stack.enter_context(pinned(a.size))
            arr[:] = a
            return arr
        return a.copy()

    def desc(self, a):
        """A fresh copy of a descriptor array (None stays None)."""
        if a is None:
            return None
        return self._tensor(a) if self.dev else a.copy()

    def out(self, n, dtype, pad=None):
        """An output array of n entries and pad sentinel words, all holding the sentinel."""
        dtype, n = np.dtype(dtype), n + (self.pad if pad is None else pad)
        if self.dev:
            t = {1: self.torch.uint8, 4: self.torch.int32, 8: self.torch.int64}[dtype.itemsize]
            return self.torch.full((n,), SENT[dtype.itemsize], dtype=t, device="cuda")
        return np.full(n, SENT[dtype.itemsize], dtype)

    def host(self, x, dtype):
        """What an array of this run holds now, as numpy (the run's stream is
        waited for)."""
        if x is None:
            return None
        if self.dev:
            return x.cpu().numpy().view(dtype)
        return np.array(x).view(dtype)


# -- the raw callers -------------------------------------------------------------
# (side: a Side, or where a fresh one lives; cfl: the client flags' bytes, 8 sets CRC32C_CFLAGS64)

def _side(side):
    return side if isinstance(side, Side) else Side(where=side)


def _words(names, null=()):
    """name -> a count word holding the sentinel, and the pointers to pass (NULL for the names in null)."""
    words = {k: ctypes.c_uint64(SENT64) for k in names}
    return words, [None if k in null else ctypes.byref(w) for k, w in words.items()]


def _outs(side, spec, null_arrays, null=()):
    """The output arrays of spec, (name, dtype, room) each, and the pointers
    to pass: NULL for the names in null and, with null_arrays, for an array
    that has no room."""
    arrays = {name: side.out(room, dtype) for name, dtype, room in spec}
    ptrs = [None if name in null or (null_arrays and room == 0) else ptr(arrays[name]) for name, _, room in spec]
    return arrays, ptrs


def _result(side, rc, page, arrays, spec, words, **more):
    got = {"rc": rc}
    got.update((name, side.host(arrays[name], dtype)) for name, dtype, _ in spec)
    got.update((k, int(w.value) if hasattr(w, "value") else int(w)) for k, w in words.items())
    got.update(more, after=side.host(page, np.uint8))
    return got


def salvage_pages(side, buf, wbuf, walked=None, walked_ok=None, *, cap, cfl=4, null_arrays=False):
    """crc32c_salvage_pages; also "walked" and "walked_ok", the caller's lists after the call (or None)."""
    side = _side(side)
    page = side.data(buf)
    dw, dk = side.desc(walked), side.desc(walked_ok)
    spec = (("offsets", np.uint64, cap),)
    arrays, ptrs = _outs(side, spec, null_arrays)
    words, refs = _words(SALVAGE_COUNTS)
    n = 0 if walked is None else walked.size
    rc = _lib().lib.crc32c_salvage_pages(ptr(page), buf.size, wbuf, ptr(dw), ptr(dk), n, *ptrs, cap, *refs,
                                         side.flags(cfl == 8), side.handle)
    return _result(side, rc, page, arrays, spec, words, walked=side.host(dw, np.uint64),
                   walked_ok=side.host(dk, np.uint8))


def listed_pages(entry, side, buf, wbuf, *, cap, cfl=4, null_arrays=False):
    """crc32c_recover_pages or crc32c_triage_pages: the list's three arrays and COUNTS[entry]."""
    side = _side(side)
    page = side.data(buf)
    spec = tuple((name, dtype, cap) for name, dtype in LISTED)
    arrays, ptrs = _outs(side, spec, null_arrays)
    words, refs = _words(COUNTS[entry])
    rc = getattr(_lib().lib, entry)(ptr(page), buf.size, wbuf, *ptrs, cap, *refs, side.flags(cfl == 8), side.handle)
    return _result(side, rc, page, arrays, spec, words)


def scrub_pages(side, buf, wbuf, *, cap, flip_cap, cfl=4, max_span=0, max_rounds=0, locate_only=False,
                gaps=False, null_arrays=False):
    """crc32c_scrub_pages; also "rooms" (name -> cap or flip_cap) and "ms", crc32c_last_kernel_ms() behind it."""
    m, side = _lib(), _side(side)
    page = side.data(buf)
    spec = tuple((name, dtype, cap if k < 3 else flip_cap) for k, (name, dtype) in enumerate(SCRUB_LISTS))
    arrays, ptrs = _outs(side, spec, null_arrays)
    opts = m.ScrubOpts(side.flags(cfl == 8, locate_only=locate_only, gaps=gaps), max_span, max_rounds, side.handle)
    out = m.ScrubOut(*ptrs[:3], cap, *ptrs[3:], flip_cap, *([SENT64] * 9), SENT[4], SENT[4])
    rc = m.lib.crc32c_scrub_pages(ptr(page), buf.size, wbuf, ctypes.byref(opts), ctypes.byref(out))
    return _result(side, rc, page, arrays, spec, {w: getattr(out, w) for w in SCRUB_WORDS},
                   rooms={name: room for name, _, room in spec}, ms=m.lib.crc32c_last_kernel_ms())


def _list_call(side, buf, offsets, n, outs, null):
    """What the three repair calls share: the copies (returned too: the call
    gets bare addresses, so they must outlive it), n (the list's length unless
    given) and the arrays."""
    side = _side(side)
    page, offs = side.data(buf), side.desc(offsets)
    spec = tuple((name, dtype, offsets.size) for name, dtype in outs)
    arrays, ptrs = _outs(side, spec, False, null)
    args = [None if "buf" in null else ptr(page), buf.size, None if "offsets" in null else ptr(offs),
            offsets.size if n is None else n]
    return side, (page, offs), spec, arrays, ptrs, args


def repair_items(side, buf, offsets, *, n=None, region=0, max_span=0, cfl=4, locate_only=False, null=()):
    """crc32c_repair_items.  null: the pointer arguments to pass as NULL, by name."""
    side, keep, spec, arrays, ptrs, (base, nbytes, offs, n) = _list_call(side, buf, offsets, n,
                                                                   (("ok", np.uint8), ("bit", np.uint64)), null)
    words, refs = _words(("nrepaired", "nbad"), null)
    rc = _lib().lib.crc32c_repair_items(base, nbytes, region, offs, n, max_span, *ptrs, *refs,
                                        side.flags(cfl == 8, locate_only=locate_only), side.handle)
    return _result(side, rc, keep[0], arrays, spec, words)


def repair_headers(side, buf, offsets, *, n=None, region=0, cfl=4, locate_only=False, null=()):
    """crc32c_repair_headers.  null: the pointer arguments to pass as NULL, by name."""
    side, keep, spec, arrays, ptrs, (base, nbytes, offs, n) = _list_call(
        side, buf, offsets, n, (("ok", np.uint8), ("bit", np.uint64), ("lens", np.uint32)), null)
    words, refs = _words(("nrepaired", "nbad"), null)
    rc = _lib().lib.crc32c_repair_headers(base, nbytes, region, offs, n, *ptrs, *refs,
                                          side.flags(cfl == 8, locate_only=locate_only), side.handle)
    return _result(side, rc, keep[0], arrays, spec, words)


def repair_bytes(side, buf, offsets, *, n=None, region=0, max_span=0, cfl=4, locate_only=False,
                 asynchronous=False, null=()):
    """crc32c_repair_bytes.  null: the pointer arguments to pass as NULL, by name."""
    m = _lib()
    side, keep, spec, arrays, ptrs, (base, nbytes, offs, n) = _list_call(
        side, buf, offsets, n, (("ok", np.uint8), ("byte", np.uint64), ("mask", np.uint8)), null)
    opts = m.BytesOpts(side.flags(cfl == 8, locate_only=locate_only, asynchronous=asynchronous), max_span, side.handle)
    out = m.BytesOut(*ptrs, SENT64, SENT64)
    rc = m.lib.crc32c_repair_bytes(base, nbytes, region, offs, n, ctypes.byref(opts), ctypes.byref(out))
    return _result(side, rc, keep[0], arrays, spec, {"nrepaired": out.nrepaired, "nbad": out.nbad})


# -- the checkers ----------------------------------------------------------------

def expect_unchanged(got, buf):
    """The call left the buffer as it was."""
    assert np.array_equal(got["after"], buf), "base was written"


def expect_listed(got, cap, model, names, lens=True, arrays=("offsets", "lens", "kind"), tag=""):
    """One call's results against an expected answer (a model's dict), cut at
    cap: rc, the counts in names, the first min(cap, n) entries of each array
    and the sentinel in every word behind them.  lens=False: the expected
    answer has no lengths (their sentinels are still checked)."""
    assert got["rc"] == model["rc"], tag
    assert {k: got[k] for k in names} == {k: model[k] for k in names}, tag
    k = min(cap, len(model[arrays[0]]))
    for name in arrays:
        a = got[name]
        assert a.size > cap, (tag, name)
        if lens or name != "lens":
            assert a[:k].tolist() == list(model[name][:k]), (tag, name)
        assert (a[k:] == SENT[a.itemsize]).all(), (tag, name, f"written behind its first {k}")


def expect_scrub(got, model, after=None):
    """A scrub_pages result against the model's, exactly; after: the bytes expected (default: the model's)."""
    assert got["rc"] == model["rc"]
    assert {w: got[w] for w in SCRUB_WORDS} == {w: model[w] for w in SCRUB_WORDS}
    for i, (name, _) in enumerate(SCRUB_LISTS):
        total = model["nitems"] if i < 3 else model["nflips"]
        room, a = got["rooms"][name], got[name]
        k = min(room, total)
        assert a.size > room, name
        assert a[:k].tolist() == list(model[name][:k]), name
        assert (a[k:] == SENT[a.itemsize]).all(), f"{name}: written behind its first {k}"
    assert np.array_equal(got["after"], model["after"] if after is None else after)

"""ctypes binding of libmcrc32c.so (include/crc32c.h + include/crc32c_batch.h).

The library is the product; this module only marshals arguments.  There is no
Python or CPU fallback for the batch entry points: if the library is missing,
importing this module raises, and a batch call without a gfx950 device raises
Crc32cError(CRC32C_ENODEV).
"""
from __future__ import annotations

import ctypes
import os

PKG = os.path.dirname(os.path.abspath(__file__))
# MCRC_LIB selects another build of the same library (A/B of two builds in one run)
LIB_PATH = os.environ.get("MCRC_LIB") or os.path.join(PKG, "libmcrc32c.so")

CRC32C_OK = 0
CRC32C_ENODEV = -1
CRC32C_EHIP = -2
CRC32C_EINVAL = -3
CRC32C_ENOMEM = -4
CRC32C_ERANGE = -5
CRC32C_EWALK = -6
CRC32C_EWORK = -7

CRC32C_DEVICE = 0x1
CRC32C_ASYNC = 0x2
CRC32C_CFLAGS64 = 0x8
CRC32C_KEEP_STAMPED = 0x10
CRC32C_LOCATE_ONLY = 0x20  # repair calls: report, write nothing into the buffer
CRC32C_ITEM_STAMPED = 1  # ok[] values of the stamp calls
CRC32C_ITEM_KEPT = 2
CRC32C_ITEM_COPIED = 1  # ok[] values of crc32c_copy_items
CRC32C_ITEM_DAMAGED = 3
CRC32C_ITEM_SALVAGED = 4  # kind[] of crc32c_recover_pages: found by the salvage (0 / 1: the walk's verdicts)
CRC32C_ITEM_REPAIRED = 5  # ok[] of crc32c_repair_items: one bit located (and flipped back)
CRC32C_ITEM_SUSPECT = 6  # kind[] of crc32c_triage_pages: an unreached candidate whose stored CRC does not match
CRC32C_NO_BIT = 2**64 - 1  # bit[] of crc32c_repair_items / crc32c_locate_bit: no position
CRC32C_REPAIR_SPAN_DEFAULT = 0x200000  # crc32c_repair_items' max_span when 0 is passed
CRC32C_REPAIR_SPAN_MAX = 0x0FFFFFC0  # the longest span whose located position is unique
CRC32C_REPAIR_BYTES_SPAN_MAX = 190231  # crc32c_repair_bytes: the longest span whose located byte is unique
CRC32C_REPAIR_BYTES_SPAN_DEFAULT = 0x10000  # its max_span when 0 is passed
CRC32C_HEADER_BITS = 42  # crc32c_repair_headers: the header bits that decide ITEM_ntotal, one variant each
CRC32C_HEADER_WORK_MAX = 8  # its work bound: the candidate variants' spans per byte of the buffer
CRC32C_SCRUB_ROUNDS_DEFAULT = 64  # crc32c_scrub_pages' max_rounds when 0 is passed
CRC32C_SCRUB_BY_HEADER = 1  # its flip_by[]: made by the crc32c_repair_headers stage
CRC32C_SCRUB_BY_ITEM = 2  # ... by the crc32c_repair_items stage
CRC32C_SCRUB_BY_BYTE = 3  # ... by the crc32c_repair_bytes stage (CRC32C_SCRUB_BYTES)
CRC32C_SCRUB_GAPS = 0x40  # crc32c_scrub_opts.mode: list the ends of the proven unreached images too
CRC32C_SCRUB_BYTES = 0x80  # crc32c_scrub_opts.mode: crc32c_repair_bytes over the item list when the item stage repaired nothing
CRC32C_MAX_SPAN = 0x7FFF0000  # longest span (include/crc32c_batch.h)
CRC32C_SALVAGE_WORK_MAX = 64  # crc32c_salvage_pages' work bound: candidates' spans per scanned byte

# every symbol include/*.h declares (checked by tests/test_abi.py)
EXPORTED = (
    "crc32c", "crc32c_init", "crc32c_sw", "crc32c_sw_little", "crc32c_sw_big",
    "crc32c_gpu_count", "crc32c_batch", "crc32c_batch_multi", "crc32c_verify_items", "crc32c_stamp_items",
    "crc32c_verify_pages", "crc32c_batch_chains", "crc32c_host_alloc", "crc32c_host_free",
    "crc32c_batch_submit", "crc32c_batch_wait", "crc32c_strerror", "crc32c_last_kernel_ms",
    "crc32c_shard_cuts", "crc32c_queue_stats", "crc32c_host_register", "crc32c_host_unregister",
    "crc32c_set_small_max", "crc32c_stamp_pages", "crc32c_copy_items", "crc32c_salvage_pages",
    "crc32c_set_k1_tail_min", "crc32c_recover_pages", "crc32c_repair_items", "crc32c_locate_bit",
    "crc32c_repair_headers", "crc32c_triage_pages", "crc32c_scrub_pages", "crc32c_repair_bytes",
    "crc32c_locate_byte", "crc32c_batch_ptrs", "crc32c_ptrs_submit", "crc32c_chains_ptrs",
)


class Crc32cError(RuntimeError):
    def __init__(self, rc: int, what: str = ""):
        msg = lib.crc32c_strerror(rc).decode() if lib is not None else str(rc)
        super().__init__(f"{what}: {msg} ({rc})" if what else f"{msg} ({rc})")
        self.rc = rc


class Spans(ctypes.Structure):
    _fields_ = [
        ("base", ctypes.c_void_p),
        ("base_bytes", ctypes.c_uint64),
        ("offsets", ctypes.c_void_p),
        ("stride", ctypes.c_uint64),
        ("lens", ctypes.c_void_p),
        ("len", ctypes.c_uint32),
        ("crc_in", ctypes.c_void_p),
        ("out", ctypes.c_void_p),
        ("n", ctypes.c_uint64),
    ]


class ScrubOpts(ctypes.Structure):
    """crc32c_scrub_opts"""
    _fields_ = [
        ("mode", ctypes.c_uint32),
        ("max_span", ctypes.c_uint32),
        ("max_rounds", ctypes.c_uint32),
        ("stream", ctypes.c_void_p),
    ]


class ScrubOut(ctypes.Structure):
    """crc32c_scrub_out: the caller's arrays and their room, then the counts the call fills"""
    _fields_ = [
        ("offsets", ctypes.c_void_p),
        ("lens", ctypes.c_void_p),
        ("kind", ctypes.c_void_p),
        ("cap", ctypes.c_uint64),
        ("flip_offsets", ctypes.c_void_p),
        ("flip_bits", ctypes.c_void_p),
        ("flip_by", ctypes.c_void_p),
        ("flip_cap", ctypes.c_uint64),
        ("nitems", ctypes.c_uint64),
        ("nbad", ctypes.c_uint64),
        ("nsalvaged", ctypes.c_uint64),
        ("nsuspect", ctypes.c_uint64),
        ("scanned", ctypes.c_uint64),
        ("ncand", ctypes.c_uint64),
        ("nflips", ctypes.c_uint64),
        ("headers_repaired", ctypes.c_uint64),
        ("items_repaired", ctypes.c_uint64),
        ("rounds", ctypes.c_uint32),
        ("complete", ctypes.c_uint32),
    ]


class BytesOpts(ctypes.Structure):
    """crc32c_bytes_opts"""
    _fields_ = [
        ("mode", ctypes.c_uint32),
        ("max_span", ctypes.c_uint32),
        ("stream", ctypes.c_void_p),
    ]


class BytesOut(ctypes.Structure):
    """crc32c_bytes_out: the caller's three arrays, then the counts the call fills"""
    _fields_ = [
        ("ok", ctypes.c_void_p),
        ("byte", ctypes.c_void_p),
        ("mask", ctypes.c_void_p),
        ("nrepaired", ctypes.c_uint64),
        ("nbad", ctypes.c_uint64),
    ]


class PtrBatch(ctypes.Structure):
    """crc32c_ptr_batch"""
    _fields_ = [
        ("ptrs", ctypes.c_void_p),
        ("lens", ctypes.c_void_p),
        ("len", ctypes.c_uint32),
        ("crc_in", ctypes.c_void_p),
        ("out", ctypes.c_void_p),
        ("n", ctypes.c_uint64),
    ]


class PtrOpts(ctypes.Structure):
    """crc32c_ptr_opts"""
    _fields_ = [
        ("mode", ctypes.c_uint32),
        ("stream", ctypes.c_void_p),
    ]


_INT, _UINT, _U32, _U64 = ctypes.c_int, ctypes.c_uint, ctypes.c_uint32, ctypes.c_uint64
_SIZE, _PTR, _SPANS, _U64P = ctypes.c_size_t, ctypes.c_void_p, ctypes.POINTER(Spans), ctypes.POINTER(ctypes.c_uint64)
_SCALAR = (_U32, [_U32, _PTR, _SIZE])  # crc_func of include/crc32c.h
_ITEMS = (_INT, [_PTR, _U64, _U64, _PTR, _U64, _PTR, _U64P, _UINT, _PTR])
_PAGES = (_INT, [_PTR, _U64, _U64, _PTR, _PTR, _U64, _U64P, _U64P, _UINT, _PTR])

# name -> (restype, argtypes) of every function in EXPORTED, as include/*.h declares them
PROTOTYPES = {
    "crc32c_init": (None, []),
    "crc32c_sw": _SCALAR,
    "crc32c_sw_little": _SCALAR,
    "crc32c_sw_big": _SCALAR,
    "crc32c_gpu_count": (_INT, []),
    "crc32c_batch": (_INT, [_SPANS, _UINT, _PTR]),
    "crc32c_batch_multi": (_INT, [_SPANS, _INT]),
    "crc32c_verify_items": _ITEMS,
    "crc32c_stamp_items": _ITEMS,
    "crc32c_verify_pages": _PAGES,
    "crc32c_stamp_pages": _PAGES,
    "crc32c_copy_items": (_INT, [_PTR, _U64, _U64, _PTR, _PTR, _U64, _PTR, _U64, _PTR, _U64P, _UINT, _PTR]),
    "crc32c_salvage_pages": (_INT, [_PTR, _U64, _U64, _PTR, _PTR, _U64, _PTR, _U64, _U64P, _U64P, _U64P, _UINT,
                                    _PTR]),
    "crc32c_recover_pages": (_INT, [_PTR, _U64, _U64, _PTR, _PTR, _PTR, _U64, _U64P, _U64P, _U64P, _U64P, _U64P, _UINT,
                                    _PTR]),
    "crc32c_triage_pages": (_INT, [_PTR, _U64, _U64, _PTR, _PTR, _PTR, _U64, _U64P, _U64P, _U64P, _U64P, _U64P, _U64P,
                                   _UINT, _PTR]),
    "crc32c_repair_items": (_INT, [_PTR, _U64, _U64, _PTR, _U64, _U32, _PTR, _PTR, _U64P, _U64P, _UINT, _PTR]),
    "crc32c_locate_bit": (_U64, [_U32, _U32, _U64]),
    "crc32c_repair_headers": (_INT, [_PTR, _U64, _U64, _PTR, _U64, _PTR, _PTR, _PTR, _U64P, _U64P, _UINT, _PTR]),
    "crc32c_scrub_pages": (_INT, [_PTR, _U64, _U64, ctypes.POINTER(ScrubOpts), ctypes.POINTER(ScrubOut)]),
    "crc32c_repair_bytes": (_INT, [_PTR, _U64, _U64, _PTR, _U64, ctypes.POINTER(BytesOpts), ctypes.POINTER(BytesOut)]),
    "crc32c_locate_byte": (_U64, [_U32, _U32, _U64, ctypes.POINTER(ctypes.c_uint8)]),
    "crc32c_batch_chains": (_INT, [_SPANS, _PTR, _U64, _PTR, _UINT, _PTR]),
    "crc32c_batch_ptrs": (_INT, [ctypes.POINTER(PtrBatch), ctypes.POINTER(PtrOpts)]),
    "crc32c_ptrs_submit": (_INT, [ctypes.POINTER(PtrBatch), ctypes.POINTER(PtrOpts), ctypes.POINTER(_PTR)]),
    "crc32c_chains_ptrs": (_INT, [ctypes.POINTER(PtrBatch), _PTR, _U64, _PTR, ctypes.POINTER(PtrOpts)]),
    "crc32c_host_alloc": (_PTR, [_SIZE]),
    "crc32c_host_free": (None, [_PTR]),
    "crc32c_batch_submit": (_INT, [_SPANS, _UINT, ctypes.POINTER(_PTR)]),
    "crc32c_batch_wait": (_INT, [_PTR]),
    "crc32c_strerror": (ctypes.c_char_p, [_INT]),
    "crc32c_last_kernel_ms": (ctypes.c_float, []),
    "crc32c_shard_cuts": (_INT, [_PTR, _U32, _U64, _INT, _PTR]),
    "crc32c_queue_stats": (_INT, [_U64P] * 4),
    "crc32c_host_register": (_INT, [_PTR, _SIZE]),
    "crc32c_host_unregister": (_INT, [_PTR]),
    "crc32c_set_small_max": (_U64, [_U64]),
    "crc32c_set_k1_tail_min": (_U64, [_U64]),
}
# what an older build loaded through MCRC_LIB (an A/B of two builds) may lack
NEWER = ("crc32c_stamp_pages", "crc32c_copy_items", "crc32c_salvage_pages", "crc32c_set_k1_tail_min",
         "crc32c_recover_pages", "crc32c_repair_items", "crc32c_locate_bit", "crc32c_repair_headers",
         "crc32c_triage_pages", "crc32c_scrub_pages", "crc32c_repair_bytes", "crc32c_locate_byte",
         "crc32c_batch_ptrs", "crc32c_ptrs_submit", "crc32c_chains_ptrs")


def _load():
    if not os.path.exists(LIB_PATH):
        raise ImportError(f"{LIB_PATH} is missing: run `python -m memcached_amd.build`")
    # the HIP runtime already loaded by torch (same soname) is reused when present
    lib = ctypes.CDLL(LIB_PATH, mode=ctypes.RTLD_GLOBAL)
    for name, (restype, argtypes) in PROTOTYPES.items():
        if name in NEWER and os.environ.get("MCRC_LIB") and not hasattr(lib, name):
            continue
        f = getattr(lib, name)
        f.restype, f.argtypes = restype, argtypes
    lib.crc32c_init()
    return lib


lib = _load()

# the crc_func data symbol: a function pointer the callers invoke directly
CRC_FUNC = ctypes.CFUNCTYPE(ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_size_t)
_crc_ptr = ctypes.c_void_p.in_dll(lib, "crc32c")


def scalar_crc32c():
    """The function currently stored in the `crc32c` data symbol."""
    if not _crc_ptr.value:
        raise RuntimeError("crc32c_init() has not run")
    return CRC_FUNC(_crc_ptr.value)


def check(rc: int, what: str = "") -> None:
    if rc != CRC32C_OK:
        raise Crc32cError(rc, what)

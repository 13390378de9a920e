"""crc32c_scrub_pages with CRC32C_SCRUB_BYTES as the GPU tests call it: the raw
caller of tests/raw_calls.py with one more mode bit.  Its result dict, its
sentinels and its checker (raw_calls.expect_scrub) are that file's."""
import ctypes

from tests import raw_calls as raw

SCRUB_BYTES = 0x80
BY_BYTE = 3


def scrub_pages(side, buf, wbuf, *, cap, flip_cap, cfl=4, max_span=0, max_rounds=0, locate_only=False, gaps=False,
                byte_rule=False, null_arrays=False):
    """raw_calls.scrub_pages, and ``byte_rule`` sets CRC32C_SCRUB_BYTES."""
    m, side = raw._lib(), raw._side(side)
    page = side.data(buf)
    spec = tuple((name, dtype, cap if k < 3 else flip_cap) for k, (name, dtype) in enumerate(raw.SCRUB_LISTS))
    arrays, ptrs = raw._outs(side, spec, null_arrays)
    mode = side.flags(cfl == 8, locate_only=locate_only, gaps=gaps) | (SCRUB_BYTES if byte_rule else 0)
    opts = m.ScrubOpts(mode, max_span, max_rounds, side.handle)
    out = m.ScrubOut(*ptrs[:3], cap, *ptrs[3:], flip_cap, *([raw.SENT64] * 9), raw.SENT[4], raw.SENT[4])
    rc = m.lib.crc32c_scrub_pages(raw.ptr(page), buf.size, wbuf, ctypes.byref(opts), ctypes.byref(out))
    return raw._result(side, rc, page, arrays, spec, {w: getattr(out, w) for w in raw.SCRUB_WORDS},
                       rooms={name: room for name, _, room in spec}, ms=m.lib.crc32c_last_kernel_ms())

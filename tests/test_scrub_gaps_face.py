"""scrub_pages' ``gaps`` argument, pinned without a GPU through the stub of
tests/test_scrub_face.py in the library's place: it puts CRC32C_SCRUB_GAPS into
the mode word and changes nothing else of the call; and the constant in the
header and in the module."""
import re

import numpy as np
import pytest

from memcached_amd import _lib
from memcached_amd import crc32c as mc
from tests.test_scrub_face import REPLY, SIZE, W, Stub


@pytest.fixture
def buf():
    return np.arange(SIZE, dtype=np.uint32).astype(np.uint8)


def _call(monkeypatch, buf, **kw):
    s = Stub([REPLY])
    monkeypatch.setattr(mc, "lib", s)
    got = mc.scrub_pages(buf.copy(), W, **kw)
    call, = s.calls
    return call, got


@pytest.mark.parametrize("kw", [{}, dict(max_span=4096, max_rounds=7, cflags64=True), dict(locate_only=True)])
def test_gaps_sets_the_bit_and_nothing_else(monkeypatch, buf, kw):
    off, got_off = _call(monkeypatch, buf, **kw)
    on, got_on = _call(monkeypatch, buf, gaps=True, **kw)
    assert on["mode"] == off["mode"] | 0x40 and not off["mode"] & 0x40
    skip = ("mode", "base", "offsets", "lens", "kind", "flip_offsets", "flip_bits", "flip_by")  # (addresses)
    assert {k: v for k, v in on.items() if k not in skip} == {k: v for k, v in off.items() if k not in skip}
    assert [a.tolist() for a in got_on[:6]] == [a.tolist() for a in got_off[:6]] and got_on[6] == got_off[6]
    explicit, _ = _call(monkeypatch, buf, gaps=False, **kw)
    assert explicit["mode"] == off["mode"]


def test_the_constant_is_in_the_header_and_the_module():
    header = open(_lib.PKG + "/../include/crc32c_batch.h").read()
    assert int(re.search(r"#define CRC32C_SCRUB_GAPS (0x[0-9a-f]+)u", header).group(1), 16) == 0x40
    assert _lib.CRC32C_SCRUB_GAPS == mc.CRC32C_SCRUB_GAPS == 0x40
    others = (_lib.CRC32C_DEVICE, _lib.CRC32C_ASYNC, _lib.CRC32C_CFLAGS64, _lib.CRC32C_KEEP_STAMPED,
              _lib.CRC32C_LOCATE_ONLY)
    assert all(not 0x40 & b for b in others)

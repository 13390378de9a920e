"""scrub_pages' ``byte_rule`` argument, pinned without a GPU through the stub
of tests/test_scrub_face.py in the library's place: it puts CRC32C_SCRUB_BYTES
into the mode word and changes nothing else of the call; the two constants in
the header and in the module; and the two structs' sizes, which the mode bit
must leave alone."""
import ctypes
import re

import numpy as np
import pytest

from memcached_amd import _lib
from memcached_amd import crc32c as mc
from tests.test_scrub_face import REPLY, SIZE, W, Stub

BY_BYTE_REPLY = dict(REPLY, flip_offsets=[100, 100, 4096], flip_bits=[402, 404, 9], flip_by=[3, 3, 1], nflips=3)


@pytest.fixture
def buf():
    return np.arange(SIZE, dtype=np.uint32).astype(np.uint8)


def _call(monkeypatch, buf, reply=REPLY, **kw):
    s = Stub([reply])
    monkeypatch.setattr(mc, "lib", s)
    page = buf.copy()
    got = mc.scrub_pages(page, W, **kw)
    call, = s.calls
    return call, got, page


@pytest.mark.parametrize("kw", [{}, dict(max_span=4096, max_rounds=7, cflags64=True), dict(locate_only=True),
                                dict(gaps=True)])
def test_byte_rule_sets_the_bit_and_nothing_else(monkeypatch, buf, kw):
    off, got_off, _ = _call(monkeypatch, buf, **kw)
    on, got_on, _ = _call(monkeypatch, buf, byte_rule=True, **kw)
    assert on["mode"] == off["mode"] | 0x80 and not off["mode"] & 0x80
    skip = ("mode", "base", "offsets", "lens", "kind", "flip_offsets", "flip_bits", "flip_by")  # (addresses)
    assert {k: v for k, v in on.items() if k not in skip} == {k: v for k, v in off.items() if k not in skip}
    assert [a.tolist() for a in got_on[:6]] == [a.tolist() for a in got_off[:6]] and got_on[6] == got_off[6]
    explicit, _, _ = _call(monkeypatch, buf, byte_rule=False, **kw)
    assert explicit["mode"] == off["mode"]


def test_it_composes_with_gaps(monkeypatch, buf):
    both, _, _ = _call(monkeypatch, buf, gaps=True, byte_rule=True)
    assert both["mode"] & 0xC0 == 0xC0


def test_a_host_page_gets_every_logged_bit_of_a_byte(monkeypatch, buf):
    """The log is per bit: the face inverts a byte stage's entries as any other's."""
    _, got, page = _call(monkeypatch, buf, BY_BYTE_REPLY, byte_rule=True)
    want = buf.copy()
    want[100 + 50] ^= 0x14
    want[4096 + 1] ^= 0x02
    assert (page == want).all()
    assert got[5].tolist() == [3, 3, 1] and got[6]["nflips"] == 3


def test_the_constants_are_in_the_header_and_the_module():
    header = open(_lib.PKG + "/../include/crc32c_batch.h").read()
    assert int(re.search(r"#define CRC32C_SCRUB_BYTES\s+(0x[0-9a-f]+)u", header).group(1), 16) == 0x80
    assert int(re.search(r"#define CRC32C_SCRUB_BY_BYTE\s+(\d+)", header).group(1)) == 3
    assert _lib.CRC32C_SCRUB_BYTES == mc.CRC32C_SCRUB_BYTES == 0x80
    assert _lib.CRC32C_SCRUB_BY_BYTE == mc.CRC32C_SCRUB_BY_BYTE == 3
    assert len({_lib.CRC32C_SCRUB_BY_HEADER, _lib.CRC32C_SCRUB_BY_ITEM, _lib.CRC32C_SCRUB_BY_BYTE}) == 3


def test_the_bit_collides_with_no_other_flag():
    header = open(_lib.PKG + "/../include/crc32c_batch.h").read()
    others = (_lib.CRC32C_DEVICE, _lib.CRC32C_ASYNC, _lib.CRC32C_CFLAGS64, _lib.CRC32C_KEEP_STAMPED,
              _lib.CRC32C_LOCATE_ONLY, _lib.CRC32C_SCRUB_GAPS)
    assert all(not 0x80 & b for b in others)
    # every one-bit flag the header defines below 0x100, by name
    flags = {n: int(v, 16) for n, v in re.findall(r"#define (CRC32C_\w+)\s+(0x[0-9a-f]{1,2})u\s", header)}
    assert flags["CRC32C_SCRUB_BYTES"] == 0x80 and len(flags) >= 7
    assert [n for n, v in flags.items() if v & 0x80] == ["CRC32C_SCRUB_BYTES"]


def test_the_structs_keep_their_sizes():
    assert ctypes.sizeof(_lib.ScrubOpts) == 24 and ctypes.sizeof(_lib.ScrubOut) == 144

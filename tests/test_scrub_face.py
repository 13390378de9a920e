"""What memcached_amd.crc32c.scrub_pages hands to the library and makes of its
answer, pinned without a GPU through a stub in the library's place (as
tests/test_python_face.py does for the other calls): the two structs' fields,
the capacities, the retry, and who inverts the bits of a host page."""
import ctypes

import numpy as np
import pytest

from memcached_amd import _lib
from memcached_amd import crc32c as mc

SIZE, W = 16 << 10, 4096
FIELDS = [f for f, _ in _lib.ScrubOut._fields_]


class Stub:
    """crc32c_scrub_pages alone.  Each call's arguments and struct fields are
    recorded; ``script`` (a list of dicts, the last repeats) gives the status,
    the count fields and the entries written through the array pointers."""

    def __init__(self, script):
        self.script, self.calls = list(script), []

    def crc32c_scrub_pages(self, base, nbytes, wbuf, opts, out):
        o, r = opts._obj, out._obj
        self.calls.append(dict(base=base, nbytes=nbytes, wbuf=wbuf, mode=o.mode, max_span=o.max_span,
                               max_rounds=o.max_rounds, stream=o.stream, **{f: getattr(r, f) for f in FIELDS[:8]}))
        reply = self.script.pop(0) if len(self.script) > 1 else self.script[0]
        for name, ctype, room in (("offsets", ctypes.c_uint64, r.cap), ("lens", ctypes.c_uint32, r.cap),
                                  ("kind", ctypes.c_uint8, r.cap), ("flip_offsets", ctypes.c_uint64, r.flip_cap),
                                  ("flip_bits", ctypes.c_uint64, r.flip_cap), ("flip_by", ctypes.c_uint8, r.flip_cap)):
            vals = reply.get(name, [])[:room]
            (ctype * len(vals)).from_address(getattr(r, name))[:] = vals
        for f in FIELDS[8:]:
            setattr(r, f, reply.get(f, 0))
        return reply.get("rc", 0)

    def crc32c_strerror(self, rc):
        return b"stub"


REPLY = dict(offsets=[0, 100, 4096], lens=[100, 60, 70], kind=[1, 4, 6], flip_offsets=[100, 4096], flip_bits=[403, 9],
             flip_by=[2, 1], nitems=3, nbad=0, nsalvaged=1, nsuspect=1, scanned=500, ncand=3, nflips=2,
             headers_repaired=1, items_repaired=1, rounds=2, complete=1)


@pytest.fixture
def buf():
    return np.arange(SIZE, dtype=np.uint32).astype(np.uint8)


def _install(monkeypatch, script):
    s = Stub(script)
    monkeypatch.setattr(mc, "lib", s)
    return s


def test_one_call_marshals_and_slices(monkeypatch, buf):
    s = _install(monkeypatch, [REPLY])
    before = buf.copy()
    offs, lens, kind, fo, fb, fy, info = mc.scrub_pages(buf, W, max_span=4096, max_rounds=7, cflags64=True)
    c, = s.calls
    assert (c["base"], c["nbytes"], c["wbuf"]) == (buf.ctypes.data, SIZE, W)
    # a host call runs locate-only: it can be made again when the arrays turn out too small
    assert c["mode"] == _lib.CRC32C_CFLAGS64 | _lib.CRC32C_LOCATE_ONLY and c["stream"] is None
    assert (c["max_span"], c["max_rounds"]) == (4096, 7)
    assert c["cap"] == SIZE // 50 + SIZE // W + SIZE // 50 and c["flip_cap"] == SIZE // 256 + 64
    assert all(c[f] for f in FIELDS[:8])
    assert (offs.dtype, lens.dtype, kind.dtype, fo.dtype, fb.dtype, fy.dtype) == (
        np.uint64, np.uint32, np.uint8, np.uint64, np.uint64, np.uint8)
    assert [a.tolist() for a in (offs, lens, kind, fo, fb, fy)] == [REPLY[k] for k in FIELDS[:3] + FIELDS[4:7]]
    assert info == dict({k: REPLY[k] for k in FIELDS[9:]}, rc=0)
    # ... and the logged bits are inverted here
    want = before.copy()
    want[100 + 403 // 8] ^= 1 << (403 % 8)
    want[4096 + 1] ^= 1 << 1
    assert (buf == want).all()


def test_locate_only_leaves_the_buffer(monkeypatch, buf):
    s = _install(monkeypatch, [REPLY])
    before = buf.copy()
    buf.flags.writeable = False
    *_, info = mc.scrub_pages(buf, W, locate_only=True)
    assert s.calls[0]["mode"] == _lib.CRC32C_LOCATE_ONLY and (buf == before).all() and info["nflips"] == 2
    assert mc.scrub_pages(bytes(64), 64, locate_only=True)[-1]["complete"] == 1


def test_a_call_that_outgrows_its_arrays_is_made_again(monkeypatch, buf):
    cap, flip_cap = SIZE // 50 + SIZE // W + SIZE // 50, SIZE // 256 + 64
    big = dict(REPLY, nitems=cap + 5, nflips=flip_cap + 1, offsets=list(range(cap + 5)), lens=[60] * (cap + 5),
               kind=[6] * (cap + 5), flip_offsets=[0] * (flip_cap + 1), flip_bits=[8 * 50] * (flip_cap + 1),
               flip_by=[2] * (flip_cap + 1))
    s = _install(monkeypatch, [big])
    before = buf.copy()
    offs, lens, kind, fo, fb, fy, info = mc.scrub_pages(buf, W)
    assert [(c["cap"], c["flip_cap"]) for c in s.calls] == [(cap, flip_cap), (cap + 5, flip_cap + 1)]
    assert len(offs) == len(kind) == cap + 5 and len(fb) == flip_cap + 1 and info["nflips"] == flip_cap + 1
    assert buf[50] == before[50] ^ ((flip_cap + 1) & 1) and (buf[51:] == before[51:]).all()


@pytest.mark.parametrize("rc", [_lib.CRC32C_EWORK, _lib.CRC32C_EWALK])
def test_a_stage_status_comes_back_in_info(monkeypatch, buf, rc):
    _install(monkeypatch, [dict(REPLY, rc=rc, complete=0)])
    assert mc.scrub_pages(buf, W)[-1]["rc"] == rc


def test_other_statuses_raise(monkeypatch, buf):
    _install(monkeypatch, [dict(rc=_lib.CRC32C_ENODEV)])
    with pytest.raises(mc.Crc32cError) as e:
        mc.scrub_pages(buf, W)
    assert e.value.rc == _lib.CRC32C_ENODEV


def test_rejections(monkeypatch, buf):
    s = _install(monkeypatch, [REPLY])
    with pytest.raises(ValueError):
        mc.scrub_pages(buf, 0)
    with pytest.raises(TypeError):
        mc.scrub_pages(bytes(buf), W)  # (not writable: only with locate_only)
    assert s.calls == []


def test_struct_layouts_are_the_headers():
    assert [f for f, _ in _lib.ScrubOpts._fields_] == ["mode", "max_span", "max_rounds", "stream"]
    assert ctypes.sizeof(_lib.ScrubOpts) == 24 and _lib.ScrubOpts.stream.offset == 16
    assert ctypes.sizeof(_lib.ScrubOut) == 8 * 8 + 9 * 8 + 8 and _lib.ScrubOut.rounds.offset == 136
    header = open(_lib.PKG + "/../include/crc32c_batch.h").read()
    body = header[header.index("typedef struct crc32c_scrub_out"):header.index("} crc32c_scrub_out;")]
    import re
    names = re.findall(r"[\*\s,](\w+)(?=\s*[,;])", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    assert names == FIELDS
    for name in ("CRC32C_SCRUB_ROUNDS_DEFAULT", "CRC32C_SCRUB_BY_HEADER", "CRC32C_SCRUB_BY_ITEM"):
        assert int(re.search(rf"#define {name} (\d+)", header).group(1)) == getattr(_lib, name)

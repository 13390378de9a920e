"""The rule of crc32c_repair_headers (include/crc32c_batch.h) restated over
numpy, with the CRCs from the CPU oracle.  Nothing here comes from the library.

The rule is stated twice.  ``hits_flip`` is the rule as written: invert each of
the 42 length bits in turn, judge the header that results, recompute the CRC of
its span through the oracle and compare it with the stored one.
``hits_xpow`` leaves the buffer as it stands: the CRC of the variant's span as
the buffer has it, XOR x^t for the exponent t the bit has in that span
(tests/repair_model.py: ``xpow``, ``t_of_k``), compared with the stored one.
``repair_one`` is the whole verdict of one header, ``repair`` of a list."""
import numpy as np

from tests import oracle
from tests import repair_model as rm
from tests import salvage_model as sm

NO_BIT, REPAIRED = rm.NO_BIT, rm.REPAIRED
HEADER_BITS = 42
WORK_MAX = 8
# the 42 length bits by image bit index: nbytes, nkey, it_flags bit 1 (ITEM_CAS), it_flags bit 8 (ITEM_CFLAGS)
BITS = list(range(256, 288)) + list(range(328, 336)) + [305, 312]
assert len(BITS) == HEADER_BITS and all(rm.length_bit(k) for k in BITS)
assert [k for k in range(8 * 48) if rm.length_bit(k)] == sorted(BITS)


def _stored(buf, o):
    return int.from_bytes(bytes(buf[o + 28:o + 32]), "little")


def _flip(buf, o, k):
    buf[o + k // 8] ^= 1 << (k % 8)


def candidates(buf, o, region=0, cfl=4):
    """[(k, nt')] of the variants of the header at o that are candidates: sane,
    nbytes' >= 2, CRLF at the end.  ``buf`` is inverted and restored in place."""
    out = []
    for k in BITS:
        _flip(buf, o, k)
        nt = sm.candidate(buf, region or (1 << 62), o, cfl)
        _flip(buf, o, k)
        if nt:
            out.append((k, nt))
    return out


def hits_flip(buf, o, region=0, cfl=4):
    """The candidates whose span, with their bit inverted, has the stored CRC."""
    out = []
    for k, nt in candidates(buf, o, region, cfl):
        _flip(buf, o, k)
        if oracle.crc32c(0, buf[o + 32:o + nt]) == _stored(buf, o):
            out.append((k, nt))
        _flip(buf, o, k)
    return out


def hits_xpow(buf, o, region=0, cfl=4):
    """The same from the buffer as it stands: crc ^ x^t == stored."""
    return [(k, nt) for k, nt in candidates(buf, o, region, cfl)
            if oracle.crc32c(0, buf[o + 32:o + nt]) ^ rm.xpow(rm.t_of_k(k, nt)) == _stored(buf, o)]


def repair_one(buf, o, region=0, cfl=4, flip=False):
    """(ok, bit, lens) of the header at o.  ``buf``: a writable array (restored)."""
    if o >= len(buf) or len(buf) - o < 48:
        return 0, NO_BIT, 0
    nt = sm.sane(buf, region or (1 << 62), o, cfl)
    if nt and oracle.crc32c(0, buf[o + 32:o + nt]) == _stored(buf, o):
        return 1, NO_BIT, nt
    hits = (hits_flip if flip else hits_xpow)(buf, o, region, cfl)
    if len(hits) != 1:
        return 0, NO_BIT, 0
    return REPAIRED, hits[0][0], hits[0][1]


def work(buf, offsets, region=0, cfl=4):
    """The work bound's sum: every candidate variant's span."""
    buf, total = sm._u8(buf).copy(), 0
    for o in np.asarray(offsets).tolist():
        o = int(o)
        if o < len(buf) and len(buf) - o >= 48:
            total += sum(n - 32 for _, n in candidates(buf, o, region, cfl))
    return total


def ncandidates(buf, offsets, region=0, cfl=4):
    buf = sm._u8(buf).copy()
    return sum(len(candidates(buf, int(o), region, cfl)) for o in np.asarray(offsets).tolist()
               if int(o) < len(buf) and len(buf) - int(o) >= 48)


def repair(buf, offsets, region=0, cfl=4, locate_only=False):
    """(ok, bit, lens, nrepaired, nbad, the buffer afterwards) for distinct offsets."""
    buf = sm._u8(buf).copy()
    after = buf.copy()
    n = len(offsets)
    ok, bit, lens = np.zeros(n, np.uint8), np.full(n, NO_BIT, np.uint64), np.zeros(n, np.uint32)
    assert work(buf, offsets, region, cfl) <= WORK_MAX * len(buf), "over the work bound: CRC32C_EWORK"
    for i, o in enumerate(np.asarray(offsets).tolist()):
        ok[i], b, lens[i] = repair_one(buf, int(o), region, cfl)
        bit[i] = b
        if ok[i] == REPAIRED and not locate_only:
            _flip(after, int(o), b)
    return ok, bit, lens, int((ok == REPAIRED).sum()), int((ok == 0).sum()), after

"""The rule of crc32c_salvage_pages (include/crc32c_batch.h) restated over
numpy, with the CRCs from the CPU oracle.  Nothing here comes from the library.

Two versions that must agree: ``salvage_bytewise`` is the rule as written, one
offset at a time; ``salvage_fast`` finds the candidates with vectorised numpy
and goes through them only (for the larger buffers of the GPU tests).  Both
return (offsets, scanned, ncand, work)."""
import numpy as np

from tests import oracle

MAX_SPAN = 0x7FFF0000
WORK_MAX = 64


def _u8(buf):
    return np.ascontiguousarray(buf).view(np.uint8).reshape(-1)


def piece_end(o, W, n):
    return min((o // W + 1) * W, n)


def ntotal_at(buf, o, cfl=4):
    nbytes = int.from_bytes(bytes(buf[o + 32:o + 36]), "little")
    flags = int(buf[o + 38]) | int(buf[o + 39]) << 8
    return 48 + int(buf[o + 41]) + 1 + nbytes + (cfl if flags & 256 else 0) + (8 if flags & 2 else 0), nbytes


def sane(buf, W, o, cfl=4):
    """ITEM_ntotal when the header at o is sane (mcrc::item_sane), else 0."""
    n = len(buf)
    if o > n or n - o < 48:
        return 0
    nt, nbytes = ntotal_at(buf, o, cfl)
    if buf[o + 41] == 0 or nbytes >= 1 << 31 or nt - 32 > MAX_SPAN or nt > n - o or o // W != (o + nt - 1) // W:
        return 0
    return nt


def candidate(buf, W, o, cfl=4):
    nt = sane(buf, W, o, cfl)
    if not nt or ntotal_at(buf, o, cfl)[1] < 2 or buf[o + nt - 2] != 13 or buf[o + nt - 1] != 10:
        return 0
    return nt


def intact(buf, W, o, cfl=4):
    nt = candidate(buf, W, o, cfl)
    if not nt:
        return 0
    stored = int.from_bytes(bytes(buf[o + 28:o + 32]), "little")
    return nt if oracle.crc32c(0, buf[o + 32:o + nt]) == stored else 0


def covered_mask(buf, W, walked, walked_ok, cfl=4):
    """One flag per byte: inside an image the walk's lists cover."""
    cov = np.zeros(len(buf), bool)
    if walked is not None:
        for o, ok in zip(np.asarray(walked).tolist(), np.asarray(walked_ok).tolist()):
            nt = sane(buf, W, int(o), cfl) if ok else 0
            if nt:
                cov[int(o):int(o) + nt] = True
    return cov


def salvage_bytewise(buf, W, walked=None, walked_ok=None, cfl=4):
    buf = _u8(buf)
    n = len(buf)
    cov = covered_mask(buf, W, walked, walked_ok, cfl)
    scanned = ncand = work = 0
    for o in range(n):
        if piece_end(o, W, n) - o >= 48 and not cov[o]:
            scanned += 1
            nt = candidate(buf, W, o, cfl)
            if nt:
                ncand += 1
                work += nt - 32
    found = []
    if work <= WORK_MAX * (scanned + W):
        for ps in range(0, n, W):
            pe, o = min(ps + W, n), ps
            while pe - o >= 48:
                if cov[o]:
                    o += 1  # (to the end of the covering image, one covered byte at a time)
                    continue
                nt = intact(buf, W, o, cfl)
                if nt:
                    found.append(o)
                    o += nt
                else:
                    o += 1
    return found, scanned, ncand, work


def regions(buf, W, walked=None, walked_ok=None, cfl=4):
    """The maximal runs [lo, hi) of eligible offsets, ascending (what the
    kernels' region pass cuts from the lists)."""
    buf = _u8(buf)
    n = len(buf)
    cov = covered_mask(buf, W, walked, walked_ok, cfl)
    out = []
    for ps in range(0, n, W):
        pe = min(ps + W, n)
        last = pe - 47 if pe - ps >= 48 else ps
        e = np.flatnonzero(np.diff(np.concatenate(([0], (~cov[ps:last]).astype(np.int8), [0]))))
        out += [(ps + int(a), ps + int(b)) for a, b in zip(e[0::2], e[1::2])]
    return out


def _candidates_fast(buf, W, cov, cfl, block=8 << 20):
    """(offsets, ntotals) of every eligible candidate, and the eligible count."""
    n = len(buf)
    offs, nts, scanned = [], [], 0
    step = max(W, block // W * W)
    for b0 in range(0, n, step):
        hi = min(b0 + step, n - 47)  # offsets with 48 bytes left in the buffer
        if hi <= b0:
            continue
        # eligible offsets, then the ones with nkey != 0 (most of a zero tail
        # goes here), then the fields of those alone
        o = np.arange(b0, hi, dtype=np.int64)
        pe = np.minimum((o // W + 1) * W, n)
        elig = (pe - o >= 48) & ~cov[b0:hi]
        scanned += int(elig.sum())
        keep = elig & (buf[b0 + 41:hi + 41] != 0)
        o, pe = o[keep], pe[keep]

        def byte(k):
            return buf[o + k].astype(np.int64)
        nbytes = byte(32) | byte(33) << 8 | byte(34) << 16 | byte(35) << 24
        flags = byte(38) | byte(39) << 8
        nt = 49 + byte(41) + nbytes + np.where(flags & 256, cfl, 0) + np.where(flags & 2, 8, 0)
        ok = (nbytes < 1 << 31) & (nt - 32 <= MAX_SPAN) & (o + nt <= pe) & (nbytes >= 2)
        so, snt = o[ok], nt[ok]
        crlf = (buf[so + snt - 2] == 13) & (buf[so + snt - 1] == 10)
        offs.append(so[crlf])
        nts.append(snt[crlf])
    cat = (lambda x: np.concatenate(x) if x else np.zeros(0, np.int64))
    return cat(offs), cat(nts), scanned


def salvage_fast(buf, W, walked=None, walked_ok=None, cfl=4):
    buf = _u8(buf)
    cov = covered_mask(buf, W, walked, walked_ok, cfl)
    offs, nts, scanned = _candidates_fast(buf, W, cov, cfl)
    work = int((nts - 32).sum())
    found = []
    if work <= WORK_MAX * (scanned + W):
        end = 0  # (images stay inside their piece, so one running end serves every piece)
        for o, nt in zip(offs.tolist(), nts.tolist()):
            if o < end:
                continue
            stored = int.from_bytes(bytes(buf[o + 28:o + 32]), "little")
            if oracle.crc32c(0, buf[o + 32:o + nt]) == stored:
                found.append(o)
                end = o + nt
    return found, scanned, len(offs), work

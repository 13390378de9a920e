"""CPU restatement of k_count's wave-cooperative whole spans (round 4,
k_plan.h whole_chunks / k_common.h span_corr_arg's pieces case).

A span D = [p, E) of vlen = len + t <= kWholeMax bytes is all its thread's
(span_corr: z = M_t(f), f the register after D from ~c).  Its lane no longer
runs that chain alone while the other 63 lanes of the wave idle: the wave
cuts the pieces [ph, ceil16(E)) of all its whole spans (ph = floor16(p),
Ea = E + t; floor16 and ceil16 of addresses -- the kernel works in offsets
from base, whose address need not be a multiple of 16, so the model carries
the base's residue b and rounds b + offset) into 128-B chunks, every lane takes a chunk (r_c = raw of its
<= 8 pieces, the span's last piece cleared from E on, shifted past the rest
of the span: M_{Ea - end_c}(r_c)), and the chunks of one span are XORed into
R = raw([ph, Ea)) as the pieces lie with the tail F_t = [E, Ea) cleared, as
the span kernel clears it (round 5).  Then
    z = R ^ Z,  Z = M_{len+t}(~c ^ raw(F_h))
(F_h: the kh foreign bytes before p, moved to the top of a zero piece) --
the identity the span kernel's units rest on.  The owner of chunk q is the
first lane whose inclusive chunk count exceeds q.
"""
import numpy as np
import pytest

from tests import oracle
from tests.span_model import M32, WHOLE_MAX, mulmodp, span_head, tail_pad, xpow8

CHUNK = 128


def raw(data):
    return ~oracle.crc32c(M32, bytes(data)) & M32


def reg(r, data):
    return ~oracle.crc32c(~r & M32, bytes(data)) & M32


def zeros(v, n):
    return oracle.lib().oracle_shift_zeros(v & M32, n)


def is_whole(p, length, b=0):
    """The span at offset p of a base whose address is b mod 16 is all its thread's."""
    g1o, drop = span_head(b + p, length)
    return length > 0 and drop and g1o == length + tail_pad(b + p, length)


def chunks_R(buf, ph, e, ea, chunk=CHUNK, b=0, round_offset=False):
    """R as the wave forms it from chunk-byte chunks (kWholeChunk) over the
    pieces [ph, ceil16(e)), the last one cleared from e on.

    ph, e and ea are offsets from base, as k_count passes them, and base's
    address is b mod 16: the byte at offset o lies at address b + o, which is
    where it is in buf.  Pieces are 16-byte aligned as addresses, so ph + b is
    a multiple of 16 and the end of the pieces is rounded up in the address
    domain: e16 = ceil16(e + b) - b.  round_offset: ceil16(e) instead, the
    form that holds for b = 0 alone (test_rounding_the_offset_is_wrong_off_the_grid).
    The chunk loop is the kernel's: a chunk takes min(8, (e16 - c0) >> 4)
    pieces, and the one that ends at e16 clears its last piece from e on."""
    assert (ph + b) % 16 == 0
    e16 = (e + 15) & ~15 if round_offset else ((e + b + 15) & ~15) - b
    R = 0
    for c0 in range(ph, e16, chunk):
        np_ = min(chunk // 16, (e16 - c0) >> 4)
        pieces = [bytearray(buf[b + c0 + 16 * k:b + c0 + 16 * k + 16]) for k in range(np_)]
        if np_ and c0 + 16 * np_ == e16:
            keep = 16 - (e16 - e)
            pieces[-1][keep:] = bytes(16 - keep)
        r = 0
        for piece in pieces:
            r = reg(r, piece)
        after = ea - (c0 + 16 * np_)
        R ^= mulmodp(r, xpow8(after)) if after else r
    return R


def z_pieces(buf, p, length, c):
    """span_corr's pieces-as-they-lie correction (its non-drop branch)."""
    kh = p & 15
    t = tail_pad(p, length)
    y = ~c & M32
    if kh:
        y ^= raw(bytes(16 - kh) + bytes(buf[p - kh:p]))
    return mulmodp(y, xpow8(length + t))


def owners(nch):
    """(owner lane, chunk index) of every chunk q, by the kernel's search."""
    inc = np.cumsum(nch)
    excl = inc - nch
    out = []
    for q in range(int(inc[-1]) if len(inc) else 0):
        s = 0
        for step in (32, 16, 8, 4, 2, 1):
            if inc[s + step - 1] <= q:
                s += step
        out.append((s, q - int(excl[s])))
    return out


BASES = (0, 1, 8, 15)  # base & 15: the grid, one past it, half a piece, one short of it


@pytest.mark.parametrize("seed", range(6))
def test_whole_span_chunks_give_the_thread_chain(seed):
    """For every base residue b: p is the span's offset from a base at address
    b mod 16, and buf holds the bytes by address."""
    for b in BASES:
        rng = np.random.default_rng(seed)
        buf = rng.integers(0, 256, 1 << 15, dtype=np.uint8).tobytes()
        seen = 0
        for _ in range(60):
            length = int(rng.integers(1, WHOLE_MAX + 1))
            p = int(rng.integers(16, len(buf) - length - 32))
            if not is_whole(p, length, b):
                continue
            seen += 1
            c = int(rng.integers(0, 1 << 32))
            a = b + p  # the span's address
            t = tail_pad(a, length)
            ph, e, ea = p - (a & 15), p + length, p + length + t
            R = chunks_R(buf, ph, e, ea, b=b)
            assert R == raw(bytes(buf[b + ph:b + e]) + bytes(t)), b
            for chunk in (32, 64, 256):  # (other chunk sizes: the same R)
                assert chunks_R(buf, ph, e, ea, chunk, b=b) == R, b
            f = reg(~c & M32, buf[a:a + length])
            assert R ^ z_pieces(buf, a, length, c) == zeros(f, t), b  # = span_corr's M_t(f)
            assert ~f & M32 == oracle.crc32c(c, buf[a:a + length])
        assert seen >= 10, (b, seen)


def test_rounding_the_offset_is_wrong_off_the_grid():
    """Why e16 is rounded as an address.  With base & 15 = b != 0, ceil16 of
    the offset e is no piece boundary: the chunk that should clear the last
    piece from e on never ends there (the foreign bytes behind the span stay
    in R), and where ceil16(e) falls short of the piece end the last piece is
    not read at all.  Every whole span whose end is not itself a piece
    boundary (e + b not 0 mod 16) comes out wrong; with b = 0 the two forms
    are one."""
    rng = np.random.default_rng(77)
    buf = rng.integers(1, 256, 1 << 14, dtype=np.uint8).tobytes()  # (no zero bytes: nothing cleared by luck)
    wrong = {b: 0 for b in BASES}
    for b in BASES:
        for length, p in ((1, 100), (15, 161), (16, 200), (100, 333), (129, 1000), (1000, 2001), (1024, 4099)):
            a = b + p
            if not is_whole(p, length, b) or (a + length) % 16 == 0:
                continue
            t = tail_pad(a, length)
            ph, e, ea = p - (a & 15), p + length, p + length + t
            want = raw(bytes(buf[b + ph:b + e]) + bytes(t))
            assert chunks_R(buf, ph, e, ea, b=b) == want
            got = chunks_R(buf, ph, e, ea, b=b, round_offset=True)
            assert (got == want) == (b == 0), (b, length, p)
            wrong[b] += got != want
    assert wrong[0] == 0 and all(wrong[b] >= 4 for b in BASES[1:]), wrong


def test_whole_spans_are_at_most_17_chunks():
    for length in range(1, WHOLE_MAX + 1):
        for al in range(16):
            if is_whole(al, length):
                assert (length + tail_pad(al, length) + al + CHUNK - 1) // CHUNK <= 9


@pytest.mark.parametrize("seed", range(4))
def test_chunk_owner_search(seed):
    rng = np.random.default_rng(seed)
    nch = rng.integers(0, 18, 64) * (rng.random(64) < 0.3)
    got = owners(nch)
    want = [(s, k) for s in range(64) for k in range(int(nch[s]))]
    assert got == want

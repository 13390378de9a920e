"""K1's window order on the GPU (k1_walk, k_consts.h; the loops of
k_fixed_body): every CRC against the CPU oracle at the smallest counts where
the window order runs and can go wrong, with a sentinel behind out[n].

With W = 16 x CUs waves and R = kK1RoundsMinSteps (32) steps per wave, the
first launches with lockstep rounds, and so with windows, are around
n0 = 2 W R items.  Without the claimed tail (the threshold at UINT64_MAX):
  n0, n0 - 1, n0 - 2      full windows; the last window cut by one item / group
  n0 + 1, n0 + 2          R + 1 steps per wave: a remainder of one step, most of
                          the last windows past the batch
  n0 - 2 x 16 R           one workgroup's window short of full
  n0 - 2 x 64             one pass short of a full window
  2 (W (R + 1) + 8) - 1   R + 2 steps: a remainder of two, an odd count
  2 (W (R + 2) + 8) + 1   R + 3 steps: a remainder of three
  n0 - 2 W                R - 1 steps per wave: no rounds, so the ranges
With the claimed tail, the threshold at its floor (crc32c_set_k1_tail_min,
restored afterwards): 2 W 37 and 2 W 37 - 3, the first static parts of 32 steps,
windows in the static part and the last pass of each left to the tail loop; and
2 W 40, the first launch that runs both by default.
Each with and without crc_in at stride 4096; one case at stride 4224, one with
the base 16 B past a line (the default-policy kernel, where neighbouring waves
share a line), and two launches back to back on one stream.

A miscounted barrier hangs, not miscomputes, so tools/gpu_suite.sh runs this
module in its first, stand-alone step and stops there on any failure.  The data
and the oracle's CRCs are computed once for the largest case: item i at stride
4096 is the same bytes in every case."""
import ctypes

import numpy as np
import pytest

try:  # GPU processes load torch (and its HIP runtime) before libmcrc32c.so
    import torch as _torch  # noqa: F401
except ImportError:
    pass

from memcached_amd import _lib

from . import k1_order_model as o
from . import k1_rounds_model as m
from . import k1_tail_model as t
from . import oracle

pytestmark = pytest.mark.gpu
NEVER = 2**64 - 1
SENTINEL = 0x5a5a5a5a
R = 32
WIDE, OFF16 = 4224, 16  # a second 128-B aligned stride; a base offset that takes the default-policy kernel

STATIC = {
    "n0": lambda W: 2 * W * R, "n0-1": lambda W: 2 * W * R - 1, "n0-2": lambda W: 2 * W * R - 2,
    "n0+1": lambda W: 2 * W * R + 1, "n0+2": lambda W: 2 * W * R + 2,
    "window short": lambda W: 2 * W * R - 2 * 16 * R,
    "pass short": lambda W: 2 * W * R - 2 * 64,
    "remainder 2, odd": lambda W: 2 * (W * (R + 1) + 8) - 1,
    "remainder 3, odd": lambda W: 2 * (W * (R + 2) + 8) + 1,
    "below the rounds": lambda W: 2 * W * R - 2 * W,
}
TAIL = {"2W37": lambda W: 2 * W * 37, "2W37-3": lambda W: 2 * W * 37 - 3}


@pytest.fixture(scope="module")
def world():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    from memcached_amd import crc32c as mc
    assert mc.gpu_count() >= 1, "libmcrc32c.so sees no gfx950 device"
    assert m.rounds_min_steps() == R
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    W = 16 * cus
    nmax, nside = 2 * W * 40, 2 * W * R + 2
    rng = np.random.default_rng(33)
    host = rng.integers(0, 256, max(nmax * 4096, nside * WIDE) + OFF16, dtype=np.uint8)
    cin = rng.integers(0, 2**32, nmax, dtype=np.uint64).astype(np.uint32)
    offs = np.arange(nmax, dtype=np.uint64) * 4096
    want = {(4096, 0, c is not None): oracle.batch(host, offs, np.full(nmax, 4096), c) for c in (None, cin)}
    side = np.arange(nside, dtype=np.uint64)
    want[WIDE, 0, True] = oracle.batch(host, side * WIDE, np.full(nside, 4096), cin[:nside])
    want[4096, OFF16, False] = oracle.batch(host, side * 4096 + OFF16, np.full(nside, 4096), None)
    dev = torch.from_numpy(host).cuda()
    dcin = torch.from_numpy(cin.view(np.int32)).cuda()
    assert dev.data_ptr() % 128 == 0
    prev = _lib.lib.crc32c_set_k1_tail_min(NEVER)
    yield dict(cus=cus, W=W, T0=t.consts()["floor"], nmax=nmax, dev=dev, dcin=dcin, want=want, torch=torch)
    _lib.lib.crc32c_set_k1_tail_min(prev)


def _launch(w, n, stride, off, with_cin, out, flags=_lib.CRC32C_DEVICE, stream=None):
    s = _lib.Spans(w["dev"].data_ptr() + off, (n - 1) * stride + 4096, None, stride, None, 4096,
                   w["dcin"].data_ptr() if with_cin else None, out.data_ptr(), n)
    _lib.check(_lib.lib.crc32c_batch(ctypes.byref(s), flags, stream))


def _check(w, n, stride, off, with_cin, out, what):
    got = out[:n].cpu().numpy().view(np.uint32)
    np.testing.assert_array_equal(got, w["want"][stride, off, with_cin][:n], err_msg=f"{what} n {n} stride {stride} + {off}")
    assert int(out[n]) == SENTINEL, f"{what}: written past the batch"


def _new_out(w, n):
    return w["torch"].full((n + 1,), SENTINEL, dtype=w["torch"].int32, device="cuda")


def _tail_min(w, steps):
    """Sets the tail's threshold for a with block's launches; the module's (never) afterwards."""
    class _Ctx:
        def __enter__(self):
            _lib.lib.crc32c_set_k1_tail_min(steps)

        def __exit__(self, *a):
            _lib.lib.crc32c_set_k1_tail_min(NEVER)
    return _Ctx()


def test_cases_reach_the_paths_they_name(world):
    W, cus, T0 = world["W"], world["cus"], world["T0"]
    geo = {k: t.geometry(f(W), cus) for k, f in STATIC.items()}
    assert all(g[0] == W for g in geo.values())
    cg = {k: g[2] for k, g in geo.items()}
    for k in ("n0", "n0-1", "n0-2", "window short", "pass short"):
        assert cg[k] == R, k
    assert cg["n0+1"] == cg["n0+2"] == R + 1 and cg["remainder 2, odd"] == R + 2 and cg["remainder 3, odd"] == R + 3
    assert STATIC["remainder 2, odd"](W) % 2 and STATIC["remainder 3, odd"](W) % 2
    assert geo["window short"][1] == W * R - 16 * R and geo["pass short"][1] == W * R - 64
    for k in STATIC:
        want = o.RANGES if k == "below the rounds" else o.WINDOW_PASS
        assert o.order_for(o.WINDOW_PASS, cg[k]) == want and not t.tail_on(STATIC[k](W), cus, t.consts()["default_min"]), k
    assert cg["below the rounds"] == R - 1 and m.library_rounds([R - 1])[1][0] == 0
    for k, f in TAIL.items():
        Wk, ngroups, c = t.geometry(f(W), cus)
        (cg_s, pool0, nchunks, _), = t.library_splits([(ngroups, Wk)])
        assert t.tail_on(f(W), cus, T0) and c == 37 and cg_s == R and nchunks > 0, k
    (cg_s, _, _, _), = t.library_splits([(W * 40, W)])
    assert t.tail_on(2 * W * 40, cus, t.consts()["default_min"]) and cg_s == R
    assert max(f(W) for f in list(STATIC.values()) + list(TAIL.values())) <= world["nmax"] == 2 * W * 40


@pytest.mark.parametrize("case", list(STATIC))
def test_windows_without_the_tail(world, case):
    w = world
    n = STATIC[case](w["W"])
    out = _new_out(w, n)
    for with_cin in (False, True):
        out.fill_(SENTINEL)
        _launch(w, n, 4096, 0, with_cin, out)
        _check(w, n, 4096, 0, with_cin, out, case)


@pytest.mark.parametrize("case", list(TAIL))
def test_windows_with_the_tail_at_its_floor(world, case):
    w = world
    n = TAIL[case](w["W"])
    out = _new_out(w, n)
    with _tail_min(w, w["T0"]):
        for with_cin in (False, True):
            out.fill_(SENTINEL)
            _launch(w, n, 4096, 0, with_cin, out)
            _check(w, n, 4096, 0, with_cin, out, case)


def test_windows_and_tail_by_default(world):
    w = world
    n = 2 * w["W"] * 40
    out = _new_out(w, n)
    with _tail_min(w, t.consts()["default_min"]):
        _launch(w, n, 4096, 0, True, out)
    _check(w, n, 4096, 0, True, out, "2W40")


def test_wide_stride(world):
    """Stride 4224: whole lines still (the non-temporal kernel), windows of 33 lines per item."""
    w = world
    n = 2 * w["W"] * R + 1
    out = _new_out(w, n)
    _launch(w, n, WIDE, 0, True, out)
    _check(w, n, WIDE, 0, True, out, "stride 4224")


def test_base_off_a_line(world):
    """A base 16 B past a line: the default-policy kernel; neighbouring waves share a line per 32 KiB."""
    w = world
    n = 2 * w["W"] * R + 2
    out = _new_out(w, n)
    _launch(w, n, 4096, OFF16, False, out)
    _check(w, n, 4096, OFF16, False, out, "base + 16")


def test_back_to_back_launches_on_one_stream(world):
    """Two asynchronous launches, no sync between them: windows with the tail, then windows without it (a remainder)."""
    w = world
    torch = w["torch"]
    st = torch.cuda.Stream()
    ns = [TAIL["2W37-3"](w["W"]), STATIC["remainder 3, odd"](w["W"])]
    outs = [_new_out(w, n) for n in ns]
    torch.cuda.synchronize()
    with _tail_min(w, 37):
        for n, out in zip(ns, outs):
            _launch(w, n, 4096, 0, False, out, _lib.CRC32C_DEVICE | _lib.CRC32C_ASYNC, ctypes.c_void_p(st.cuda_stream))
        st.synchronize()
    for n, out in zip(ns, outs):
        _check(w, n, 4096, 0, False, out, "back to back")

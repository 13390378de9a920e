"""K1's lockstep rounds on the GPU: at the item counts where a wave's barrier
count can go wrong, every CRC is checked against the CPU oracle, with and
without crc_in, at stride 4096 (the non-temporal instantiations) and 4112 (the
default-policy ones).

With W = 16 x CUs waves, S = kK1RoundSteps, M = kK1RoundsMinSteps (launches of
fewer steps per wave run without rounds) and cg = the steps of a full range:
  1 .. 65                one to three workgroups, most waves with an empty range
                         (they only pay the barriers they owe)
  2 W c, c = S-1, S,     rounds one step short, exactly full, one over, and the
  S+1, 2S, 2S+1          same at two rounds (below M: launches that must not
                         meet at all, whatever S divides)
  2 W (S+1) - W - 3      some waves a step shorter than others; the last range
                         cut, ending in an odd item
  2 W S + 5              cg = S + 1 with almost every wave ending far below it
  2 W c, c = M-1, M,     the last launch without rounds, the first with them,
  M+1                    and one step over
  2 W M - W - 3,         the two shapes above where the rounds run: cut ranges
  2 W M + 5              and empty ones make up arrivals
A miscounted barrier shows as a hang, not as a wrong CRC, so this module runs
first and alone under a short time limit (tools/gpu_suite.sh).  The data and
the oracle's CRCs are computed once for the largest case: item i at a given
stride is the same bytes in every case."""
import ctypes

import numpy as np
import pytest

try:  # GPU processes load torch (and its HIP runtime) before libmcrc32c.so
    import torch as _torch  # noqa: F401
except ImportError:
    pass

from memcached_amd import _lib
from memcached_amd import crc32c as mc

from . import k1_rounds_model as m
from . import oracle

pytestmark = pytest.mark.gpu
STRIDES = (4096, 4112)

CASES = {
    "1": lambda W, S, M: 1, "2": lambda W, S, M: 2, "3": lambda W, S, M: 3, "31": lambda W, S, M: 31,
    "32": lambda W, S, M: 32, "33": lambda W, S, M: 33, "65": lambda W, S, M: 65,
    "2W(S-1)": lambda W, S, M: 2 * W * (S - 1), "2WS": lambda W, S, M: 2 * W * S,
    "2W(S+1)": lambda W, S, M: 2 * W * (S + 1),
    "2W2S": lambda W, S, M: 2 * W * 2 * S, "2W(2S+1)": lambda W, S, M: 2 * W * (2 * S + 1),
    "2W(S+1)-W-3": lambda W, S, M: 2 * W * (S + 1) - W - 3,
    "2WS+5": lambda W, S, M: 2 * W * S + 5,
    "2W(M-1)": lambda W, S, M: 2 * W * (M - 1), "2WM": lambda W, S, M: 2 * W * M,
    "2W(M+1)": lambda W, S, M: 2 * W * (M + 1),
    "2WM-W-3": lambda W, S, M: 2 * W * M - W - 3, "2WM+5": lambda W, S, M: 2 * W * M + 5,
}


@pytest.fixture(scope="module")
def world():
    """W, S, the bytes on the host and the device, crc_in, and the oracle's
    CRCs per (stride, with crc_in) at the largest item count."""
    import torch
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    assert mc.gpu_count() >= 1, "libmcrc32c.so sees no gfx950 device"
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    W, S, M = 16 * cus, m.round_steps(), m.rounds_min_steps()
    nmax = max(f(W, S, M) for f in CASES.values())
    rng = np.random.default_rng(20)
    host = rng.integers(0, 256, nmax * max(STRIDES), dtype=np.uint8)
    cin = rng.integers(0, 2**32, nmax, dtype=np.uint64).astype(np.uint32)
    want = {}
    for stride in STRIDES:
        offs = np.arange(nmax, dtype=np.uint64) * stride
        for c in (None, cin):
            want[stride, c is not None] = oracle.batch(host, offs, np.full(nmax, 4096), c)
    dev = torch.from_numpy(host).cuda()
    dcin = torch.from_numpy(cin.view(np.int32)).cuda()
    out = torch.empty(nmax, dtype=torch.int32, device="cuda")
    return dict(cus=cus, W=W, S=S, M=M, dev=dev, dcin=dcin, out=out, want=want, torch=torch)


@pytest.mark.parametrize("case", list(CASES))
def test_k1_lockstep_counts(world, case):
    w = world
    n = CASES[case](w["W"], w["S"], w["M"])
    cg, ranges = m.split(n, w["cus"])
    for stride in STRIDES:
        for with_cin in (False, True):
            w["out"].fill_(0x5a5a5a5a)
            s = _lib.Spans(w["dev"].data_ptr(), n * stride, None, stride, None, 4096,
                           w["dcin"].data_ptr() if with_cin else None, w["out"].data_ptr(), n)
            _lib.check(_lib.lib.crc32c_batch(ctypes.byref(s), _lib.CRC32C_DEVICE, None))
            got = w["out"][:n].cpu().numpy().view(np.uint32)
            np.testing.assert_array_equal(got, w["want"][stride, with_cin][:n], err_msg=f"{case} n {n} cg {cg} stride {stride}")
            # nothing is written past the batch
            if n < w["out"].numel():
                assert int(w["out"][n]) == 0x5a5a5a5a


def test_cases_reach_the_paths_they_name(world):
    """The model's walk of the same splits: the list does hold launches with
    empty ranges, launches just below and at the length where rounds start,
    full rounds, and cut and empty ranges that make up arrivals."""
    W, S, M, cus = world["W"], world["S"], world["M"], world["cus"]
    _, rounds = m.library_rounds([m.split(f(W, S, M), cus)[0] for f in CASES.values()])
    seen = {}
    for (name, f), r in zip(CASES.items(), rounds):
        n = f(W, S, M)
        cg, ranges = m.split(n, cus)
        ngroups = (n + 1) // 2
        walks = [m.walk(g0, g1, ngroups, cg, S, r) for g0, g1 in ranges]
        assert all(a + b == r and (a == p if r else a == 0) for a, b, p, _ in walks)
        seen[name] = (cg, r, sum(1 for g0, _ in ranges if g0 >= ngroups), sum(1 for _, b, _, _ in walks if b))
    on = lambda cg: cg // S if cg >= M else 0
    for name, cg in (("2W(S-1)", S - 1), ("2WS", S), ("2W(S+1)", S + 1), ("2W2S", 2 * S), ("2W(2S+1)", 2 * S + 1),
                     ("2W(M-1)", M - 1), ("2WM", M), ("2W(M+1)", M + 1)):
        assert seen[name][:2] == (cg, on(cg)), name
    assert seen["2W(M-1)"][1] == 0 and seen["2WM"][1] == M // S > 0
    assert seen["2WS+5"][0] == S + 1 and seen["2W(S+1)-W-3"][0] == S + 1
    # where the rounds run: waves that make up arrivals, cut ranges and empty ones
    assert seen["2WM+5"][:2] == (M + 1, on(M + 1)) and seen["2WM+5"][2] > 0 and seen["2WM+5"][3] > 0
    assert seen["2WM-W-3"][:2] == (M, on(M)) and seen["2WM-W-3"][3] > 0
    assert seen["65"][2] > 0 and seen["1"][1] == 0

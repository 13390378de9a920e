"""The host shim's decisions (memcached_amd/csrc/host_route.h: which kernels a
batch goes to, the launch geometry, the plan's rounds and capacity, the host
pipeline's staging order and chunk cuts, the shard cuts), checked on the CPU:
tests/integration/host_route_check.cpp compiles the header as plain C++ under
the address and undefined-behaviour sanitizers and asserts every boundary; this
module recomputes from the Python models what the program prints."""
import os
import subprocess

import numpy as np
import pytest

from memcached_amd import shard
from tests import span_model
from tests.test_items_lines_model import lines_shape

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("host_route") / "host_route_check")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-I", os.path.join(ROOT, "memcached_amd", "csrc"),
                    os.path.join(HERE, "integration", "host_route_check.cpp"), "-o", out], check=True)
    return out


def test_host_route_decisions(exe):
    """Every assertion of the program (routes of fixed-length, small and item
    batches, geometry, pipeline cuts), and its two fixed-length sets against
    the models: K5 takes the lengths that lines_shape calls fused at all 128
    alignments, k_blocks those that one_block calls one block (with a unit)
    at all 128."""
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "host_route ok" in r.stdout
    sets = {line.split()[0]: [int(x) for x in line.split()[1:]] for line in r.stdout.splitlines()[:2]}
    k5 = [n for n in range(9001) if n >= 4 and all(lines_shape(al, n)[2] for al in range(128))]
    blocks = [n for n in range(9001)
              if all(span_model.one_block(al, n)[0] and not span_model.one_block(al, n)[1] for al in range(128))]
    assert k5 == list(range(4099, 4228)) and sets["k5"] == k5
    # (K5 is tested first; its lengths and k_blocks' are disjoint anyway)
    assert blocks == list(range(4081, 4098)) and sets["blocks"] == blocks


def test_chain_cases_take_the_routes_they_name(exe):
    """tests/chain_cases.py labels every case with the span route its iovs take
    in a device call (the base 16-B aligned, as device allocations are):
    span_route's own answer for each, so test_gpu_chains.py does run the fold
    behind K1, K5, k_blocks, k_spans, k_final, k_small and the planned path."""
    from tests import chain_cases as cc
    cases = cc.small_cases() + [cc.million_case()]
    for c in cases:
        args = [c.n, c.length, c.stride, int(c.offsets is not None), int(c.lens is not None), 0, c.buf.size,
                8192 if c.small_max is None else c.small_max]
        r = subprocess.run([exe, "route"] + [str(a) for a in args], capture_output=True, text=True, timeout=60)
        assert r.returncode == 0 and r.stdout.strip() == c.route, (c.name, r.stdout, r.stderr)
    assert {c.route for c in cases} == {"k1", "small", "k5", "id_blocks", "id_spans", "id_final", "planned"}


def _route(exe, n, length, stride, has_lens, base_mod, base_bytes, small_max):
    """span_route's answer for a batch without offsets[], by the program's `route` mode."""
    args = [n, length, stride, 0, int(has_lens), base_mod, base_bytes, 8192 if small_max is None else small_max]
    r = subprocess.run([exe, "route"] + [str(a) for a in args], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, (args, r.stdout, r.stderr)
    return r.stdout.strip()


def test_stride_cases_take_the_routes_they_name(exe):
    """tests/stride_cases.py labels every fixed-stride case with its span route:
    span_route's own answer for each, at the three base residues
    tests/test_gpu_strides.py places it at (no case has K1's shape, so the base
    decides nothing).  And the 2^31 line: 4096-byte spans at a stride of
    2^31 - 16 are K1's, at 2^31 k_blocks'."""
    from tests import stride_cases as sc
    for c in sc.cases():
        for base_mod in (0, 1, 127):
            got = _route(exe, c.n, c.length, c.stride, c.lens is not None, base_mod, c.nbytes, c.small_max)
            assert got == c.route, (c.name, base_mod, got)
    assert {c.route for c in sc.cases()} == set(sc.ROUTES) == {"small", "k5", "id_blocks", "id_spans", "id_final",
                                                                "planned"}
    # every length and size the cases are there for
    have = {(c.route, c.length) for c in sc.cases() if c.lens is None}
    assert {(r, L) for r, (lengths, _) in sc.FIXED.items() for L in lengths} <= have
    assert {c.n for c in sc.cases() if c.route == "k5"} >= {1, 63, 64, 65, 131, 8193}
    assert any(c.length == 4096 and c.stride % 16 for c in sc.cases() if c.route == "id_blocks")
    assert {(c.route, c.stride >= int(c.lens.max())) for c in sc.cases() if c.lens is not None} == {
        ("planned", True), ("planned", False), ("small", False)}
    assert {c.route for c in sc.cases() if c.host} == set(sc.ROUTES)
    for length, stride, route in sc.LINE_CASES:
        size = (sc.LINE_N - 1) * stride + length
        assert _route(exe, sc.LINE_N, length, stride, False, 0, size, 0) == route, (length, stride)
        assert (sc.LINE_N - 1) * stride >= 1 << 32 or route == "k1"
    assert ((4096, sc.LINE - 16, "k1") in sc.LINE_CASES and (4096, sc.LINE, "id_blocks") in sc.LINE_CASES)


def test_stride_case_buffers_are_the_smallest_accepted(exe):
    """Every case's buffer is exactly (n - 1) * stride + len bytes: with one
    byte less fixed_spans_fit refuses the descriptor (span_route: invalid, which
    crc32c_batch returns as CRC32C_EINVAL).  With lens[] the spans are checked
    on the device, and the buffer ends where the last span does."""
    from tests import stride_cases as sc
    for c in sc.cases():
        assert c.buf.size == c.nbytes
        if c.lens is None:
            assert c.nbytes == (c.n - 1) * c.stride + c.length
            if c.nbytes:
                got = _route(exe, c.n, c.length, c.stride, False, 0, c.nbytes - 1, c.small_max)
                assert got == "invalid", (c.name, got)
        else:
            ends = c.offsets().astype(np.int64) + c.lens.astype(np.int64)
            assert c.nbytes == ends.max() and c.length == sc.DECOY_LEN
    for length, stride, _ in sc.LINE_CASES:
        size = (sc.LINE_N - 1) * stride + length
        assert _route(exe, sc.LINE_N, length, stride, False, 0, size - 1, 0) == "invalid"


@pytest.mark.parametrize("parts", range(1, 9))
def test_shard_cuts_match_plan(exe, parts):
    """crc32c_shard_cuts' body against memcached_amd/shard.py plan() on the
    same lengths: Zipf-like, equal, empty, zeros and one dominant span."""
    rng = np.random.default_rng(parts)
    cases = [rng.zipf(1.3, 1000).clip(1, 1 << 20), np.full(1000, 4096), np.zeros(0, dtype=np.int64),
             np.zeros(7, dtype=np.int64), np.array([5, 0, 0, 1 << 30, 3, 3]), rng.integers(0, 1 << 32, 257)]
    for lens in cases:
        r = subprocess.run([exe, "cuts", str(parts)], input=" ".join(str(int(x)) for x in lens),
                           capture_output=True, text=True, timeout=60)
        assert r.returncode == 0, r.stdout + r.stderr
        assert [int(x) for x in r.stdout.split()] == list(shard.plan(lens, parts))

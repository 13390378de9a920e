"""The pointer batches' host decisions (memcached_amd/csrc/host_route.h:
ptr_route, the pack plan) on the CPU: tests/integration/ptr_pack_check.cpp
compiles the header as plain C++ under the address and undefined-behaviour
sanitizers, packs spans that are each their own exact-size malloc, and asserts
every boundary."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("ptr_pack") / "ptr_pack_check")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-I", os.path.join(ROOT, "memcached_amd", "csrc"),
                    os.path.join(HERE, "integration", "ptr_pack_check.cpp"), "-o", out], check=True)
    return out


def test_ptr_route_and_pack_plan(exe):
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ptr_pack ok" in r.stdout


def test_the_shim_packs_with_the_plan_that_is_checked():
    """The host shim calls the functions the program checks, and only span bytes are copied."""
    src = open(os.path.join(ROOT, "memcached_amd", "csrc", "shim_ptrs.h")).read()
    assert "mcrc::pack_chunk(b, k0, pos)" in src and "mcrc::pack_copy(b, k0, ch.k1, pos" in src
    assert "mcrc::ptr_route(" in src and "mcrc::ptr_span_route(" in src and "mcrc::ptr_spans_ok(b)" in src

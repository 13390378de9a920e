"""tests/integration/ptrs_sim.c: the proxy's read path -- a malloc'ed buffer per
read, verified through crc32c_ptrs_submit by several IO threads -- once with
the buffers as malloc returns them (every job runs alone, packed) and once with
buffers from a registered 1 MiB page per thread (the jobs share launches).
Every CRC equals the host crc32c()'s and the torn reads are the only
mismatches with the stored CRC (both are failures of the run inside the sim).
Without a GPU the submit reports CRC32C_ENODEV and writes nothing."""
import re

import pytest

from .test_integration import _build_c, _run_sim

FIELDS = ("reads", "mismatches", "torn", "detected", "false_bad", "rc_fail", "launches", "coalesced_jobs", "solo_jobs")


@pytest.fixture(scope="module")
def ptrs_exe(tmp_path_factory):
    return _build_c(tmp_path_factory, "ptrs_sim")


def test_ptrs_sim_without_gpu(ptrs_exe):
    assert "no gfx950 device" in _run_sim(ptrs_exe)


@pytest.mark.gpu
def test_ptrs_sim_verifies_every_read_on_both_legs(ptrs_exe):
    out = _run_sim(ptrs_exe, "8", "100", "4", gpu=True)
    assert "ptrs_sim ok" in out
    legs = {}
    for leg in ("malloc", "registered"):
        m = re.search(f"^leg={leg} " + " ".join(f"{f}=(\\d+)" for f in FIELDS) + "$", out, re.M)
        assert m, out
        legs[leg] = dict(zip(FIELDS, map(int, m.groups())))
    for f in legs.values():
        assert f["reads"] == 8 * 100 * 4 and f["mismatches"] == f["false_bad"] == f["rc_fail"] == 0
        assert f["detected"] == f["torn"] > 0
    assert legs["malloc"]["solo_jobs"] == 800 and legs["malloc"]["coalesced_jobs"] == 0
    assert legs["registered"]["coalesced_jobs"] == 800 and legs["registered"]["solo_jobs"] == 0
    assert 1 <= legs["registered"]["launches"] <= 800

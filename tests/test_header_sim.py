"""tests/integration/header_sim.c: recover_sim.c's read-back of a page whose
headers were damaged on flash, with single length bits and data bits flipped
inside other live images as well, played through crc32c_recover_pages, rounds
of crc32c_repair_headers with the page walked again, and crc32c_repair_items.
At the end the page loses exactly what the sim's own count from the pristine
bytes and its own layout says no rule can fix."""
import pytest

from .test_integration import _build_c, _run_sim, _sim_fields

FIELDS = ("live", "lost_recover", "lost_headers", "lost_items", "headers_repaired", "items_repaired", "rounds",
          "unrepairable", "multi", "behind")


@pytest.fixture(scope="module")
def header_exe(tmp_path_factory):
    return _build_c(tmp_path_factory, "header_sim")


def test_header_sim_without_gpu(header_exe):
    assert "no gfx950 device" in _run_sim(header_exe)


@pytest.mark.gpu
def test_header_sim_loses_only_what_no_rule_can_fix(header_exe):
    f = _sim_fields(_run_sim(header_exe, gpu=True), FIELDS)
    assert f["lost_items"] == f["unrepairable"] == f["multi"] + f["behind"]
    assert f["lost_items"] < f["lost_headers"] < f["lost_recover"]
    assert f["headers_repaired"] > 0 and f["items_repaired"] > 0 and f["rounds"] >= 1
    assert f["multi"] > 0 and f["behind"] > 0

"""tests/integration/repair_sim.c: recover_sim.c's read-back of a page whose
headers were damaged on flash, with bits flipped inside live images as well,
played three ways over the same bytes: the reference's walk, the one call
crc32c_recover_pages, and that call followed by crc32c_repair_items over its
bad sane entries.  With the repair the page loses exactly what the sim's own
CPU search says the rule cannot fix."""
import pytest

from .test_integration import _build_c, _run_sim, _sim_fields

FIELDS = ("live", "lost_reference", "lost_recover", "lost_repair", "repaired", "unrepairable", "length", "multi",
          "unlisted")


@pytest.fixture(scope="module")
def repair_exe(tmp_path_factory):
    return _build_c(tmp_path_factory, "repair_sim")


def test_repair_sim_without_gpu(repair_exe):
    assert "no gfx950 device" in _run_sim(repair_exe)


@pytest.mark.gpu
def test_repair_sim_loses_only_what_the_rule_cannot_fix(repair_exe):
    f = _sim_fields(_run_sim(repair_exe, gpu=True), FIELDS)
    assert f["lost_repair"] == f["unrepairable"] == f["length"] + f["multi"] + f["unlisted"]
    assert f["lost_repair"] < f["lost_recover"] < f["lost_reference"]
    assert f["repaired"] == f["lost_recover"] - f["lost_repair"] > 0
    assert f["length"] > 0 and f["multi"] > 0

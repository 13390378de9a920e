"""tests/integration/triage_sim.c: header_sim.c's damaged page played through
its old flow (crc32c_recover_pages, crc32c_repair_headers, crc32c_repair_items)
and through the new one, crc32c_triage_pages in crc32c_recover_pages' place and
the filtered suspects added to the repair list.  At the end the new flow loses
exactly what the sim's own count from the pristine bytes and its own layout
says no rule can fix now, and fewer than the old flow lost in the same run."""
import pytest

from .test_integration import _build_c, _run_sim, _sim_fields

FIELDS = ("live", "lost_old", "lost_recover", "lost_headers", "lost_triage", "headers_repaired", "items_repaired",
          "suspects", "suspects_kept", "rounds", "unrepairable", "multi", "behind_length", "behind_crlf")


@pytest.fixture(scope="module")
def triage_exe(tmp_path_factory):
    return _build_c(tmp_path_factory, "triage_sim")


def test_triage_sim_without_gpu(triage_exe):
    assert "no gfx950 device" in _run_sim(triage_exe)


@pytest.mark.gpu
def test_triage_sim_loses_only_what_no_rule_can_fix(triage_exe):
    f = _sim_fields(_run_sim(triage_exe, gpu=True), FIELDS)
    assert f["lost_triage"] == f["unrepairable"] == f["multi"] + f["behind_length"] + f["behind_crlf"]
    assert f["lost_triage"] < f["lost_old"]
    assert f["lost_triage"] < f["lost_headers"] < f["lost_recover"]
    assert 0 < f["suspects_kept"] <= f["suspects"] and f["items_repaired"] > 0 and f["headers_repaired"] > 0
    assert f["multi"] > 0 and f["behind_length"] > 0

"""tests/integration/scrub_sim.c: triage_sim.c's damaged page played through
that sim's host loop over the three calls and through one crc32c_scrub_pages.
The scrub loses exactly what the sim's own count from the pristine bytes and
its own layout says no rule can fix, which is what the written-out flow loses
in the same run; every rescued image equals its pristine bytes from byte 28 and
the log replayed on the damaged bytes gives the page (both are failures of the
run inside the sim).  Without a GPU the call reports CRC32C_ENODEV and writes
nothing, not one word of its struct."""
import pytest

from .test_integration import _build_c, _run_sim, _sim_fields

FIELDS = ("live", "lost_written_out", "lost_scrub", "calls_written_out", "headers_repaired", "items_repaired", "rounds",
          "nflips", "complete", "unrepairable", "multi", "behind_length", "behind_crlf")


@pytest.fixture(scope="module")
def scrub_exe(tmp_path_factory):
    return _build_c(tmp_path_factory, "scrub_sim")


def test_scrub_sim_without_gpu(scrub_exe):
    assert "no gfx950 device" in _run_sim(scrub_exe)


@pytest.mark.gpu
def test_scrub_sim_loses_only_what_no_rule_can_fix(scrub_exe):
    f = _sim_fields(_run_sim(scrub_exe, gpu=True), FIELDS)
    assert f["lost_scrub"] == f["unrepairable"] == f["multi"] + f["behind_length"] + f["behind_crlf"]
    assert f["lost_scrub"] == f["lost_written_out"]
    assert f["complete"] == 1 and f["nflips"] == f["headers_repaired"] + f["items_repaired"]
    assert f["headers_repaired"] > 0 and f["items_repaired"] > 0 and f["rounds"] >= 2
    assert f["calls_written_out"] > f["rounds"] and f["multi"] > 0 and f["behind_length"] > 0

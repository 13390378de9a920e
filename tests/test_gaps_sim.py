"""tests/integration/gaps_sim.c: scrub_sim.c's damaged page through one
crc32c_scrub_pages without CRC32C_SCRUB_GAPS and one with it, in one run.  With
the bit the scrub loses exactly what the sim's own count from the pristine
bytes and its own layout says the rule cannot fix -- two or more flipped bits,
a dead header, or a single length or CRLF bit behind the first dead header
with a lost image in front -- which is fewer than without it, and without it
loses what scrub_sim.c reports.  Every rescued image equals its pristine bytes
from byte 28 and the log replayed on the damaged bytes gives the page (both
are failures of the run inside the sim).  Without a GPU the call reports
CRC32C_ENODEV and writes nothing."""
import pytest

from .test_integration import _build_c, _run_sim, _sim_fields
from .test_scrub_sim import FIELDS as SCRUB_FIELDS

FIELDS = ("live", "lost_scrub", "unrepairable_scrub", "lost_gaps", "unrepairable_gaps", "multi", "dead", "behind_lost",
          "rounds_scrub", "rounds_gaps", "headers_repaired", "items_repaired", "nflips", "complete")


@pytest.fixture(scope="module")
def gaps_exe(tmp_path_factory):
    return _build_c(tmp_path_factory, "gaps_sim")


@pytest.fixture(scope="module")
def scrub_exe(tmp_path_factory):
    return _build_c(tmp_path_factory, "scrub_sim")


def test_gaps_sim_without_gpu(gaps_exe):
    assert "no gfx950 device" in _run_sim(gaps_exe)


@pytest.mark.gpu
def test_gaps_sim_loses_only_what_the_rule_cannot_fix(gaps_exe, scrub_exe):
    f = _sim_fields(_run_sim(gaps_exe, gpu=True), FIELDS)
    assert f["lost_gaps"] == f["unrepairable_gaps"] == f["multi"] + f["dead"] + f["behind_lost"]
    assert f["lost_gaps"] < f["lost_scrub"] == f["unrepairable_scrub"]
    assert f["complete"] == 1 and f["nflips"] == f["headers_repaired"] + f["items_repaired"]
    assert f["rounds_gaps"] >= 2 and f["rounds_scrub"] >= 2
    assert f["behind_lost"] < f["lost_scrub"] - f["multi"] - f["dead"]
    assert _sim_fields(_run_sim(scrub_exe, gpu=True), SCRUB_FIELDS)["lost_scrub"] == f["lost_scrub"]

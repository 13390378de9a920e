"""tests/integration/bytes_sim.c: repair_sim.c's read-back of a page whose
headers and data were damaged on flash, its multi-bit hits split into two bits
of one byte and bits of two bytes, played three ways over the same bytes: the
reference's walk, the one call crc32c_recover_pages, and that call followed by
crc32c_repair_bytes over its bad sane entries.  With the byte rule the page
loses exactly what the sim's own CPU search says the rule cannot fix."""
import pytest

from .test_integration import _build_c, _run_sim, _sim_fields

FIELDS = ("live", "lost_reference", "lost_recover", "lost_bytes", "repaired", "samebyte", "unrepairable", "length",
          "twobyte", "unlisted")


@pytest.fixture(scope="module")
def bytes_exe(tmp_path_factory):
    return _build_c(tmp_path_factory, "bytes_sim")


def test_bytes_sim_without_gpu(bytes_exe):
    assert "no gfx950 device" in _run_sim(bytes_exe)


@pytest.mark.gpu
def test_bytes_sim_loses_only_what_the_rule_cannot_fix(bytes_exe):
    f = _sim_fields(_run_sim(bytes_exe, gpu=True), FIELDS)
    assert f["lost_bytes"] == f["unrepairable"] == f["length"] + f["twobyte"] + f["unlisted"]
    assert f["lost_bytes"] < f["lost_recover"] < f["lost_reference"]
    assert f["repaired"] == f["lost_recover"] - f["lost_bytes"] > 0
    assert f["length"] > 0 and f["twobyte"] > 0 and f["samebyte"] > 0

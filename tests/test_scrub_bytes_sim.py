"""tests/integration/scrub_bytes_sim.c: bytes_sim.c's damaged page (every tenth
data-damaged image with two bits of one byte inverted) through one
crc32c_scrub_pages with CRC32C_SCRUB_GAPS and one with CRC32C_SCRUB_GAPS |
CRC32C_SCRUB_BYTES, in one run.  No count is fixed in advance: every image the
second run logs CRC32C_SCRUB_BY_BYTE equals its pristine bytes, every one-byte
image the first run's final list names for the item stage is rescued by the
second, the second loses no image the first rescued, and it loses fewer.  The
log replayed on the damaged bytes gives the page and items_repaired is the item
stage's entries plus the byte stage's images (failures of the run inside the
sim).  Without a GPU the call reports CRC32C_ENODEV and writes nothing."""
import pytest

from .test_integration import _build_c, _run_sim, _sim_fields

FIELDS = ("live", "lost_gaps", "lost_bytes", "rounds_gaps", "rounds_bytes", "by_byte", "by_byte_wrong", "named",
          "named_rescued", "regressed", "nflips", "items_repaired", "samebyte")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return _build_c(tmp_path_factory, "scrub_bytes_sim")


def test_scrub_bytes_sim_without_gpu(exe):
    assert "no gfx950 device" in _run_sim(exe)


@pytest.mark.gpu
def test_scrub_bytes_sim_brings_back_the_one_byte_images(exe):
    f = _sim_fields(_run_sim(exe, gpu=True), FIELDS)
    assert f["by_byte"] > 0 and f["by_byte_wrong"] == 0
    assert f["named"] > 0 and f["named_rescued"] == f["named"]
    assert f["regressed"] == 0
    assert f["lost_bytes"] < f["lost_gaps"]
    assert f["rounds_bytes"] > f["rounds_gaps"] >= 1

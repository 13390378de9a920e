"""tests/integration/recover_sim.c: salvage_sim.c's read-back of a page whose
headers were damaged on flash, through the one call crc32c_recover_pages and a
single rescue loop over its merged list.  It loses only the images whose own
header was hit, and reaches and salvages exactly what crc32c_verify_pages
followed by crc32c_salvage_pages does."""
import pytest

from .test_integration import _build_c, _run_sim
from .test_salvage_sim import _counts


@pytest.fixture(scope="module")
def recover_exe(tmp_path_factory):
    return _build_c(tmp_path_factory, "recover_sim")


@pytest.fixture(scope="module")
def salvage_exe(tmp_path_factory):
    return _build_c(tmp_path_factory, "salvage_sim")


def test_recover_sim_without_gpu(recover_exe):
    assert "no gfx950 device" in _run_sim(recover_exe)


@pytest.mark.gpu
def test_recover_sim_loses_only_the_damaged_images(recover_exe, salvage_exe):
    f = _counts(_run_sim(recover_exe, gpu=True))
    assert f["lost"] == f["damaged"] > 0
    assert f["reached"] + f["salvaged"] + f["lost"] == f["live"]

    # the two-call flow on the same page and damage
    g = _counts(_run_sim(salvage_exe, gpu=True))
    assert (g["live"], g["damaged"]) == (f["live"], f["damaged"])
    assert (f["reached"], f["salvaged"]) == (g["reached"], g["salvaged"]) and f["salvaged"] > 0

"""tests/integration/salvage_sim.c: storage_compact_readback over a page whose
headers were damaged on flash.  The reference's walk loses every live image
packed behind a damaged header; crc32c_verify_pages followed by
crc32c_salvage_pages loses only the images whose own header was hit."""
import pytest

from .test_integration import _build_c, _run_sim, _sim_fields

FIELDS = ("live", "reached", "salvaged", "lost", "damaged")


@pytest.fixture(scope="module")
def salvage_exe(tmp_path_factory):
    return _build_c(tmp_path_factory, "salvage_sim")


def _counts(out):
    return _sim_fields(out, FIELDS)


def test_salvage_sim_without_gpu(salvage_exe):
    assert "no gfx950 device" in _run_sim(salvage_exe)


@pytest.mark.gpu
def test_salvage_sim_loses_only_the_damaged_images(salvage_exe):
    f = _counts(_run_sim(salvage_exe, gpu=True))
    assert f["lost"] == f["damaged"] > 0
    assert f["salvaged"] > 0 and f["reached"] + f["salvaged"] + f["lost"] == f["live"]

    # the reference's walk alone, on the same damage
    g = _counts(_run_sim(salvage_exe, "--walk", gpu=True))
    assert g["damaged"] == f["damaged"] and g["live"] == f["live"]
    assert g["lost"] > g["damaged"] and g["salvaged"] == 0
    assert g["reached"] == f["reached"]  # the walk is the same walk

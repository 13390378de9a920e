"""tests/integration/salvage_sim.c: storage_compact_readback over a page whose
headers were damaged on flash.  The reference's walk loses every live image
packed behind a damaged header; crc32c_verify_pages followed by
crc32c_salvage_pages loses only the images whose own header was hit."""
import re
import subprocess

import pytest

from .test_integration import _NOGPU, _build_c


@pytest.fixture(scope="module")
def salvage_exe(tmp_path_factory):
    return _build_c(tmp_path_factory, "salvage_sim")


def _counts(out):
    m = re.search(r"^live=(\d+) reached=(\d+) salvaged=(\d+) lost=(\d+) damaged=(\d+)$", out, re.M)
    assert m, out
    return dict(zip(("live", "reached", "salvaged", "lost", "damaged"), map(int, m.groups())))


def test_salvage_sim_without_gpu(salvage_exe):
    r = subprocess.run([salvage_exe], capture_output=True, text=True, env=_NOGPU, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "no gfx950 device" in r.stdout


@pytest.mark.gpu
def test_salvage_sim_loses_only_the_damaged_images(salvage_exe):
    r = subprocess.run([salvage_exe, "--gpu"], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    f = _counts(r.stdout)
    assert f["lost"] == f["damaged"] > 0
    assert f["salvaged"] > 0 and f["reached"] + f["salvaged"] + f["lost"] == f["live"]

    # the reference's walk alone, on the same damage
    r2 = subprocess.run([salvage_exe, "--gpu", "--walk"], capture_output=True, text=True, timeout=300)
    print(r2.stdout)
    assert r2.returncode == 0, r2.stdout + r2.stderr
    g = _counts(r2.stdout)
    assert g["damaged"] == f["damaged"] and g["live"] == f["live"]
    assert g["lost"] > g["damaged"] and g["salvaged"] == 0
    assert g["reached"] == f["reached"]  # the walk is the same walk

"""tests/integration/repair_sim.c: recover_sim.c's read-back of a page whose
headers were damaged on flash, with bits flipped inside live images as well,
played three ways over the same bytes: the reference's walk, the one call
crc32c_recover_pages, and that call followed by crc32c_repair_items over its
bad sane entries.  With the repair the page loses exactly what the sim's own
CPU search says the rule cannot fix."""
import re
import subprocess

import pytest

from .test_integration import _NOGPU, _build_c

FIELDS = ("live", "lost_reference", "lost_recover", "lost_repair", "repaired", "unrepairable", "length", "multi",
          "unlisted")


@pytest.fixture(scope="module")
def repair_exe(tmp_path_factory):
    return _build_c(tmp_path_factory, "repair_sim")


def test_repair_sim_without_gpu(repair_exe):
    r = subprocess.run([repair_exe], capture_output=True, text=True, env=_NOGPU, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "no gfx950 device" in r.stdout


@pytest.mark.gpu
def test_repair_sim_loses_only_what_the_rule_cannot_fix(repair_exe):
    r = subprocess.run([repair_exe, "--gpu"], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.search("^" + " ".join(f"{f}=(\\d+)" for f in FIELDS) + "$", r.stdout, re.M)
    assert m, r.stdout
    f = dict(zip(FIELDS, map(int, m.groups())))
    assert f["lost_repair"] == f["unrepairable"] == f["length"] + f["multi"] + f["unlisted"]
    assert f["lost_repair"] < f["lost_recover"] < f["lost_reference"]
    assert f["repaired"] == f["lost_recover"] - f["lost_repair"] > 0
    assert f["length"] > 0 and f["multi"] > 0

"""tests/integration/header_sim.c: recover_sim.c's read-back of a page whose
headers were damaged on flash, with single length bits and data bits flipped
inside other live images as well, played through crc32c_recover_pages, rounds
of crc32c_repair_headers with the page walked again, and crc32c_repair_items.
At the end the page loses exactly what the sim's own count from the pristine
bytes and its own layout says no rule can fix."""
import re
import subprocess

import pytest

from .test_integration import _NOGPU, _build_c

FIELDS = ("live", "lost_recover", "lost_headers", "lost_items", "headers_repaired", "items_repaired", "rounds",
          "unrepairable", "multi", "behind")


@pytest.fixture(scope="module")
def header_exe(tmp_path_factory):
    return _build_c(tmp_path_factory, "header_sim")


def test_header_sim_without_gpu(header_exe):
    r = subprocess.run([header_exe], capture_output=True, text=True, env=_NOGPU, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "no gfx950 device" in r.stdout


@pytest.mark.gpu
def test_header_sim_loses_only_what_no_rule_can_fix(header_exe):
    r = subprocess.run([header_exe, "--gpu"], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.search("^" + " ".join(f"{f}=(\\d+)" for f in FIELDS) + "$", r.stdout, re.M)
    assert m, r.stdout
    f = dict(zip(FIELDS, map(int, m.groups())))
    assert f["lost_items"] == f["unrepairable"] == f["multi"] + f["behind"]
    assert f["lost_items"] < f["lost_headers"] < f["lost_recover"]
    assert f["headers_repaired"] > 0 and f["items_repaired"] > 0 and f["rounds"] >= 1
    assert f["multi"] > 0 and f["behind"] > 0

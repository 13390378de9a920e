"""tests/integration/compact_sim.c: the device-walk stamp hook of INTEGRATION.md
section 2 under compaction.  Images rewritten verbatim with their stored CRC
keep it under CRC32C_KEEP_STAMPED, so a byte that flipped on flash before the
rewrite still fails the read-back compare; the plain stamp (--launder) gives
the damaged bytes a valid CRC."""
import os
import re
import subprocess

import pytest

from .test_integration import _NOGPU, _build_c


@pytest.fixture(scope="module")
def compact_exe(tmp_path_factory):
    return _build_c(tmp_path_factory, "compact_sim")


def _counts(out):
    m = re.search(r"^badcrc=(\d+) expected=(\d+) kept=(\d+) stamped=(\d+)$", out, re.M)
    assert m, out
    return dict(zip(("badcrc", "expected", "kept", "stamped"), map(int, m.groups())))


def test_compact_sim_without_gpu(compact_exe):
    r = subprocess.run([compact_exe], capture_output=True, text=True, env=_NOGPU, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "no gfx950 device" in r.stdout


@pytest.mark.gpu
def test_compact_sim_keeps_carried_crcs(compact_exe):
    r = subprocess.run([compact_exe, "--gpu"], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    f = _counts(r.stdout)
    assert f["badcrc"] == f["expected"] > 0
    # the hook counted the same images when it verified them (like badcrc_from_extstore)
    assert int(re.search(r"hook items \d+ nbad (\d+)", r.stdout).group(1)) == f["expected"]
    assert f["kept"] > 0 and f["stamped"] > 6000

    # the negative control: the plain stamp launders every damaged image
    r2 = subprocess.run([compact_exe, "--gpu", "--launder"], capture_output=True, text=True, timeout=300)
    print(r2.stdout)
    assert r2.returncode == 0, r2.stdout + r2.stderr
    g = _counts(r2.stdout)
    assert g["badcrc"] == 0 and g["expected"] == f["expected"] and g["kept"] == 0
    assert g["stamped"] == f["stamped"] + f["kept"] + f["expected"]

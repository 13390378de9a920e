"""tests/integration/copy_sim.c: storage_compact_readback's rescue copy through
crc32c_copy_items.  The images compaction keeps are moved by one call that also
verifies them, and only the intact ones are relinked: an image damaged on flash
is dropped at the moment of the copy instead of failing a client's read later.
The reference's unchecked memcpy (--memcpy) carries every damaged image along."""
import re
import subprocess

import pytest

from .test_integration import _NOGPU, _build_c


@pytest.fixture(scope="module")
def copy_exe(tmp_path_factory):
    return _build_c(tmp_path_factory, "copy_sim")


def _counts(out):
    m = re.search(r"^rescued=(\d+) dropped=(\d+) expected=(\d+) badcrc_after=(\d+)$", out, re.M)
    assert m, out
    return dict(zip(("rescued", "dropped", "expected", "badcrc_after"), map(int, m.groups())))


def test_copy_sim_without_gpu(copy_exe):
    r = subprocess.run([copy_exe], capture_output=True, text=True, env=_NOGPU, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "no gfx950 device" in r.stdout


@pytest.mark.gpu
def test_copy_sim_drops_damaged_images_at_the_copy(copy_exe):
    r = subprocess.run([copy_exe, "--gpu"], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    f = _counts(r.stdout)
    assert f["dropped"] == f["expected"] > 0
    assert f["badcrc_after"] == 0 and f["rescued"] > 500

    # the negative control: the unchecked copy relinks every damaged image
    r2 = subprocess.run([copy_exe, "--gpu", "--memcpy"], capture_output=True, text=True, timeout=300)
    print(r2.stdout)
    assert r2.returncode == 0, r2.stdout + r2.stderr
    g = _counts(r2.stdout)
    assert g["expected"] == f["expected"] and g["badcrc_after"] == g["expected"] and g["dropped"] == 0
    assert g["rescued"] == f["rescued"] + f["dropped"]

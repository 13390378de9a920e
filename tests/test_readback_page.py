"""tests/integration/readback_page.h: the page and the damage that the eight
read-back sims share, pinned on the CPU.  The sims return before they build the
page when there is no GPU, so readback_page_check.c builds it for each damage
profile and prints the counts and the scalar crc32c of the pristine and of the
damaged page.

The lines below were measured on the commit before the header existed, from
each sim's own copy of the generator: its no-GPU return dropped and this line
printed right after its damage passes.  The sims that claimed the same page
printed the same line: salvage_sim and recover_sim profile 0, repair_sim 1,
bytes_sim 2, header_sim, triage_sim, scrub_sim and gaps_sim 3.  A change of
the header that moves one of them has changed what the GPU tests of the sims
run on."""
import pytest

from .test_integration import _build_c, _run_sim

PAGES = """\
profile=0 nitems=5317 live=2078 ndamaged=56 nlen=0 ndata=0 nsame=0 ntwo=0 pristine=32e0e800 damaged=1f45e9e8
profile=1 nitems=5317 live=2078 ndamaged=56 nlen=0 ndata=289 nsame=0 ntwo=0 pristine=32e0e800 damaged=55d80493
profile=2 nitems=5317 live=2078 ndamaged=56 nlen=0 ndata=289 nsame=29 ntwo=28 pristine=32e0e800 damaged=687bea7f
profile=3 nitems=5317 live=2078 ndamaged=56 nlen=184 ndata=263 nsame=0 ntwo=0 pristine=32e0e800 damaged=ed0d765f
"""


@pytest.fixture(scope="module")
def check_exe(tmp_path_factory):
    return _build_c(tmp_path_factory, "readback_page_check")


def test_readback_page_bytes_are_the_sims_own(check_exe):
    assert _run_sim(check_exe) == PAGES

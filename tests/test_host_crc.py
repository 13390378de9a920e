"""The scalar drop-in's host CRC (memcached_amd/csrc/crc32c_host.cpp) against
the oracle where its loops change, checked on the CPU: tests/integration/
host_crc_check.cpp links crc32c_host.cpp with oracle/crc32c_oracle.c under the
address and undefined-behaviour sanitizers.  The three-stream merge of
crc32c_host_hw runs its 3 x 4096-B round first at 12 288 bytes behind the
alignment prologue, which tests/golden/spans.npz (lengths 0..4200) never
reaches."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SAN = "-fsanitize=address,undefined"


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("host_crc")
    obj, out = str(tmp / "crc32c_oracle.o"), str(tmp / "host_crc_check")
    subprocess.run(["gcc", "-O1", "-Wall", "-Werror", SAN, "-c", os.path.join(ROOT, "oracle", "crc32c_oracle.c"),
                    "-o", obj], check=True)
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", SAN,
                    "-I", os.path.join(ROOT, "memcached_amd", "csrc"),
                    os.path.join(HERE, "integration", "host_crc_check.cpp"),
                    os.path.join(ROOT, "memcached_amd", "csrc", "crc32c_host.cpp"), obj, "-o", out], check=True)
    return out


def test_host_crc_matches_the_oracle_at_the_merge_rounds(exe):
    """crc32c_host_hw and crc32c_host_sw equal oracle_crc32c at 30 lengths
    around the rounds of 3 x 256 B and 3 x 4096 B, from starts 0..8 of a 64-B
    aligned base, seeded with 0, 0xdeadbeef and 0xffffffff, whole and in two
    calls cut at 256 and 4096 bytes; crc32c_host_combine equals the oracle's
    CRC of the appended bytes."""
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "host_crc ok" in r.stdout
    print(r.stdout.strip())

"""The K1 counter-slot table (memcached_amd/csrc/k1_slots.h) on the CPU:
tests/integration/k1_slots_check.cpp drives it from 8 threads (one key,
distinct keys, more keys than slots, the special handles), built plain and
with -fsanitize=thread (skipped where the toolchain cannot link that runtime)."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "memcached_amd", "csrc")
SRC = os.path.join(HERE, "integration", "k1_slots_check.cpp")


def _build(out, extra):
    return subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-pthread"] + extra +
                          ["-I", CSRC, SRC, "-o", out], capture_output=True, text=True)


def test_k1_slots_plain(tmp_path):
    out = str(tmp_path / "k1_slots_check")
    b = _build(out, [])
    assert b.returncode == 0, b.stderr
    r = subprocess.run([out], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr


def test_k1_slots_thread_sanitizer(tmp_path):
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    p = subprocess.run(["g++", "-fsanitize=thread", str(probe), "-o", str(tmp_path / "probe")], capture_output=True)
    if p.returncode != 0 or subprocess.run([str(tmp_path / "probe")], capture_output=True).returncode != 0:
        pytest.skip("this toolchain cannot link or start the thread sanitizer's runtime")
    out = str(tmp_path / "k1_slots_check_tsan")
    b = _build(out, ["-fsanitize=thread"])
    assert b.returncode == 0, b.stderr
    r = subprocess.run([out], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr

"""The store decomposition of k_copy (memcached_amd/csrc/copy_edges.h) on the
CPU: tests/integration/copy_edges_check.cpp runs it for every source alignment
x destination alignment x ITEM_ntotal in 50..300, 4096 +- 80 and 8192 +- 80
and checks that the stores cover the image exactly once, touch nothing else
and take every byte from the aligned 16-B source piece that holds it."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def test_copy_edges_exhaustive(tmp_path):
    exe = str(tmp_path / "copy_edges_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "memcached_amd", "csrc"),
                    os.path.join(HERE, "integration", "copy_edges_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "copy_edges ok (146688 cases)" in r.stdout  # 256 pairs x (251 + 2 x 161) lengths

"""tools/codeobj_diff.py names the target of a PC-relative address by symbol
and offset before it compares two builds; its self-test shows the rewrite on
a synthetic function: the same function moved compares equal, and an add that
is not of that shape is left as text.  No GPU, no built library needed."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_self_test_passes():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "codeobj_diff.py"), "--self-test"],
                       capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "self-test ok" in r.stdout, r.stdout + r.stderr

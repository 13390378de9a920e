"""The grow-only buffer type behind every scratch allocation of the host shim
(memcached_amd/csrc/grow_buf.h), checked on the CPU: tests/integration/
grow_buf_check.cpp instantiates it over a memory policy that keeps a ledger of
live blocks, counts calls, fails the allocation it is told to and aborts on the
free of an address that is not live."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def test_grow_buf_contract(tmp_path):
    """Grow (one allocation of exactly the requested size), no shrink and no
    churn (a smaller or equal reserve: same pointer, no allocator call),
    regrow (the old block freed exactly once), failed regrow (buffer empty,
    old block freed once, the next reserve afresh), the mapped policy (host
    and device address both reset on failure), and a group of ten buffers
    reserved in sequence with allocation k failing, for every k in 1..10,
    each followed by the whole sequence without a failure: ten live blocks of
    the right sizes at the end and no free of an address that is not live.

    The group case fails on a transliteration of the scheme the buffers
    replaced (ensure_plan's free-everything, allocate-in-one-||-chain, one
    watermark): after allocation k fails, the pointers past k keep freed
    addresses and the next call frees them again.  The program runs that
    transliteration over the same ledger as a negative control and requires
    the ledger to report it."""
    exe = str(tmp_path / "grow_buf_check")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "memcached_amd", "csrc"),
                    os.path.join(HERE, "integration", "grow_buf_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "grow_buf ok" in r.stdout

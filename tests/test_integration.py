"""The extstore CRC flow of storage.c driven through libmcrc32c.so from C:

* storage_sim.c: scalar drop-in on the CPU; batched spill stamping, page walk
  + verify and an IO read batch on the GPU.
* extstore_config1.c: BASELINE configs[0], 10 000 SETs of 4 KiB values spilled
  to a page file and read back, checked against the reference's CRCs of the
  same items (tests/golden/config1.json).
* queue_sim.c: many IO threads' read-verify batches (io_depth-sized,
  extstore.c:853-945) through the coalescing queue.
* extstore_sim.c: the deferred (batched) spill CRC under a concurrent writer,
  flusher and readers, with the open-wbuf read fence -- and without it, the
  negative control that shows the false bad CRCs the fence prevents."""
import json
import os
import re
import subprocess

import numpy as np

import pytest

from memcached_amd import build

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def _build_c(tmp_path_factory, name):
    lib = build.build_lib()
    exe = str(tmp_path_factory.mktemp(name) / name)
    subprocess.run(["gcc", "-O2", "-Wall", "-Werror", "-pthread", "-I", os.path.join(ROOT, "include"),
                    os.path.join(HERE, "integration", name + ".c"), "-L", os.path.dirname(lib), "-lmcrc32c",
                    f"-Wl,-rpath,{os.path.dirname(lib)}", "-o", exe], check=True)
    return exe


_NOGPU = dict(os.environ, HIP_VISIBLE_DEVICES="-1")


def _run_sim(exe, *args, gpu=False):
    """Runs a sim with --gpu, or without it on its no-GPU leg; returns its
    stdout.  The run itself must have worked: exit status 0."""
    if gpu:
        r = subprocess.run([exe, "--gpu", *args], capture_output=True, text=True, timeout=300)
    else:
        r = subprocess.run([exe, *args], capture_output=True, text=True, env=_NOGPU, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout


def _sim_fields(stdout, fields):
    """The sim's line of counts, `name=<int> ...` in exactly this order, as a dict."""
    m = re.search("^" + " ".join(f"{f}=(\\d+)" for f in fields) + "$", stdout, re.M)
    assert m, stdout
    return dict(zip(fields, map(int, m.groups())))


@pytest.fixture(scope="module")
def sim(tmp_path_factory):
    return _build_c(tmp_path_factory, "storage_sim")


def test_storage_sim_scalar_dropin(sim):
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1")  # the CPU leg: batch calls must report ENODEV
    r = subprocess.run([sim], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "scalar drop-in ok" in r.stdout


@pytest.mark.gpu
def test_storage_sim_gpu(sim):
    r = subprocess.run([sim, "--gpu"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "badcrc 1" in r.stdout


@pytest.fixture(scope="module")
def config1_exe(tmp_path_factory):
    return _build_c(tmp_path_factory, "extstore_config1")


def _golden_config1():
    return json.load(open(os.path.join(HERE, "golden", "config1.json")))


def test_config1_extstore_spill_and_readback(config1_exe, tmp_path):
    """Config 1 on the CPU: scalar drop-in for spill and read-back, 0 bad CRCs,
    exactly 1 after one byte is torn on disk, and the spill CRCs of all 10 000
    items identical to the reference crc32c.c's (digest + the page file
    re-checked item by item with the oracle)."""
    from memcached_amd import layout

    from . import oracle
    g = _golden_config1()
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1")
    r = subprocess.run([config1_exe, str(tmp_path)], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.search(r"config1: (\d+) written in (\d+) wbufs, (\d+) read, badcrc (\d+), torn-item badcrc (\d+), "
                  r"digest ([0-9a-f]{8})", r.stdout)
    assert m, r.stdout
    written, wbufs, read, bad, torn, digest = m.groups()
    assert (int(written), int(wbufs), int(read)) == (g["items"], g["wbufs"], g["items"])
    assert (int(bad), int(torn)) == (0, 1)
    assert int(digest, 16) == g["digest"]
    page = np.fromfile(tmp_path / "extstore.page", np.uint8)
    offs = []
    for w in range(g["wbufs"]):
        o = w * g["wbuf"]
        while o + 48 <= (w + 1) * g["wbuf"] and page[o + layout.NKEY_OFF] != 0:
            offs.append(o)
            o += layout.ntotal_of(page, o)
    offs = np.asarray(offs, np.uint64)
    assert offs.size == g["items"]
    soffs, slens = layout.spans_of(page, offs)
    crcs = oracle.batch(page, soffs, slens)
    stored = page[(offs[:, None] + np.arange(28, 32)).astype(np.int64)].copy().view("<u4").reshape(-1)
    np.testing.assert_array_equal(stored, crcs)
    assert [int(c) for c in crcs[:8]] == g["first_crcs"] and [int(c) for c in crcs[-8:]] == g["last_crcs"]


@pytest.mark.gpu
def test_config1_extstore_batched_gpu(config1_exe, tmp_path):
    """Config 1 with the batched calls: stamp == scalar spill, the page read
    back from the file verifies clean, the 10 000-read batch matches."""
    r = subprocess.run([config1_exe, str(tmp_path), "--gpu"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "config1 gpu: stamped == scalar, page verify nbad 0, read batch mismatches 0" in r.stdout
    assert "digest %08x" % _golden_config1()["digest"] in r.stdout


@pytest.fixture(scope="module")
def queue_exe(tmp_path_factory):
    return _build_c(tmp_path_factory, "queue_sim")


@pytest.fixture(scope="module")
def extstore_exe(tmp_path_factory):
    return _build_c(tmp_path_factory, "extstore_sim")


def test_queue_sim_without_gpu(queue_exe):
    r = subprocess.run([queue_exe], capture_output=True, text=True, env=_NOGPU, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "no gfx950 device" in r.stdout


def test_extstore_sim_without_gpu(extstore_exe):
    r = subprocess.run([extstore_exe], capture_output=True, text=True, env=_NOGPU, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "no gfx950 device" in r.stdout


def _fields(line):
    toks = line.split()
    return {toks[i]: toks[i + 1] for i in range(len(toks) - 1)}


@pytest.mark.gpu
@pytest.mark.parametrize("threads,reads,depth", [(16, 2000, 1), (8, 1000, 8), (1, 300, 1)])
def test_queue_sim_many_io_threads(queue_exe, threads, reads, depth):
    """io_depth-sized read batches from many threads: every CRC exact, every
    torn read (and only those) detected, and the batches shared launches."""
    r = subprocess.run([queue_exe, "--gpu", str(threads), str(reads), str(depth)], capture_output=True, text=True,
                       timeout=300)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    f = _fields(r.stdout)
    assert int(f["mismatches"]) == 0 and int(f["false_bad"]) == 0 and f["detected"] == f["torn"]
    assert int(f["spans"]) == threads * reads * depth
    if threads > 1:
        assert int(f["launches"]) < int(f["jobs"])  # coalesced


@pytest.mark.gpu
def test_extstore_sim_open_wbuf_fence(extstore_exe):
    """Deferred stamping with the fence: reads of the open wbuf (and all
    others) verify clean; every image ends with the scalar spill CRC."""
    r = subprocess.run([extstore_exe, "--gpu", "8"], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    f = _fields(r.stdout.replace(",", ""))
    assert int(f["badcrc"]) == 0 and int(f["wbuf"].rstrip(")")) > 0


@pytest.mark.gpu
def test_extstore_sim_without_fence_sees_false_badcrc(extstore_exe):
    """Negative control: the same run with the fence removed reports bad CRCs
    for reads served from the open wbuf (the hole of a deferred stamp)."""
    r = subprocess.run([extstore_exe, "--gpu", "--no-fence", "8"], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert int(_fields(r.stdout.replace(",", ""))["badcrc"]) > 0


# The reference's own extstore.c with the INTEGRATION.md section 2 hunks
# (tests/integration/extstore_ref.patch), built in the build container by
# oracle/build_extstore_ref.sh into oracle/_ref/ (test infrastructure, like
# the reference crc32c.c build there); the binaries travel to the GPU box.
_EXT_REF = os.path.join(ROOT, "oracle", "_ref", "extstore_ref")


def _run_ext_ref(tmp_path, nofence=False, gpu=False):
    exe = _EXT_REF + ("_nofence" if nofence else "")
    if not os.path.exists(exe):
        pytest.skip("oracle/_ref/extstore_ref not built (no /root/reference where the tree was built)")
    r = subprocess.run([exe, str(tmp_path), "8"], capture_output=True, text=True, timeout=300,
                       env=None if gpu else _NOGPU)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("extstore_ref:")][0]
    toks = line.split(":", 1)[1].split()
    return {k: int(v) for k, v in zip(toks[0::2], toks[1::2])}


def test_reference_extstore_deferred_stamp_with_fence_cpu(tmp_path):
    """The reference extstore.c with the batched stamp at _submit_wbuf and the
    open-wbuf fence, no GPU (the stamp hook falls back to storage.c:567 per
    item): every read verifies, and reads of the open wbuf were stamped on
    demand."""
    f = _run_ext_ref(tmp_path)
    assert f["badcrc"] == 0 and f["corrupt"] == 0 and f["short"] == 0
    assert f["open_wbuf_stamps"] > 0 and f["fallback_batches"] > 0 and f["batches"] == 0
    assert f["reads"] > 24000


def test_reference_extstore_without_fence_sees_false_badcrc_cpu(tmp_path):
    """Negative control: the fence hunk compiled out, reads of the open wbuf
    see unstamped images (bad CRC, bytes intact)."""
    f = _run_ext_ref(tmp_path, nofence=True)
    assert f["badcrc"] > 0 and f["false_bad"] == f["badcrc"] and f["corrupt"] == 0


@pytest.mark.gpu
def test_reference_extstore_batched_stamp_gpu(tmp_path):
    """The same run with the GPU: every submitted wbuf stamped by one
    crc32c_stamp_items call inside the reference's _submit_wbuf, badcrc 0, and
    the page file the reference's flush thread wrote verifies clean on the
    device walk (crc32c_verify_pages)."""
    f = _run_ext_ref(tmp_path, gpu=True)
    assert f["badcrc"] == 0 and f["corrupt"] == 0 and f["short"] == 0 and f["open_wbuf_stamps"] > 0
    assert f["batches"] > 0 and f["fallback_batches"] == 0 and f["stamp_nbad"] == 0
    assert f["page_verify_rc"] == 0 and f["nbad"] == 0 and f["nitems"] >= 0.9 * f["written"]


@pytest.mark.gpu
def test_reference_extstore_without_fence_sees_false_badcrc_gpu(tmp_path):
    f = _run_ext_ref(tmp_path, nofence=True, gpu=True)
    assert f["batches"] > 0 and f["badcrc"] > 0 and f["false_bad"] == f["badcrc"] and f["corrupt"] == 0
    assert f["page_verify_rc"] == 0 and f["nbad"] == 0

#!/usr/bin/env python3
"""Compare the gfx950 code objects of two builds of libmcrc32c.so (no GPU).

    python tools/codeobj_diff.py OLD.so NEW.so

Per function symbol: the disassembly (llvm-objdump -d --no-show-raw-insn, the
trailing `// address` comments stripped, and the padding between a function's
last instruction and the next symbol dropped).  Per kernel: the VGPR, SGPR and AGPR
counts, the LDS, scratch and kernarg sizes, .name and .symbol of its metadata
note.  Prints the names that differ, or that only one side has, and exits 1 if
there are any: the gate of a refactor that must not change the device code.
"""
import os
import re
import subprocess
import sys
import tempfile

LLVM = os.environ.get("LLVM_BIN", "/opt/rocm/lib/llvm/bin")
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"
FIELDS = (".vgpr_count", ".sgpr_count", ".agpr_count", ".group_segment_fixed_size", ".private_segment_fixed_size",
          ".kernarg_segment_size", ".name", ".symbol")


def _out(*cmd):
    return subprocess.run(cmd, check=True, capture_output=True, text=True).stdout


def code_object(lib, tmp):
    """As tests/test_kernel_resources.py: the fat binary section, unbundled."""
    fat, co = os.path.join(tmp, "fatbin.bin"), os.path.join(tmp, "gfx950.co")
    subprocess.run(["objcopy", "-O", "binary", "--only-section=.hip_fatbin", lib, fat], check=True)
    subprocess.run([os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o", f"--input={fat}",
                    f"--targets={TARGET}", f"--output={co}"], check=True)
    return co


def functions(co):
    out, cur = {}, None
    for line in _out(os.path.join(LLVM, "llvm-objdump"), "-d", "--no-show-raw-insn", co).splitlines():
        m = re.match(r"[0-9a-f]+ <(\S+)>:$", line)
        if m:
            cur = out.setdefault(m.group(1), [])
        elif cur is not None and line.strip():
            cur.append(re.sub(r"\s*//.*$", "", line).strip())
    # what follows a function's last s_endpgm up to the next symbol is padding
    # (s_nop fill behind the section's last function, "..." for skipped zeros):
    # it moves when a function is added behind it and is no instruction of it
    # (only behind an instruction that ends the function: nothing else is cut)
    for body in out.values():
        k = len(body)
        while k and body[k - 1] in ("s_nop 0", "..."):
            k -= 1
        if k and body[k - 1].split()[0] in ("s_endpgm", "s_branch", "s_setpc_b64"):
            del body[k:]
    return out


def kernels(co):
    out = {}
    for blk in _out(os.path.join(LLVM, "llvm-readobj"), "--notes", co).split("  - .agpr_count")[1:]:
        blk = ".agpr_count" + blk
        rec = {f: re.search(rf"{re.escape(f)}:\s+(\S+)", blk).group(1) for f in FIELDS}
        out[rec[".name"]] = rec
    return out


def load(lib):
    with tempfile.TemporaryDirectory() as tmp:
        co = code_object(lib, tmp)
        return functions(co), kernels(co)


def main(old, new):
    (fo, ko), (fn, kn) = load(old), load(new)
    bad = 0
    for what, a, b in (("function", fo, fn), ("kernel", ko, kn)):
        for name in sorted(set(a) | set(b)):
            if name not in a or name not in b:
                print(f"{what} only in {'NEW' if name in b else 'OLD'}: {name}")
            elif a[name] != b[name]:
                detail = ""
                if what == "kernel":
                    detail = " " + ", ".join(f"{f} {a[name][f]} -> {b[name][f]}" for f in FIELDS
                                             if a[name][f] != b[name][f])
                else:
                    detail = f" ({len(a[name])} -> {len(b[name])} instructions)"
                print(f"{what} differs: {name}{detail}")
            else:
                continue
            bad += 1
    print(f"{len(fo)} / {len(fn)} functions, {len(ko)} / {len(kn)} kernels compared: "
          + (f"{bad} differences" if bad else "identical"))
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    sys.exit(main(sys.argv[1], sys.argv[2]))

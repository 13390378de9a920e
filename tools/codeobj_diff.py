#!/usr/bin/env python3
"""Compare the gfx950 code objects of two builds of libmcrc32c.so (no GPU).

    python tools/codeobj_diff.py OLD.so NEW.so
    python tools/codeobj_diff.py --self-test

Per function symbol: the disassembly (llvm-objdump -d --no-show-raw-insn, the
trailing `// address` comments stripped, and the padding between a function's
last instruction and the next symbol dropped, the literal of a PC-relative
address named by the symbol it points at: symbolise below).  Per kernel: the VGPR, SGPR and AGPR
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


def symbols(co):
    """(address, name) of every symbol that is no function, ascending."""
    out = []
    for line in _out(os.path.join(LLVM, "llvm-readelf"), "-s", "-W", co).splitlines():
        f = line.split()  # Num: Value Size Type Bind Vis Ndx Name
        if len(f) == 8 and f[3] in ("OBJECT", "NOTYPE") and f[6] not in ("UND", "ABS"):
            out.append((int(f[1], 16), f[7]))
    return sorted(out)


def _where(syms, addr):
    """addr as symbol + offset (data a function addresses moves when kernels are added beside it)."""
    best = None
    for a, name in syms:
        if a > addr:
            break
        best = (a, name)
    return f"<{best[1]}+{addr - best[0]:#x}>" if best else f"{addr:#x}"


def symbolise(lines, syms):
    """The instructions of one function, `lines` = [(address or None, text)],
    with the literal of a PC-relative address formation replaced by what it
    addresses.  The compiler forms such an address as

        s_getpc_b64 s[N:N+1]          (at A: the registers receive A + 4)
        s_add_u32   sN, sN, lit       (lit = target - (A + 4), the low half)
        s_addc_u32  sN+1, sN+1, hi    (0 or 0xffffffff: lit's sign)

    so lit, read as a signed 32-bit distance from A + 4, names the target (a
    code object is far smaller than 2 GiB).  The distance changes whenever
    kernels or their descriptors are added between the function and its data,
    although no instruction of the function does; `<symbol+offset>` does not.
    Only this one shape is rewritten: the add must name the register pair's low
    half, carry a literal, and come within three instructions of the
    s_getpc_b64, before anything else writes that register.  Everything else
    is compared as text."""
    out, pending = [], {}  # register -> (A + 4, instructions since)
    for at, ins in lines:
        g = re.match(r"s_getpc_b64 s\[(\d+):\d+\]$", ins)
        a = re.match(r"s_add_u32 s(\d+), s(\d+), (0x[0-9a-f]+)$", ins)
        if a and a.group(1) == a.group(2) and a.group(1) in pending:
            lit = int(a.group(3), 16)
            target = pending.pop(a.group(1))[0] + (lit - (1 << 32) if lit >> 31 else lit)
            ins = f"s_add_u32 s{a.group(1)}, s{a.group(1)}, {_where(syms, target)}"
        else:
            w = re.match(r"\S+ s(\d+),", ins)  # (another write of the register ends the wait)
            if w:
                pending.pop(w.group(1), None)
        pending = {r: (v, k + 1) for r, (v, k) in pending.items() if k < 3}
        if g and at is not None:
            pending[g.group(1)] = (at + 4, 0)
        out.append(ins)
    return out


def self_test():
    syms = [(0x100, ".tab"), (0x4500, ".other")]
    body = [(0x1000, "s_getpc_b64 s[6:7]"), (0x1004, "s_add_u32 s6, s6, 0xfffff0fc"),
            (0x100c, "s_addc_u32 s7, s7, -1"), (0x1010, "s_add_u32 s6, s6, 0x10"),
            (0x2000, "s_getpc_b64 s[8:9]"), (0x2004, "s_mov_b32 s8, 0"), (0x2008, "s_add_u32 s8, s8, 0x40"),
            (0x3000, "s_getpc_b64 s[4:5]"), (None, "v_nop"), (None, "v_nop"), (None, "v_nop"), (None, "v_nop"),
            (0x3014, "s_add_u32 s4, s4, 0x40"), (0x4000, "s_getpc_b64 s[2:3]"), (0x4004, "s_add_u32 s2, s2, 0x4fc")]
    got = symbolise(body, syms)
    # 0x1004 - 0xf04 = 0x100: the table itself; the same function moved by 0x40 names it the same way
    moved = symbolise([(a + 0x40 if a is not None else a,
                        i.replace("0xfffff0fc", "0xfffff0bc").replace("0x4fc", "0x4bc")) for a, i in body], syms)
    assert got == moved, (got, moved)
    assert got[1] == "s_add_u32 s6, s6, <.tab+0x0>" and got[14] == "s_add_u32 s2, s2, <.other+0x0>"
    assert got[3] == body[3][1] and got[6] == body[6][1] and got[12] == body[12][1]  # not the shape: left alone
    print("codeobj_diff self-test ok")
    return 0


def functions(co):
    raw, cur = {}, None
    syms = symbols(co)
    for line in _out(os.path.join(LLVM, "llvm-objdump"), "-d", "--no-show-raw-insn", co).splitlines():
        m = re.match(r"[0-9a-f]+ <(\S+)>:$", line)
        if m:
            cur = raw.setdefault(m.group(1), [])
        elif cur is not None and line.strip():
            at = re.search(r"//\s*([0-9A-Fa-f]+):", line)
            cur.append((int(at.group(1), 16) if at else None, re.sub(r"\s*//.*$", "", line).strip()))
    out = {name: symbolise(lines, syms) for name, lines in raw.items()}
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
    if sys.argv[1:] == ["--self-test"]:
        sys.exit(self_test())
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    sys.exit(main(sys.argv[1], sys.argv[2]))

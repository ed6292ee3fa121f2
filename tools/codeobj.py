"""Kernel resource records of the shipped library, read from its gfx950 code objects (no GPU needed).

libhdf_hip.so carries one clang offload bundle per translation unit in .hip_fatbin; each holds a gfx950 ELF whose
NT_AMDGPU_METADATA note lists, per kernel: registers, spills, scratch (private segment) and static LDS.
`kernels(so)` returns {demangled name: record}; `disassemble(so, name_substring)` the instruction mnemonics of one kernel.
CLI: python tools/codeobj.py [regex]        -> one line per kernel
     python tools/codeobj.py --diff A.so B.so [--rename 'OLD_REGEX=NEW' ...]
                                              -> what a refactor changed between two builds (exit status 1 if anything);
                                                 --rename pairs a kernel of A with the kernel of B that carries its new name."""
import collections
import os
import re
import struct
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "h-denseformer_amd", "lib", "libhdf_hip.so")
LLVM = "/opt/rocm/lib/llvm/bin"
MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"


def code_objects(so=LIB):
    """the gfx950 ELF images inside the library, in file order"""
    data = open(so, "rb").read()
    out = []
    for m in re.finditer(MAGIC, data):
        p = m.start()
        nb = struct.unpack_from("<Q", data, p + 24)[0]
        q = p + 32
        for _ in range(nb):
            off, size, tl = struct.unpack_from("<QQQ", data, q)
            triple = data[q + 24:q + 24 + tl].decode()
            q += 24 + tl
            if "gfx950" in triple and size:
                out.append(data[p + off:p + off + size])
    return out


def _demangle(names):
    r = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True)
    return [n.replace("(anonymous namespace)::", "").replace("void ", "") for n in r.stdout.splitlines()]


def kernels(so=LIB):
    recs = {}
    for img in code_objects(so):
        with tempfile.NamedTemporaryFile(suffix=".elf") as f:
            f.write(img)
            f.flush()
            txt = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", f.name], capture_output=True, text=True).stdout
        cur = None
        items = []
        for line in txt.splitlines():
            m = re.match(r"\s+- \.agpr_count:\s+(\d+)", line)
            if m:
                cur = {"agpr_count": int(m.group(1))}
                items.append(cur)
                continue
            m = re.match(r"\s+\.(name|vgpr_count|sgpr_count|vgpr_spill_count|sgpr_spill_count|private_segment_fixed_size|"
                         r"group_segment_fixed_size|max_flat_workgroup_size):\s+(\S+)", line)
            if m and cur is not None:
                cur[m.group(1)] = m.group(2) if m.group(1) == "name" else int(m.group(2))
        names = _demangle([k["name"] for k in items])
        for k, n in zip(items, names):
            k["mangled"] = k["name"]
            k["name"] = re.sub(r"\(.*", "", n)
            k["regs"] = k["vgpr_count"]   # (unified file: .vgpr_count already includes the AGPRs)
            alloc = -(-max(k["regs"], 1) // 8) * 8
            k["waves_per_simd"] = min(8, 512 // alloc)
            recs[k["name"]] = k
    return recs


def _objdump(img, symbol=None):
    """llvm-objdump -d of one code object (of one symbol): [(symbol, instruction line)].  A failed whole-object run raises;
    with a symbol, a code object that lacks it just yields nothing"""
    with tempfile.NamedTemporaryFile(suffix=".elf") as f:
        f.write(img)
        f.flush()
        sel = [f"--disassemble-symbols={symbol}"] if symbol else []
        r = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", "--no-show-raw-insn"] + sel + [f.name],
                           capture_output=True, text=True)
    if r.returncode != 0 and not symbol:
        raise RuntimeError("llvm-objdump failed:\n" + r.stderr[-2000:])
    out, cur = [], None
    for line in r.stdout.splitlines():
        m = re.match(r"[0-9a-f]+ <(\S+)>:", line)
        if m:
            cur = m.group(1)
        elif re.match(r"\s+[a-z_0-9]+ ", line) or re.match(r"\s+[sv]_[a-z_0-9]+", line):
            out.append((cur, line.strip()))
    return out


def disassemble(mangled, so=LIB):
    """instruction lines of one kernel (by mangled name)"""
    for img in code_objects(so):
        lines = [l for _, l in _objdump(img, mangled)]
        if lines:
            return lines
    return []


RESOURCES = ("vgpr_count", "agpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size",
             "group_segment_fixed_size", "max_flat_workgroup_size")


def instruction_streams(so=LIB):
    """{mangled name: instruction lines} of every kernel, one objdump run per code object; made comparable between builds:
    the trailing comment (address, encoding, branch-target label) is dropped -- the relative branch offset stays -- as is
    the padding behind the last s_endpgm, and the literal of an s_add_u32 / s_addc_u32 that follows s_getpc_b64 (the
    pc-relative address of a global, which moves with the layout of the code object)"""
    out = {}
    for img in code_objects(so):
        pcrel = 0
        for sym, line in _objdump(img):
            cur = out.setdefault(sym, [])
            ins = re.sub(r"\s+", " ", line.split("//")[0].strip())
            if not cur:
                pcrel = 0
            if ins.startswith("s_getpc_b64"):
                pcrel = 3
            elif pcrel and re.match(r"s_addc?_u32 ", ins):
                ins = re.sub(r", (0x[0-9a-f]+|\d+)$", ", <pcrel>", ins)
            pcrel = max(0, pcrel - 1)
            cur.append(ins)
    for name, lines in out.items():
        while lines and re.match(r"s_nop|s_code_end", lines[-1]):
            lines.pop()
    return out


def _mnemonic_counts(lines):
    """{mnemonic: count}; an s_waitcnt counts per operand string (hand-counted vmcnt waits are part of a kernel's design)"""
    c = collections.Counter()
    for l in lines:
        c[l if l.startswith("s_waitcnt") else l.split(" ")[0]] += 1
    return c


def diff(so_a, so_b, renames=()):
    """print the differences between two builds; returns their number.  renames: (regex, replacement) pairs applied to the
    demangled kernel names of A -- a kernel whose name changes that way is compared with B's kernel of the new name"""
    ka = {k["mangled"]: k for k in kernels(so_a).values()}
    kb = {k["mangled"]: k for k in kernels(so_b).values()}
    b_by_name = {k["name"]: m for m, k in kb.items()}
    pairs = {}  # mangled name in A -> mangled name in B
    for m, k in ka.items():
        new = k["name"]
        for pat, rep in renames:
            new = re.sub(pat, rep, new)
        mb = b_by_name.get(new) if new != k["name"] else (m if m in kb else None)
        if mb is not None:
            pairs[m] = mb
    n = 0
    for tag, recs, only in (("only in A", ka, sorted(set(ka) - set(pairs))),
                            ("only in B", kb, sorted(set(kb) - set(pairs.values())))):
        for m in only:
            print("%s: %s" % (tag, recs[m]["name"]))
            n += 1
    sa, sb = instruction_streams(so_a), instruction_streams(so_b)
    for tag, streams, names in (("A", sa, pairs), ("B", sb, pairs.values())):
        missing = [m for m in names if not streams.get(m)]
        if missing:
            raise RuntimeError("no instruction stream in %s for %d kernels, e.g. %s" % (tag, len(missing), missing[0]))
    for m, mb in sorted(pairs.items()):
        ra, rb = [ka[m].get(r, 0) for r in RESOURCES], [kb[mb].get(r, 0) for r in RESOURCES]
        if ra != rb:
            print("resources differ: %s\n    %s" % (ka[m]["name"], ", ".join(
                "%s %d -> %d" % (r, x, y) for r, x, y in zip(RESOURCES, ra, rb) if x != y)))
            n += 1
        if sa[m] != sb[mb]:
            la, lb = sa[m], sb[mb]
            first = next((i for i, (x, y) in enumerate(zip(la, lb)) if x != y), min(len(la), len(lb)))
            print("instructions differ: %s\n    %d -> %d instructions, first difference at %d: %s | %s" % (
                ka[m]["name"], len(la), len(lb), first, la[first] if first < len(la) else "-", lb[first] if first < len(lb) else "-"))
            ca, cb = _mnemonic_counts(la), _mnemonic_counts(lb)
            moved = ["%s %+d" % (k, cb[k] - ca[k]) for k in sorted(set(ca) | set(cb)) if ca[k] != cb[k]]
            print("    counts moved: %s" % (", ".join(moved) or "none (order or operands only)"))
            n += 1
    print("%d kernels in A, %d in B, %d paired, %d differences" % (len(ka), len(kb), len(pairs), n))
    return n


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--diff":
        args, renames = sys.argv[2:], []
        while "--rename" in args:
            i = args.index("--rename")
            renames.append(tuple(args[i + 1].split("=", 1)))
            del args[i:i + 2]
        sys.exit(1 if diff(args[0], args[1], renames) else 0)
    pat = sys.argv[1] if len(sys.argv) > 1 else ""
    for n, k in sorted(kernels().items()):
        if pat and not re.search(pat, n):
            continue
        print("%-100s V%3d A%3d S%3d spillV%3d scr%4d lds%6d w/simd %d" % (
            n[:100], k["vgpr_count"], k["agpr_count"], k["sgpr_count"], k.get("vgpr_spill_count", 0),
            k.get("private_segment_fixed_size", 0), k.get("group_segment_fixed_size", 0), k["waves_per_simd"]))

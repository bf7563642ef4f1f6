#!/usr/bin/env python3
"""Generated code of two builds side by side, per kernel (no GPU needed): what "the same kernel" means when a refactor moves code.

    python tools/codeobj_compare.py OLD NEW k_nee k_direct ...

OLD and NEW are libmpt_hip.so builds (their gfx950 code object is taken out as tests/test_nee_codeobj.py takes it out) or gfx950 code
objects themselves.  A kernel is chosen when its name, without the template arguments, is one of the names given (none: every kernel).
Per kernel: vgpr / sgpr counts, the two spill counts, scratch and static LDS of both builds, and the class of its text:
    text      the same instructions with the same operands (addresses dropped, branch targets as offsets within the kernel)
    mnemonics the same sequence of mnemonics: registers renamed or operands reordered only
    differs   neither, with the instruction counts of both
Exit status 1 when a chosen kernel is missing from either build or any metadata field differs."""
import argparse
import os
import re
import shutil
import subprocess
import sys
import tempfile

LLVM = os.environ.get("LLVM_BIN", "/opt/rocm/lib/llvm/bin")
FIELDS = ("vgpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size", "group_segment_fixed_size")


def tool(name, *args, cwd=None):
    return subprocess.run([os.path.join(LLVM, name), *args], cwd=cwd, check=True, capture_output=True, text=True).stdout


def code_object(path, tmp):
    """The gfx950 code object of `path`: the file itself when it is one, else the bundle llvm-objdump --offloading writes next to it."""
    d = tempfile.mkdtemp(dir=tmp)
    shutil.copy(path, os.path.join(d, "in.bin"))
    if "EM_AMDGPU" in tool("llvm-readelf", "-h", "in.bin", cwd=d):
        return os.path.join(d, "in.bin")
    tool("llvm-objdump", "--offloading", "in.bin", cwd=d)
    co = [f for f in os.listdir(d) if "gfx950" in f]
    if len(co) != 1:
        sys.exit("%s: expected one gfx950 code object, found %r" % (path, co))
    return os.path.join(d, co[0])


def metadata(co):
    out = {}
    for block in re.split(r"\n\s*- \.agpr_count:", tool("llvm-readelf", "--notes", co))[1:]:
        name = re.search(r"\.name:\s+(\S+)", block)
        if name:
            out[name.group(1)] = {k: int(v) for k, v in re.findall(r"\.(\w+):\s+(\d+)\s*$", block, flags=re.M)}
    return out


def instructions(co):
    """{symbol: [instruction text]}: the address column and the comments dropped, a branch target kept as its offset within the kernel."""
    out, cur = {}, None
    for line in tool("llvm-objdump", "-d", "--no-show-raw-insn", co).splitlines():
        m = re.match(r"^[0-9a-f]+ <(\S+)>:$", line)
        if m:
            cur = out.setdefault(m.group(1), [])
            continue
        if cur is None or not line.startswith((" ", "\t")):
            continue
        text = line.split("//")[0].strip()
        if text:
            cur.append(re.sub(r"\s+", " ", re.sub(r"\b\d+ <\S+?(\+0x[0-9a-f]+)?>", lambda t: "<" + (t.group(1) or "+0x0") + ">", text)))
    return out


def plain_name(symbol):
    """(name, "<template arguments>") of an Itanium-mangled function at namespace scope; integer arguments only, else the mangled rest."""
    m = re.match(r"^_Z(\d+)", symbol)
    if not m:
        return symbol, ""
    end = m.end() + int(m.group(1))
    name, rest = symbol[m.end():end], symbol[end:]
    t = re.match(r"^I((?:L[a-z]\d+E)+)E", rest)
    return name, "<%s>" % ",".join(re.findall(r"L[a-z](\d+)E", t.group(1))) if t else ""


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("kernels", nargs="*")
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        co = [code_object(p, tmp) for p in (a.old, a.new)]
        md = [metadata(c) for c in co]
        ins = [instructions(c) for c in co]
    names = sorted(set(md[0]) | set(md[1]))
    if a.kernels:
        names = [n for n in names if plain_name(n)[0] in a.kernels]
    bad = 0
    counts = {"text": 0, "mnemonics": 0, "differs": 0}
    print("%-44s %-9s %s" % ("kernel", "code", "  ".join(f.replace("_count", "").replace("_fixed_size", "") for f in FIELDS)))
    for n in names:
        label = "%s%s" % plain_name(n)
        if n not in md[0] or n not in md[1]:
            print("%-44s missing from the %s build" % (label, "old" if n not in md[0] else "new"))
            bad += 1
            continue
        m0, m1 = md[0][n], md[1][n]
        same_md = all(m0.get(f) == m1.get(f) for f in FIELDS)
        i0, i1 = ins[0].get(n, []), ins[1].get(n, [])
        if i0 == i1:
            cls = "text"
        elif [i.split(" ")[0] for i in i0] == [i.split(" ")[0] for i in i1]:
            cls = "mnemonics"
        else:
            cls = "differs"
        counts[cls] += 1
        cols = "  ".join("%d" % m0.get(f, -1) if m0.get(f) == m1.get(f) else "%d->%d" % (m0.get(f, -1), m1.get(f, -1)) for f in FIELDS)
        print("%-44s %-9s %s   %d%s instr%s" % (label, cls, cols, len(i0), "" if cls != "differs" else " -> %d" % len(i1),
                                                "" if same_md else "   METADATA DIFFERS"))
        bad += not same_md
    print("%d kernels: %d identical text, %d identical mnemonics, %d neither; %d with other metadata or missing"
          % (len(names), counts["text"], counts["mnemonics"], counts["differs"], bad))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())

"""Static instruction counts of the p2p engine's device code, from hipcc -S output (no GPU needed).

Per function of a translation unit (kernels and out-of-line device functions): instructions, v_readlane /
v_writelane (reloads and saves of spilled SGPRs), vector memory ops, LDS ops, waits, branches, and the compiler's
resource lines (VGPRs, spilled SGPRs and VGPRs, scratch bytes a lane, LDS bytes).  With --region the translation
unit is compiled with -gline-tables-only and the instructions whose inlining chain passes through the named function
of the named header are counted on their own (for k2_handle: handle_node2, the holder region).

Usage: python scripts/asm_counts.py [--src DIR] [--tu nsgpu_p2p.hip] [--match k2_] [--region nsgpu_p2p_win.h:handle_node2]
DIR is a tree's ns-3-dev-dnemu_amd directory (default: this tree's).  It is a counting tool only."""
import argparse
import os
import re
import subprocess
import sys
import tempfile
from collections import OrderedDict

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FLAGS = "--offload-arch=gfx950 -O3 -ffp-contract=off -fno-fast-math -fPIC -std=c++17 -Wno-unused-function".split()

INSTR = re.compile(r"^\t([a-z][a-z0-9_]+)(\s|$)")
LOC = re.compile(r"^\t\.loc\t(\d+) (\d+) \d+(.*)$")
CHAIN = re.compile(r"([\w./-]+):(\d+):\d+")


def function_lines(path, name):
    """[first, last] source lines of the function template `name` in a header (its closing brace at column 0)."""
    lines = open(path).read().split("\n")
    for i, l in enumerate(lines):
        if re.search(r"\b" + name + r"\(", l) and l.startswith("__device__"):
            for j in range(i, len(lines)):
                if lines[j].startswith("}"):
                    return i + 1, j + 1
    raise SystemExit(f"{name} not found in {path}")


def classify(m):
    if m.startswith(("v_readlane", "v_readfirstlane")):
        return "readlane" if m.startswith("v_readlane") else None
    if m.startswith("v_writelane"):
        return "writelane"
    if m.startswith(("global_", "flat_", "buffer_", "scratch_")):
        return "vmem"
    if m.startswith("ds_"):
        return "lds"
    if m.startswith("s_waitcnt"):
        return "wait"
    if m.startswith(("s_cbranch", "s_branch")):
        return "branch"
    return None


def demangle(names):
    filt = os.path.join(os.path.dirname(os.path.realpath(HIPCC)), "..", "llvm", "bin", "llvm-cxxfilt")
    if not os.path.exists(filt):
        filt = "c++filt"
    out = subprocess.run([filt], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
    return dict(zip(names, out))


def count(src, tu, region):
    with tempfile.TemporaryDirectory() as td:
        asm = os.path.join(td, "tu.s")
        cmd = [HIPCC] + FLAGS + ["-I" + os.path.join(src, "..", "include"), "--cuda-device-only", "-S",
                                 os.path.join(src, "csrc", tu), "-o", asm]
        if region:
            cmd.insert(1, "-gline-tables-only")
        subprocess.run(cmd, check=True, cwd=src)
        text = open(asm).read().split("\n")
    rfile, rlo, rhi = None, 0, 0
    if region:
        rfile, rname = region.split(":")
        rlo, rhi = function_lines(os.path.join(src, "csrc", rfile), rname)
    files, funcs, cur, inreg = {}, OrderedDict(), None, False
    meta, kmeta = {}, {}
    for l in text:
        if l.startswith("\t.file\t"):
            m = re.match(r'\t\.file\t(\d+) (?:"[^"]*" )?"([^"]*)"', l)
            if m:
                files[m.group(1)] = os.path.basename(m.group(2))
            continue
        m = re.match(r"^(_Z\w+):", l)
        if m:
            cur = funcs.setdefault(m.group(1), {"instr": 0, "readlane": 0, "writelane": 0, "vmem": 0, "lds": 0,
                                                "wait": 0, "branch": 0, "r_instr": 0, "r_readlane": 0})
            inreg = False
            continue
        if l.startswith(".Lfunc_end"):
            cur = None
            continue
        m = re.match(r"^(?:  - | {4})\.(\w+):\s*(.*)$", l)
        if m and cur is None:  # the code object's metadata: a kernel's own keys (amdhsa.kernels; not its arguments')
            k, v = m.group(1), m.group(2).strip().strip("'")
            if l.startswith("  - "):
                kmeta = {}
            if k == "name":
                meta[v] = kmeta
            elif k in ("vgpr_count", "sgpr_count", "sgpr_spill_count", "vgpr_spill_count",
                       "private_segment_fixed_size", "group_segment_fixed_size"):
                kmeta[k] = v
            continue
        if cur is None:
            continue
        m = LOC.match(l)
        if m:
            if rfile:
                chain = [(files.get(m.group(1), ""), int(m.group(2)))]
                chain += [(os.path.basename(f), int(n)) for f, n in CHAIN.findall(m.group(3))][1:]
                inreg = any(f == rfile and rlo <= n <= rhi for f, n in chain)
            continue
        m = INSTR.match(l)
        if not m:
            continue
        cur["instr"] += 1
        c = classify(m.group(1))
        if c:
            cur[c] += 1
        if inreg:
            cur["r_instr"] += 1
            cur["r_readlane"] += c == "readlane"
    return funcs, meta


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--src", default=os.path.join(REPO, "ns-3-dev-dnemu_amd"))
    ap.add_argument("--tu", default="nsgpu_p2p.hip")
    ap.add_argument("--match", default="k2_", help="substrings of the demangled names to list, comma separated")
    ap.add_argument("--region", default=None, help="header:function, e.g. nsgpu_p2p_win.h:handle_node2")
    a = ap.parse_args()
    funcs, meta = count(a.src, a.tu, a.region)
    names = demangle(list(funcs))
    subs = a.match.split(",")
    print(f"`{a.tu}`" + (f", region `{a.region}`" if a.region else ""))
    print()
    print("| function | instructions | v_readlane | v_writelane | vector memory | LDS | waits | branches | VGPRs | "
          "SGPRs spilled | VGPRs spilled | scratch B/lane | LDS B |" + (" region instr | region v_readlane |" if a.region else ""))
    print("|---|---|---|---|---|---|---|---|---|---|---|---|---|" + ("---|---|" if a.region else ""))
    for sym, c in funcs.items():
        d = re.sub(r"^void ", "", names[sym]).split("(")[0].replace("nsgpu::", "")
        if not any(s in d for s in subs):
            continue
        k = meta.get(sym, {})
        row = [f"`{d}`", c["instr"], c["readlane"], c["writelane"], c["vmem"], c["lds"], c["wait"], c["branch"],
               k.get("vgpr_count", ""), k.get("sgpr_spill_count", ""), k.get("vgpr_spill_count", ""),
               k.get("private_segment_fixed_size", ""), k.get("group_segment_fixed_size", "")]
        if a.region:
            row += [c["r_instr"], c["r_readlane"]]
        print("| " + " | ".join(str(x) for x in row) + " |")


if __name__ == "__main__":
    sys.exit(main())

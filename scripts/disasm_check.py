"""Compare the gfx950 code of one source file's kernels in two source trees: every kernel of BASE must be, in NEW, the same
instructions with the same resources.

    python scripts/disasm_check.py BASE_CSRC NEW_CSRC SOURCE.hip [--rename OLD=NEW ...] [--resources FILE]

BASE_CSRC is e.g. a checkout of the parent commit's aruco_slam_amd/csrc.  Each tree gets one device-only compile of SOURCE.hip to
assembly with its Makefile's flags and -Rpass-analysis=kernel-resource-usage.  Kernels are matched by demangled name without the
argument list and without `aslam::`; --rename matches BASE's kernel OLD to NEW's kernel NEW, e.g.
    --rename 'k_loc_steps_umap_gated=k_loc_steps<Gated, UncertainMap, FrozenMean>'
Prints a markdown table of NEW's kernels: resources and, against BASE, same / CHANGED (n lines) / new, then BASE's kernels MISSING
from NEW.  A changed kernel whose two instruction lists are equal as multisets gets a line below the table with the positions that
differ and the position of the first s_barrier.  The kernel descriptors (.amdhsa_ lines) are compared apart from the instructions:
a kernel with the same instructions and resources whose descriptor differs is `same` with the differing lines beside it.
--resources writes the compiler's figures of every kernel of both trees to FILE.  Exits 1 if a kernel of BASE changed or is missing."""
import argparse
import collections
import concurrent.futures
import difflib
import os
import re
import subprocess
import sys
import tempfile

ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")
RES = {"TotalSGPRs": "SGPR", "VGPRs": "VGPR", "AGPRs": "AGPR", "ScratchSize [bytes/lane]": "scratch", "LDS Size [bytes/block]": "LDS",
       "SGPRs Spill": "SGPR spill", "VGPRs Spill": "VGPR spill", "Occupancy [waves/SIMD]": "occupancy"}
SAME = ("VGPR", "AGPR", "scratch", "LDS", "SGPR spill", "VGPR spill")


def makefile_flags(csrc):
    """FLAGS of the tree's Makefile with $(ARCH) filled in"""
    mk = open(os.path.join(csrc, "Makefile")).read()
    arch = re.search(r"^ARCH\s*\?=\s*(\S+)", mk, re.M).group(1)
    return re.search(r"^FLAGS\s*=\s*(.*)$", mk, re.M).group(1).replace("$(ARCH)", arch).split()


def compile_source(csrc, source, out):
    """device-only compile to assembly: {demangled name: (instructions, descriptor, resources)} of every function the compiler reports on"""
    asm = os.path.join(out, "out.s")
    r = subprocess.run([f"{ROCM}/bin/hipcc", *makefile_flags(csrc), "--cuda-device-only", "-S", source, "-o", asm,
                        "-Rpass-analysis=kernel-resource-usage"], cwd=csrc, capture_output=True, text=True)
    if r.returncode:
        sys.exit(f"{csrc}/{source} does not compile:\n{r.stderr[-4000:]}")
    res, cur = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"remark: (.*)$", line)
        if not m:
            continue
        t = m.group(1).strip()
        f = re.match(r"Function Name: (\S+)", t)
        if f:
            cur = f.group(1)
            res[cur] = {}
            continue
        for k, short in RES.items():
            if cur and t.startswith(k + ":"):
                res[cur][short] = int(re.match(r"\s*(\d+)", t.split(":")[1]).group(1))
    body, desc, cur = {}, {}, None
    for line in open(asm):
        m = re.match(r"^(\w+):", line)
        if m and m.group(1) in res:
            cur = m.group(1)
            body[cur], desc[cur] = [], []
        elif cur:
            if line.startswith(".Lfunc_end"):
                cur = None
                continue
            t = line.split(";")[0].strip()
            if t.startswith(".amdhsa_"):
                if not t.startswith(".amdhsa_kernel "):                 # (the line that names the kernel)
                    desc[cur].append(t)
            elif t and not t.startswith((".section", ".text", ".p2align", ".end_amdhsa_kernel")):
                t = re.sub(r"\.LBB\d+_", ".LBB_", t)
                body[cur].append(re.sub(r"_Z\w+", "SYM", t))
    syms = list(res)
    dem = subprocess.run(["c++filt"], input="\n".join(syms), capture_output=True, text=True, check=True).stdout.split("\n")
    names = [d.split("(")[0].replace("aslam::", "").replace("void ", "") for d in dem[:len(syms)]]
    twice = [n for n, c in collections.Counter(names).items() if c > 1]
    if twice:
        sys.exit(f"{csrc}/{source}: more than one kernel named {twice}")
    return {n: (body[s], desc[s], res[s]) for n, s in zip(names, syms)}


def figures(r):
    return ", ".join(f"{k} {r.get(k)}" for k in RES.values())


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("base")
    ap.add_argument("new")
    ap.add_argument("source")
    ap.add_argument("--rename", action="append", default=[], metavar="OLD=NEW")
    ap.add_argument("--resources", metavar="FILE")
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as ta, tempfile.TemporaryDirectory() as tb, concurrent.futures.ThreadPoolExecutor(2) as ex:
        fb, fn = ex.submit(compile_source, a.base, a.source, ta), ex.submit(compile_source, a.new, a.source, tb)
        base, new = fb.result(), fn.result()
    renames = dict(r.split("=", 1) for r in a.rename)
    for old in renames:
        if old not in base:
            sys.exit(f"--rename: BASE has no kernel {old}")
    base = {renames.get(n, n): v for n, v in base.items()}
    was = {nw: old for old, nw in renames.items()}
    bad, notes = 0, []
    print(f"`{a.source}`: {len(new)} kernels, {len(base)} in BASE\n")
    print("| kernel | " + " | ".join(SAME) + " | SGPR | instructions | against BASE |")
    print("|---|" + "---|" * (len(SAME) + 3))
    for name in sorted(new):
        ins, dsc, r = new[name]
        row = f"| `{name}` | " + " | ".join(str(r.get(k)) for k in SAME) + f" | {r.get('SGPR')} | {len(ins)} |"
        if name not in base:
            print(row + " new |")
            continue
        bins, bdsc, br = base[name]
        verdict = "same" if name not in was else f"same as `{was[name]}`"
        if dsc != bdsc:
            verdict += "; descriptor: " + ", ".join(f"`{x}` -> `{y.split()[-1]}`" for x, y in zip(bdsc, dsc) if x != y)
        diff = [l for l in difflib.unified_diff(bins, ins, lineterm="", n=0) if l[:1] in "+-" and l[:3] not in ("+++", "---")]
        res_diff = [f"{k} {br.get(k)} -> {r.get(k)}" for k in SAME if br.get(k) != r.get(k)]
        if diff or res_diff:
            bad += 1
            verdict = f"CHANGED ({len(diff)} lines" + (f"; {', '.join(res_diff)}" if res_diff else "") + ")" + (f" from `{was[name]}`" if name in was else "")
            if not res_diff and collections.Counter(bins) == collections.Counter(ins):
                pos = [i for i, (x, y) in enumerate(zip(bins, ins)) if x != y]
                bar = next((i for i, x in enumerate(ins) if x.split()[0] == "s_barrier"), None)
                notes.append(f"- `{name}`: the same instructions as a multiset; positions {pos} differ; first `s_barrier` at {bar}")
        print(row + f" {verdict} |")
    for name in sorted(base):
        if name not in new:
            bad += 1
            print(f"| `{name}` |" + " |" * (len(SAME) + 2) + " MISSING |")
    if notes:
        print("\n" + "\n".join(notes))
    print(f"\n{bad} of BASE's {len(base)} kernels changed or missing")
    if a.resources:
        with open(a.resources, "w") as f:
            f.write(f"-Rpass-analysis=kernel-resource-usage, gfx950, the Makefile's flags: every kernel of {a.source}\n")
            for title, tree in (("BASE", base), ("NEW", new)):
                f.write(f"\n== {title} ==\n")
                for name in sorted(tree):
                    f.write(f"{name}: {figures(tree[name][2])}\n")
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()

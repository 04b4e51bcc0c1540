"""Compare the gfx950 code of ekf.hip's kernels in two source trees: every kernel of BASE must be, in NEW, the same
instructions with the same resources (the solve kernels' FrozenMean instantiations carry one more template argument in their symbol
names, nothing else), and the RunningMean instantiations of NEW are listed beside their frozen twins.

    python scripts/consistent_disasm_check.py BASE_CSRC_DIR NEW_CSRC_DIR        # e.g. a checkout of the parent commit's csrc

Prints a markdown report; exits 1 if a kernel of BASE changed."""
import difflib
import os
import re
import subprocess
import sys
import tempfile

ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")
RES = {"VGPRs": "VGPR", "AGPRs": "AGPR", "ScratchSize [bytes/lane]": "scratch", "LDS Size [bytes/block]": "LDS"}


def compile_ekf(csrc, out):
    """device-only compile of ekf.hip to assembly with the Makefile's flags: (instructions per function, resources per function)"""
    asm = os.path.join(out, "ekf.s")
    r = subprocess.run([f"{ROCM}/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-Wno-unused-function",
                        "-Wno-unused-value", "-Wno-unused-result", "--cuda-device-only", "-S", "ekf.hip", "-o", asm,
                        "-Rpass-analysis=kernel-resource-usage"], cwd=csrc, capture_output=True, text=True, check=True)
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
    body, cur = {}, None
    for line in open(asm):
        m = re.match(r"^(_Z\w+|k_\w+):", line)
        if m:
            cur = m.group(1)
            body[cur] = []
        elif cur:
            if line.startswith(".Lfunc_end"):
                cur = None
                continue
            t = line.split(";")[0].rstrip()
            if t.strip():
                t = re.sub(r"\.LBB\d+_", ".LBB_", t)
                body[cur].append(re.sub(r"_Z\w+", "SYM", t))
    return body, res


def demangle(names):
    out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
    return [o.split("(")[0].replace("aslam::", "").replace("void ", "") for o in out[:len(names)]]


def main():
    base, new = sys.argv[1], sys.argv[2]
    with tempfile.TemporaryDirectory() as a, tempfile.TemporaryDirectory() as b:
        (bb, br), (nb, nr) = compile_ekf(base, a), compile_ekf(new, b)
    bn = dict(zip(demangle(list(br)), br))
    nn = dict(zip([d.replace(", FrozenMean>", ">") for d in demangle(list(nr))], nr))
    bad = 0
    print("| kernel | VGPR | AGPR | scratch B/lane | LDS B | against BASE |")
    print("|---|---|---|---|---|---|")
    for name in sorted(nn):
        r = nr[nn[name]]
        row = f"| `{name}` | {r.get('VGPR')} | {r.get('AGPR')} | {r.get('scratch')} | {r.get('LDS')} |"
        if name in bn:
            same_res = br[bn[name]] == r
            diff = [l for l in difflib.unified_diff(bb[bn[name]], nb[nn[name]], lineterm="", n=0) if l[:1] in "+-" and l[:3] not in ("+++", "---")]
            verdict = "same resources, same instructions" if same_res and not diff else f"CHANGED (resources same: {same_res}, {len(diff)} lines differ)"
            bad += verdict.startswith("CHANGED")
            print(row + f" {verdict} |")
        else:
            print(row + " new |")
    for name in bn:
        if name not in nn:
            bad += 1
            print(f"| `{name}` | | | | | MISSING |")
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()

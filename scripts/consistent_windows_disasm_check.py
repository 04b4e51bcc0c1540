"""Compare the gfx950 code of ekf_window.hip's kernels in two source trees (scripts/consistent_disasm_check.py pointed
at the window source): every kernel of BASE must be, in NEW, the same instructions with the same resources (the step kernel's FrozenMean
instantiations carry one more template argument in their symbol names, nothing else), and the RunningMean instantiations of NEW are
listed beside their frozen twins.

    python scripts/consistent_windows_disasm_check.py BASE_CSRC_DIR NEW_CSRC_DIR [--resources FILE]

Prints a markdown report; --resources also writes the compiler's resource figures of every k_ekf_win_step and k_ekf_win_gate_finish
instantiation of both trees to FILE; exits 1 if a kernel of BASE changed."""
import concurrent.futures
import difflib
import os
import re
import subprocess
import sys
import tempfile

ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")
RES = {"TotalSGPRs": "SGPR", "VGPRs": "VGPR", "AGPRs": "AGPR", "ScratchSize [bytes/lane]": "scratch", "Occupancy [waves/SIMD]": "occupancy",
       "VGPRs Spill": "VGPR spill", "LDS Size [bytes/block]": "LDS"}
SAME = ("VGPR", "AGPR", "scratch", "LDS")


def compile_window(csrc, out):
    """device-only compile of ekf_window.hip to assembly with the Makefile's flags: (instructions per function, resources per function)"""
    asm = os.path.join(out, "ekf_window.s")
    r = subprocess.run([f"{ROCM}/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-Wno-unused-function",
                        "-Wno-unused-value", "-Wno-unused-result", "--cuda-device-only", "-S", "ekf_window.hip", "-o", asm,
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


def figures(r):
    return ", ".join(f"{k} {r.get(k)}" for k in RES.values())


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    base, new = args[0], args[1]
    res_file = sys.argv[sys.argv.index("--resources") + 1] if "--resources" in sys.argv else None
    with tempfile.TemporaryDirectory() as a, tempfile.TemporaryDirectory() as b, concurrent.futures.ThreadPoolExecutor(2) as ex:
        fb, fn = ex.submit(compile_window, base, a), ex.submit(compile_window, new, b)
        (bb, br), (nb, nr) = fb.result(), fn.result()
    bn = dict(zip(demangle(list(br)), br))
    nn = dict(zip([d.replace(", FrozenMean>", ">") for d in demangle(list(nr))], nr))
    bad = 0
    print("| kernel | VGPR | AGPR | scratch B/lane | LDS B | against BASE |")
    print("|---|---|---|---|---|---|")
    for name in sorted(nn):
        r = nr[nn[name]]
        row = f"| `{name}` | {r.get('VGPR')} | {r.get('AGPR')} | {r.get('scratch')} | {r.get('LDS')} |"
        if name in bn:
            same_res = all(br[bn[name]].get(k) == r.get(k) for k in SAME)
            diff = [l for l in difflib.unified_diff(bb[bn[name]], nb[nn[name]], lineterm="", n=0) if l[:1] in "+-" and l[:3] not in ("+++", "---")]
            verdict = "same resources, same instructions" if same_res and not diff else f"CHANGED (resources same: {same_res}, {len(diff)} lines differ)"
            bad += verdict.startswith("CHANGED")
            print(row + f" {verdict} |")
        else:
            twin = name.replace(", RunningMean>", ">")
            print(row + (f" new, beside `{twin}`: {figures(nr[nn[twin]])} |" if twin in nn and twin != name else " new |"))
    for name in bn:
        if name not in nn:
            bad += 1
            print(f"| `{name}` | | | | | MISSING |")
    if res_file:
        with open(res_file, "w") as f:
            f.write("-Rpass-analysis=kernel-resource-usage, gfx950, the Makefile's flags: every k_ekf_win_step and k_ekf_win_gate_finish instantiation\n")
            for title, names, res in (("BASE", bn, br), ("NEW", nn, nr)):
                f.write(f"\n== {title} ==\n")
                for name in sorted(names):
                    if name.startswith(("k_ekf_win_step", "k_ekf_win_gate_finish")):
                        f.write(f"{name}: {figures(res[names[name]])}\n")
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()

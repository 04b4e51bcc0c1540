"""Compare the gfx950 code of the EKF chain kernels of two source trees: every kernel's single-filter
instantiation in NEW must be instruction for instruction the kernel of BASE (symbol names and trailing padding aside); prints the
resource table of both and of the fleet instantiation.

    python scripts/chain_disasm_check.py BASE_CSRC_DIR NEW_CSRC_DIR        # e.g. a checkout of the parent commit's csrc
"""
import os
import re
import subprocess
import sys
import tempfile

ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")
KERNELS = ["k_ekf_plan", "k_ekf_mid", "k_ekf_apply", "k_ekf_mid64", "k_ekf_T", "k_ekf_update_mfma<4>", "k_ekf_update_mfma<5>",
           "k_ekf_gather", "k_ekf_small"]
RES = ["VGPRs", "AGPRs", "ScratchSize [bytes/lane]", "LDS Size [bytes/block]", "SGPRs Spill"]


def compile_ekf(csrc, out, src="ekf.hip"):
    """device-only compile of src (ekf.hip) with the Makefile's flags: (disassembly per function, resource remarks per function)"""
    stem = os.path.splitext(src)[0]
    co, elf = os.path.join(out, stem + ".co"), os.path.join(out, stem + ".elf")
    r = subprocess.run([f"{ROCM}/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-Wno-unused-function",
                        "-Wno-unused-value", "-Wno-unused-result", "--cuda-device-only", "-c", src, "-o", co,
                        "-Rpass-analysis=kernel-resource-usage"], cwd=csrc, capture_output=True, text=True, check=True)
    subprocess.run([f"{ROCM}/llvm/bin/clang-offload-bundler", "--unbundle", "--type=o", f"--input={co}",
                    "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--output={elf}"], check=True)
    dis = subprocess.run([f"{ROCM}/llvm/bin/llvm-objdump", "-d", "--no-show-raw-insn", "--no-leading-addr", elf],
                         capture_output=True, text=True, check=True).stdout
    funcs, cur = {}, None
    for line in dis.splitlines():
        m = re.match(r"^<(.*)>:$", line.strip())
        if m:
            cur = m.group(1)
            funcs[cur] = []
        elif cur and line.startswith("\t"):
            funcs[cur].append(line.split("//")[0].strip())
    for v in funcs.values():
        while v and v[-1] in ("s_nop 0", "..."):
            v.pop()
    res, cur = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = m.group(1)
            res[cur] = {}
            continue
        m = re.search(r"remark:\s+([^:]+): (\S+) \[", line)
        if cur and m:
            res[cur][m.group(1).strip()] = m.group(2)
    return funcs, res


GATED = "8SlamGateE"                     # mangled gate policy of a gated solve kernel; the ungated one has NoSlamGate or none
SOLVE = ["k_ekf_mid", "k_ekf_mid64", "k_ekf_small"]


def symbol(names, kernel, inst=None, gated=False):
    base, _, wct = kernel.partition("<")
    for n in names:
        if re.search(r"\d" + re.escape(base) + r"(I|E)", n) and (not wct or f"Li{wct[0]}E" in n) and (inst is None or inst in n) \
                and (GATED in n) == gated:
            return n
    raise KeyError(kernel)


def main():
    base, new = sys.argv[1], sys.argv[2]
    with tempfile.TemporaryDirectory() as ta, tempfile.TemporaryDirectory() as tb:
        fa, ra = compile_ekf(base, ta)
        fb, rb = compile_ekf(new, tb)
    ok = True
    print("| kernel | before | EkfSingle | EkfFleet | single == before |")
    print("|---|---|---|---|---|")
    for k in KERNELS:
        a, s, f = symbol(fa, k), symbol(fb, k, "EkfSingle"), symbol(fb, k, "EkfFleet")
        same = fa[a] == fb[s]
        ok &= same
        row = lambda r, n: " / ".join(r[n][x] for x in RES) + f" ({len((fa if r is ra else fb)[n])} instr.)"
        print(f"| `{k}` | {row(ra, a)} | {row(rb, s)} | {row(rb, f)} | {'yes' if same else 'NO'} |")
    print("columns: " + " / ".join(RES))
    try:                                                 # the gated instantiations, if NEW has them
        rows = [(f"`{k}` gated", symbol(fb, k, "EkfSingle", True), symbol(fb, k, "EkfFleet", True)) for k in SOLVE]
        rows.append(("`k_ekf_gate_finish`", symbol(fb, "k_ekf_gate_finish", "EkfSingle", True), symbol(fb, "k_ekf_gate_finish", "EkfFleet", True)))
    except KeyError:
        rows = []
    if rows:
        print("\n| kernel | EkfSingle | EkfFleet |\n|---|---|---|")
        for name, s_, f_ in rows:
            cell = lambda n: " / ".join(rb[n][x] for x in RES) + f" ({len(fb[n])} instr.)"
            print(f"| {name} | {cell(s_)} | {cell(f_)} |")
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()

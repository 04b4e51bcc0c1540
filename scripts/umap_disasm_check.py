"""Compare the gfx950 code of the localization kernels of two source trees: the four fixed-map kernels of NEW must be
instruction for instruction those of BASE (trailing padding aside); prints their resource table and that of the four uncertain-map
kernels, as markdown (profiles/umap_disasm_check.md).  The compile and the disassembly are scripts/chain_disasm_check.py's.

    python scripts/umap_disasm_check.py BASE_CSRC_DIR NEW_CSRC_DIR        # e.g. a checkout of the parent commit's csrc
"""
import os
import re
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from chain_disasm_check import RES, compile_ekf  # noqa: E402

FIXED = ["k_loc_steps", "k_loc_steps_gated", "k_fleet_steps", "k_fleet_steps_gated"]
UMAP = ["k_loc_steps_umap", "k_loc_steps_umap_gated", "k_fleet_steps_umap", "k_fleet_steps_umap_gated"]


def symbol(names, kernel):
    for n in names:
        if re.search(r"\d" + re.escape(kernel) + "E", n):
            return n
    raise KeyError(kernel)


def main():
    base, new = sys.argv[1], sys.argv[2]
    with tempfile.TemporaryDirectory() as ta, tempfile.TemporaryDirectory() as tb:
        fa, ra = compile_ekf(base, ta)
        fb, rb = compile_ekf(new, tb)
    row = lambda f, r, n: " / ".join(r[n][x] for x in RES) + f" ({len(f[n])} instr.)"
    ok = True
    print("| kernel | before | after | after == before |")
    print("|---|---|---|---|")
    for k in FIXED:
        a, b = symbol(fa, k), symbol(fb, k)
        same = fa[a] == fb[b]
        ok &= same
        print(f"| `{k}` | {row(fa, ra, a)} | {row(fb, rb, b)} | {'yes' if same else 'NO'} |")
    print()
    print("| new kernel | resources |")
    print("|---|---|")
    for k in UMAP:
        print(f"| `{k}` | {row(fb, rb, symbol(fb, k))} |")
    print()
    print("columns: " + " / ".join(RES) + "; LDS is the static part, the uncertain-map kernels add 72 bytes per landmark at launch")
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()

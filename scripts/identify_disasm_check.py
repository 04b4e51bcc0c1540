"""Compare the gfx950 code of k_identify of two source trees: the production kernel k_identify in NEW must be instruction for
instruction the k_identify of BASE (trailing padding aside).  Prints the resource table of BASE's kernel and of NEW's k_identify
and k_identify_record (the test instrumentation built from the same body, detect_identify.h).

    python scripts/identify_disasm_check.py BASE_CSRC_DIR NEW_CSRC_DIR     # e.g. a checkout of the parent commit's csrc
"""
import os
import re
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from chain_disasm_check import RES, compile_ekf  # noqa: E402


def kernel_symbol(names, kernel):
    for n in names:
        if re.search(r"\d" + re.escape(kernel) + r"E", n):
            return n
    raise KeyError(kernel)


def main():
    base, new = sys.argv[1], sys.argv[2]
    with tempfile.TemporaryDirectory() as ta, tempfile.TemporaryDirectory() as tb:
        fa, ra = compile_ekf(base, ta, "detect.hip")
        fb, rb = compile_ekf(new, tb, "detect.hip")
    a, prod, rec = kernel_symbol(fa, "k_identify"), kernel_symbol(fb, "k_identify"), kernel_symbol(fb, "k_identify_record")
    same = fa[a] == fb[prod]
    row = lambda r, f, n: " / ".join(r[n][x] for x in RES) + f" ({len(f[n])} instr.)"
    print("| kernel | resources |")
    print("|---|---|")
    print(f"| before `{a}` | {row(ra, fa, a)} |")
    print(f"| production `{prod}` | {row(rb, fb, prod)} |")
    print(f"| record `{rec}` | {row(rb, fb, rec)} |")
    print("columns: " + " / ".join(RES))
    print(f"production k_identify identical to before: {'yes' if same else 'NO'}")
    if not same:
        for i, (x, y) in enumerate(zip(fa[a], fb[prod])):
            if x != y:
                print(f"first difference at instruction {i}: {x!r} vs {y!r}")
                break
        else:
            print(f"lengths differ: {len(fa[a])} vs {len(fb[prod])}")
    sys.exit(0 if same else 1)


if __name__ == "__main__":
    main()

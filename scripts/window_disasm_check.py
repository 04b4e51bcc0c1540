"""Compare the gfx950 code of the window kernels of two source trees: every ungated kernel of ekf_window.hip in NEW
must be instruction for instruction the kernel of BASE (symbol names, trailing padding and the pc-relative displacement of a call to
an out-of-line device function aside: that constant is the distance to the callee in the object, which moves when code is added);
prints the resource table of both and of the gated instantiations of k_ekf_win_step and of k_ekf_win_gate_finish.

    python scripts/window_disasm_check.py BASE_CSRC_DIR NEW_CSRC_DIR        # e.g. a checkout of the parent commit's csrc
"""
import re
import sys
import tempfile

from chain_disasm_check import RES, compile_ekf

GATED = "7WinGateE"                      # mangled gate policy of a gated step kernel
STEP = [(T, one) for one in (True, False) for T in (4, 8, 12)]
OTHERS = ["k_ekf_win_thin<4>", "k_ekf_win_thin<8>", "k_ekf_win_thin<12>", "k_ekf_win_fix", "k_ekf_win_gather", "k_ekf_win_next",
          "k_ekf_win_next_gather", "k_ekf_win_next_fix"]


def step_symbol(names, T, one, gated=False):
    for n in names:
        if re.search(r"\d+k_ekf_win_stepILi%dELi2ELb%d" % (T, 1 if one else 0), n) and (GATED in n) == gated:
            return n
    raise KeyError((T, one, gated))


def other_symbol(names, kernel):
    base, _, arg = kernel.partition("<")
    for n in names:
        if re.search(r"\d" + re.escape(base) + r"(I|E)", n) and (not arg or f"ILi{arg[:-1]}E" in n):
            return n
    raise KeyError(kernel)


def without_call_displacements(funcs):
    """the literal of the s_add_u32 that follows an s_getpc_b64 is the distance to a callee: masked"""
    for v in funcs.values():
        for i in range(1, len(v)):
            if v[i - 1].startswith("s_getpc_b64") and v[i].startswith("s_add_u32"):
                v[i] = re.sub(r"0x[0-9a-f]+$", "<pc-relative>", v[i])
    return funcs


def main():
    base, new = sys.argv[1], sys.argv[2]
    with tempfile.TemporaryDirectory() as ta, tempfile.TemporaryDirectory() as tb:
        fa, ra = compile_ekf(base, ta, "ekf_window.hip")
        fb, rb = compile_ekf(new, tb, "ekf_window.hip")
    fa, fb = without_call_displacements(fa), without_call_displacements(fb)
    cell = lambda f, r, n: " / ".join(r[n][x] for x in RES) + f" ({len(f[n])} instr.)"
    ok = True
    print("| kernel | before | after, ungated | same | after, gated |")
    print("|---|---|---|---|---|")
    for T, one in STEP:
        a, b = step_symbol(fa, T, one), step_symbol(fb, T, one)
        same = fa[a] == fb[b]
        ok &= same
        gated = cell(fb, rb, step_symbol(fb, T, one, True)) if one else "(the piece schedule is not gated)"
        print(f"| `k_ekf_win_step<{T}, 2, {'true' if one else 'false'}>` | {cell(fa, ra, a)} | {cell(fb, rb, b)} | {'yes' if same else 'NO'} | {gated} |")
    for k in OTHERS:
        a, b = other_symbol(fa, k), other_symbol(fb, k)
        same = fa[a] == fb[b]
        ok &= same
        print(f"| `{k}` | {cell(fa, ra, a)} | {cell(fb, rb, b)} | {'yes' if same else 'NO'} | |")
    fin = other_symbol(fb, "k_ekf_win_gate_finish")
    print(f"| `k_ekf_win_gate_finish` | | | | {cell(fb, rb, fin)} |")
    print("columns: " + " / ".join(RES))
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()

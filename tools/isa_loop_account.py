"""Instruction accounting of a blend kernel's inner pair loop from `hipcc -S` output.

    python tools/isa_loop_account.py FILE.s KERNEL_SYMBOL_SUBSTRING

Finds the kernel, then the innermost loop that contains `s_ff1_i32_b64` (the live-mask walk of
the pair steps), and counts its instructions by unit (VALU incl. v_exp / DPP, SALU, LDS, VMEM,
branch) and, for VALU, by role using the operand patterns of render_fwd.hip / render_bwd.hip:
  power   gauss_power (v_sub of the pixel offsets, v_mul / v_fmac on the staged conic)
  exp     r3dg_expf (v_med3 clamp, 0x3fb8aa3b log2e, Cody-Waite 0xbf317200 / 0xb5bfbe8e, the
          polynomial constants, v_lshl_add exponent add) or v_exp_f32
  ...     everything else is reported as 'other' with the instruction list, labelled by hand in
          DESIGN.md.
Blocks are counted once each (both instances of the pair and the accumulate branches); the counts per
block tell the pair's main path from the rare blocks the loop also holds (the backward's settle
re-evaluation and inlined flush). The SALU and branch instructions are listed after the VALU ones."""
import re
import sys


def kernel_body(text, sym):
    start = None
    lines = text.splitlines()
    for i, ln in enumerate(lines):
        if start is None and ln.startswith("_Z") and sym in ln and ln.rstrip().endswith(sym.split()[-1] + ":") is False:
            pass
        if start is None and re.match(r"^_Z\S*" + re.escape(sym) + r"\S*:", ln):
            start = i
        elif start is not None and ".end_amdhsa_kernel" in ln:
            return lines[start:i]
    raise SystemExit(f"kernel {sym} not found")


def inner_loop(body):
    """The blocks of the innermost loop that holds `s_ff1_i32_b64`: its header block and every block
    the compiler annotates `in Loop: Header=<header>` (the latch may fall through to the header)."""
    blocks, cur = [], None
    for ln in body:
        m = re.match(r"^(\.LBB\S+):(.*)$", ln) or re.match(r"^; (%bb\.\d+):(.*)$", ln)
        if m:
            cur = [m.group(1), m.group(2), []]
            blocks.append(cur)
        elif cur is not None:
            if not cur[2] and ln.strip().startswith(";") and "Loop" in ln:
                cur[1] += ln
            else:
                cur[2].append(ln)
    # the walk's s_ff1 may sit in the header (a `while (mask)` loop) or in the latch (the pair taken at
    # the loop's end for the next iteration): the first inner loop any of whose blocks holds it
    bb = lambda name: name.lstrip(".").replace("LBB", "BB")  # noqa: E731
    hdr = None
    for name, comment, lines in blocks:
        if not any("s_ff1_i32_b64" in x for x in lines):
            continue
        m = re.search(r"in Loop: Header=(BB\w+)", comment)
        cand = bb(name) if "Inner Loop Header" in comment else m.group(1) if m else None
        if cand and any(bb(n) == cand and "Inner Loop Header" in c for n, c, _ in blocks):
            hdr = cand
            break
    if hdr is None:
        raise SystemExit("no s_ff1 loop found")
    out = []
    for name, comment, lines in blocks:
        if bb(name) == hdr or f"Header={hdr} " in comment + " ":
            out += [f"; block {name}"] + lines
    return out


POWER = re.compile(r"v_(sub|mul|fmac|fma)_f32")
EXP_CONST = ("0x3fb8aa3b", "0xcb400000", "0xbf317200", "0xb5bfbe8e", "0x3ab54ace", "0x3d2aac28", "0x3e2aaa49",
             "0x3efffffe")


def main():
    text = open(sys.argv[1]).read()
    loop = inner_loop(kernel_body(text, sys.argv[2]))
    insts, block_of, blk = [], {}, "?"
    for ln in loop:
        s = ln.strip()
        if s.startswith("; block "):
            blk = s[len("; block "):]
        if not s or s.startswith((";", ".", "/", "s_waitcnt")):
            continue
        block_of[len(insts)] = blk
        insts.append(s)
    units = {"valu": [], "salu": [], "lds": [], "vmem": [], "branch": []}
    per_block = {}
    for i, s in enumerate(insts):
        op = s.split()[0]
        u = ("branch" if op.startswith(("s_cbranch", "s_branch")) else "lds" if op.startswith("ds_")
             else "vmem" if op.startswith(("global_", "buffer_", "flat_")) else "salu" if op.startswith("s_")
             else "valu" if op.startswith("v_") else None)
        if u:
            per_block.setdefault(block_of[i], dict.fromkeys(units, 0))[u] += 1
            units[u].append(s)
    exp = [s for s in units["valu"] if s.startswith(("v_exp_f32", "v_med3_f32", "v_lshl_add_u32"))
           or any(c in s for c in EXP_CONST) or re.match(r"v_fma_f32 \S+, \S+, \S+, 1\.0", s)]
    print(f"loop: {len(insts)} instructions")
    for u, v in units.items():
        print(f"  {u:6s} {len(v)}")
    print(f"  VALU in the exp statement: {len(exp)}")
    print("per block (valu salu lds vmem branch):")
    for b, c in per_block.items():
        print(f"  {b:12s} " + " ".join(f"{c[u]:4d}" for u in units))
    print("VALU listing:")
    for s in units["valu"]:
        print("   ", s)
    # the scalar side of the walk (DESIGN.md §4's SALU table); branches listed with it, as they issue
    # on the scalar unit too
    print("SALU listing:")
    for s in units["salu"]:
        print("   ", s)
    print("branch listing:")
    for s in units["branch"]:
        print("   ", s)


if __name__ == "__main__":
    main()

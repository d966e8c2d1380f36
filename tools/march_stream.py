#!/usr/bin/env python3
"""What one period of a strip march costs in instructions: a histogram of a kernel's main loop, from the compiler's own assembly.

    python tools/march_stream.py gcmf_ringc_zip.hip "gcmf::k_ringcz<double, 9, false, false, true>" [--asm FILE] [--keep FILE] [--top N]

Cross-compiles the translation unit (a name under gcm_filters_amd/csrc/ or a path) to gfx950 assembly with the flags of
gcm_filters_amd/_build.py plus `--cuda-device-only -S` (no GPU needed; minutes for the static-ring units -- `--asm` reads a listing made
earlier, `--keep` saves this one), finds the kernel whose demangled name is the one given (with or without `void ` and the parameter list)
and in it the MAIN LOOP: loops are the ranges from a label to the last branch back to it (the compiler also branches back to rare blocks
it has laid out earlier, a few hundred instructions at most: `--min`, default 1000, leaves those out), an inner loop holds no other; the main
loop is the first inner loop in code order -- in the static-ring kernels the ring period of the fast march, which the compiler lays out
before the nan_to_num redo march.  Prints the loop's instruction count, a histogram by opcode,
the classes DESIGN.md 6 speaks of, every inner loop's size, and the kernel's register / spill metadata.  It is a histogram of whatever is
there, nothing more.
"""
import argparse
import collections
import os
import re
import subprocess
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
LLVM = "/opt/rocm/lib/llvm/bin"

CLASSES = [
    ("f64 arithmetic", r"v_(add|mul|fma|fmac)_f64"),
    ("v_accvgpr_read / write", r"v_accvgpr_"),
    ("DPP / lane moves (v_mov)", r"v_mov_b(32|64)"),
    ("other VALU", r"v_"),
    ("SALU (s_* but branches, waits, nops, loads)", r"s_(?!cbranch|branch|waitcnt|nop|load|buffer_load|barrier|endpgm|setpc|sleep)"),
    ("branches", r"s_(cbranch|branch|setpc)"),
    ("scalar loads", r"s_(load|buffer_load)"),
    ("s_waitcnt", r"s_waitcnt"),
    ("s_nop", r"s_nop"),
    ("vector memory", r"(global|buffer|flat|scratch)_"),
    ("LDS", r"ds_"),
    ("other", r""),
]


def build_flags():
    from gcm_filters_amd import _build
    return _build.hipcc(), list(_build.FLAGS)


def compile_to_asm(unit, out):
    exe, flags = build_flags()
    src = unit if os.path.exists(unit) else os.path.join(REPO, "gcm_filters_amd", "csrc", unit)
    cmd = [exe, *flags, "--cuda-device-only", "-S", src, "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        sys.exit("hipcc failed:\n" + r.stdout + r.stderr)


def demangle(names):
    tool = os.path.join(LLVM, "llvm-cxxfilt")
    r = subprocess.run([tool if os.path.exists(tool) else "c++filt"], input="\n".join(names), capture_output=True, text=True)
    out = r.stdout.splitlines()
    return out if len(out) == len(names) else names


def short(dname):
    return dname.replace("void ", "").split("(")[0].strip()


def kernel_body(lines, mangled):
    """The instruction lines of one function: from its label to its .Lfunc_end."""
    start = next(i for i, l in enumerate(lines) if l.startswith(mangled + ":"))
    end = next(i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end"))
    return lines[start + 1:end]


def parse(body):
    """[(opcode, operands)] and {label: index of the next instruction}."""
    insts, labels = [], {}
    for l in body:
        s = l.split(";")[0].strip()
        if not s or s.startswith("."):
            m = re.match(r"^(\.L\w+):", s)
            if m:
                labels[m.group(1)] = len(insts)
            continue
        m = re.match(r"^([\w.$]+):$", s)
        if m:
            labels[m.group(1)] = len(insts)
            continue
        op, _, rest = s.partition(" ")
        insts.append((op, rest.strip()))
    return insts, labels


def loops(insts, labels, least):
    """Inner loops [(first, last)] of at least `least` instructions, in code order: from a label to the last branch back to it, with no
    other such range inside."""
    last = {}
    for i, (op, rest) in enumerate(insts):
        if op.startswith(("s_cbranch", "s_branch")) and rest in labels and labels[rest] <= i:
            last[labels[rest]] = i
    back = []
    for r in sorted((a, b) for a, b in last.items() if b - a + 1 >= least):
        # (a range that starts inside an earlier one and ends beyond it is no loop: a rare block laid out behind the loop that branches back into it)
        if not any(o[0] < r[0] <= o[1] < r[1] for o in back):
            back.append(r)
    inner = [r for r in back if not any(o != r and r[0] <= o[0] and o[1] <= r[1] for o in back)]
    return sorted(inner)


def metadata(text, mangled):
    import yaml
    m = re.search(r"\.amdgpu_metadata\n(---.*?)\n\.\.\.", text, re.S)
    if not m:
        return {}
    for k in (yaml.safe_load(m.group(1)) or {}).get("amdhsa.kernels", []):
        if k.get(".name") == mangled:
            return {key.lstrip("."): k[key] for key in (".sgpr_count", ".sgpr_spill_count", ".vgpr_count", ".agpr_count", ".vgpr_spill_count",
                                                          ".private_segment_fixed_size", ".group_segment_fixed_size") if key in k}
    return {}


def classify(op):
    for name, pat in CLASSES:
        if re.match(pat, op):
            return name
    return "other"


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("unit", help="translation unit: a name under gcm_filters_amd/csrc/ or a path")
    ap.add_argument("kernel", help="the kernel's demangled name, as check_isa.py -v prints it")
    ap.add_argument("--asm", help="read this assembly listing instead of compiling")
    ap.add_argument("--keep", help="save the assembly listing here")
    ap.add_argument("--min", type=int, default=1000, help="instructions a range must have to count as a loop")
    ap.add_argument("--top", type=int, default=0, help="opcodes to list (0: all)")
    args = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        path = args.asm or args.keep or os.path.join(tmp, "unit.s")
        if not args.asm:
            compile_to_asm(args.unit, path)
        text = open(path).read()
    lines = text.splitlines()
    syms = [m.group(1) for l in lines for m in [re.match(r"^\s*\.amdhsa_kernel\s+(\S+)", l)] if m]
    want = short(args.kernel)
    hits = [s for s, d in zip(syms, demangle(syms)) if short(d) == want]
    if len(hits) != 1:
        sys.exit(f"{len(hits)} kernels named {want!r}; the unit has:\n  " + "\n  ".join(sorted(short(d) for d in demangle(syms))))
    mangled = hits[0]
    insts, labels = parse(kernel_body(lines, mangled))
    inner = loops(insts, labels, args.min)
    if not inner:
        sys.exit("no loop found in the kernel")
    a, b = inner[0]
    loop = insts[a:b + 1]
    print(f"unit    {os.path.basename(args.unit)}")
    print(f"kernel  {want}")
    print("metadata  " + "  ".join(f"{k}={v}" for k, v in metadata(text, mangled).items()))
    print(f"kernel instructions  {len(insts)}")
    print("inner loops (first instruction, instructions)  " + "  ".join(f"{x}:{y - x + 1}" for x, y in inner))
    print(f"main loop  {len(loop)} instructions (from instruction {a})")
    by_class = collections.Counter(classify(op) for op, _ in loop)
    print("\nclass                                         instructions")
    for name, _ in CLASSES:
        if by_class[name]:
            print(f"  {name:44s}{by_class[name]:6d}")
    hist = collections.Counter(op for op, _ in loop)
    print("\nopcode                                        instructions")
    for op, n in sorted(hist.items(), key=lambda t: (-t[1], t[0]))[: args.top or None]:
        print(f"  {op:44s}{n:6d}")
    return 0


if __name__ == "__main__":
    sys.exit(main())

"""Per-kernel comparison of the gfx950 machine code of two builds (CPU only).

    python tools/isa_diff.py PARENT/ex4dgs_amd/csrc ex4dgs_amd/csrc [--files ex4d_attributes ex4d_motion] [--only REGEX] [--show N]

For every kernel of every object both directories hold: whether the instruction stream (mnemonics and operands, in order) is identical,
the two instruction counts and the two VGPR / AGPR counts.  A refactor of a hot kernel that claims "same machine code" is shown, and
re-checked, with this.  --only keeps the instructions whose mnemonic matches REGEX before comparing (e.g. the floating-point and memory
instructions: '_f(16|32|64)|^(global|flat|buffer|ds|scratch)_'); --show prints the first N differing positions of a kernel that differs.
Exit status 1 when some kernel differs or exists on one side only."""
import argparse
import glob
import os
import re
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ex4dgs_amd import isa_check          # noqa: E402


LABEL = re.compile(r"\bL(\d+)\b")


def kernels(obj, only):
    """{kernel symbol: ([instruction text, ...], (vgprs, agprs))} of a host object's code object; {} for host-only objects.  A stretch
    that begins at a branch target begins with the entry "<label>"; the disassembler numbers the labels through the whole file, so branch
    operands are renumbered from the kernel's own lowest one (a kernel must not differ because an earlier one gained a branch)."""
    with tempfile.TemporaryDirectory(prefix="ex4d_isa_") as d:
        co = isa_check.device_code(obj, d)
        if co is None:
            return {}
        regs = isa_check.kernel_registers(co)
        out = {}
        for sym, run in isa_check.disassembly(co):
            if sym in regs:
                text = out.setdefault(sym, ([], regs[sym]))[0]
                text.extend((["<label>"] if text else []) + [t for t in run if only is None or only.search(t.split()[0])])
        for text, _ in out.values():
            base = min((int(n) for t in text for n in LABEL.findall(t)), default=0)
            text[:] = [LABEL.sub(lambda m: f"L{int(m.group(1)) - base}", t) for t in text]
        return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("a", help="csrc directory of the first build (built objects)")
    ap.add_argument("b", help="csrc directory of the second build")
    ap.add_argument("--files", nargs="*", help="object names without .o (default: every object the first directory holds)")
    ap.add_argument("--only", help="compare only the instructions whose mnemonic matches this regular expression")
    ap.add_argument("--show", type=int, default=0, help="print the first N differing positions of each differing kernel")
    args = ap.parse_args()
    only = re.compile(args.only) if args.only else None
    names = args.files or sorted(os.path.basename(p)[:-2] for p in glob.glob(os.path.join(args.a, "*.o")))
    differ = 0
    for name in names:
        ka, kb = (kernels(os.path.join(d, name + ".o"), only) for d in (args.a, args.b))
        for sym in sorted(set(ka) | set(kb)):
            if sym not in ka or sym not in kb:
                differ += 1
                print(f"{name}: {'only in ' + (args.a if sym in ka else args.b):<40} {sym}")
                continue
            (ia, ra), (ib, rb) = ka[sym], kb[sym]
            same = ia == ib
            differ += not same
            na, nb = (sum(t != "<label>" for t in text) for text in (ia, ib))
            print(f"{name}: {'identical' if same else 'DIFFERS  '}  instructions {na:5d} -> {nb:5d}  VGPR {ra[0]:3d} -> {rb[0]:3d}  "
                  f"AGPR {ra[1]:3d} -> {rb[1]:3d}  {sym}")
            if not same and args.show:
                shown = 0
                for i in range(max(len(ia), len(ib))):
                    x, y = (ia[i] if i < len(ia) else "-"), (ib[i] if i < len(ib) else "-")
                    if x != y:
                        print(f"    [{i}] {x}   |   {y}")
                        shown += 1
                        if shown >= args.show:
                            break
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main())

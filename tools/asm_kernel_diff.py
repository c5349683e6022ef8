"""Compare the kernels of two `hipcc -S` outputs of one source file, before and after a refactor.

    hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -fno-fast-math \
        --cuda-device-only -S -o old.s csrc/lba.hip      (the same for the new tree -> new.s)
    python tools/asm_kernel_diff.py old.s new.s [--rename OLD_SYMBOL=NEW_SYMBOL ...] [--show SYMBOL] [--ops]

Per kernel of old.s: `same` when the instruction stream between its label and .Lfunc_end and its
.amdhsa_ descriptor (registers, LDS, scratch) are equal in new.s, `DIFF` with the number of
differing lines otherwise, `gone` when new.s has no such kernel.  Comments are dropped and the
function number in .LBB<fn>_<block> labels is normalised.  Exit status 1 on any DIFF.
--ops adds, per DIFF kernel, the opcodes whose counts differ (s_nop and s_waitcnt apart) and
whether any of them is floating-point: a reordering of the same opcodes shows none.
"""
import argparse
import collections
import difflib
import re
import sys


def kernels(path):
    body, desc, cur, in_desc = {}, {}, None, None
    for line in open(path):
        m = re.match(r"^(\w+):\s*(;.*)?$", line)
        if m and not line.startswith(".L") and cur is None and in_desc is None:
            cur = m.group(1)
            body[cur] = []
            continue
        if cur is not None and re.match(r"^\.Lfunc_end\d+:", line):
            cur = None
            continue
        m = re.match(r"^\s*\.amdhsa_kernel\s+(\w+)", line)
        if m:
            in_desc = m.group(1)
            desc[in_desc] = []
            continue
        if line.strip() == ".end_amdhsa_kernel":
            in_desc = None
            continue
        text = re.sub(r";.*", "", line)
        text = re.sub(r"\.L(BB|tmp|func_begin|func_end)\d+", r".L\1", text).strip()
        if not text:
            continue
        if in_desc is not None:
            desc[in_desc].append(text)
        elif cur is not None:
            body[cur].append(text)
    return {k: (body[k], desc[k]) for k in body if k in desc}  # kernels only (they have a descriptor)


def main(argv):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--rename", action="append", default=[], metavar="OLD=NEW")
    ap.add_argument("--show", metavar="SYMBOL", help="print this kernel's differing lines")
    ap.add_argument("--ops", action="store_true", help="per DIFF kernel: the opcodes whose counts differ")
    opt = ap.parse_args(argv)
    rename, show = dict(r.split("=") for r in opt.rename), opt.show
    old, new = kernels(opt.old), kernels(opt.new)
    bad = 0
    for k, (b0, d0) in old.items():
        k1 = rename.get(k, k)
        if k1 not in new:
            print(f"gone  {k}")
            continue
        b1, d1 = new[k1]
        b0 = [x.replace(k, k1) for x in b0]
        nb = sum(1 for x in difflib.ndiff(b0, b1) if x[0] in "+-") if b0 != b1 else 0
        nd = sum(1 for x, y in zip(d0, d1) if x != y) + abs(len(d0) - len(d1))
        bad += bool(nb or nd)
        print(f"{'DIFF' if nb or nd else 'same'}  {k1}  {len(b1)} instructions"
              + (f"  body lines differing: {nb}, descriptor lines: {nd}" if nb or nd else ""))
        if opt.ops and (nb or nd):
            c0, c1 = (collections.Counter(re.sub(r"_e(32|64)$", "", x.split()[0]) for x in b if x[0] != "." and x[-1] != ":") for b in (b0, b1))
            ops = sorted(o for o in c0.keys() | c1.keys() if c0[o] != c1[o] and o not in ("s_nop", "s_waitcnt"))
            fp = [o for o in ops if re.search(r"_f(16|32|64)", o)]
            print("      opcode counts differing: " + (", ".join(f"{o} {c0[o]}->{c1[o]}" for o in ops) or "none"))
            print("      floating-point opcodes among them: " + (", ".join(fp) or "none"))
        if show == k1:
            print("\n".join(x for x in difflib.unified_diff(b0 + d0, b1 + d1, lineterm="", n=0)))
    for k in new:
        if k not in old and k not in rename.values():
            print(f"new   {k}")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))

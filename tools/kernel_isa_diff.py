"""Do the kernels of one source file compile to the same instructions in two builds?  (k_seqdp's DTW, Frechet and
ERP instantiations before and after MSM and TWE joined the kernel.)

  hipcc <the flags of annchor_amd/build.py> --cuda-device-only -S annchor_amd/csrc/seqdp.hip -o new.s      (and the same on the
                                                                                                            parent's file: old.s)
  python tools/kernel_isa_diff.py old.s new.s [--prefix _Z7k_seqdp]

Every kernel of old.s whose name starts with the prefix is looked up in new.s and its instruction stream compared line by line,
comments, labels and directives aside (a branch target is compared by its block number within the kernel).  A kernel whose only differences are immediates of `s_load_dword*` / `s_add_u32` on the
kernel-argument pointer -- offsets of hidden arguments, which move when the argument struct grows -- counts as the same; the
distinct (old, new) pairs of such lines are printed so that they can be read.  Exit status 1 if a kernel is missing or differs
otherwise.  Kernels that only new.s has are counted."""
import argparse
import re
import sys

# a branch target is .LBB<number of the function in the file>_<block>: the first number moves when kernels are instantiated ahead
BLOCK = re.compile(r"\.LBB\d+_(\d+)")
OFFSET = re.compile(r"^((?:s_load_dword\S*|s_add_u32)\s+\S+,\s*(?:s\[\d+:\d+\]|s\d+),\s*)0x[0-9a-f]+$")


def offset_only(x, y):
    mx, my = OFFSET.match(x), OFFSET.match(y)
    return bool(mx and my and mx.group(1) == my.group(1))


def kernels(path, prefix):
    """name -> instruction lines, label .. .Lfunc_end."""
    out, cur = {}, None
    for line in open(path):
        m = re.match(r"^(%s\S*):" % re.escape(prefix), line)
        if m:
            cur = out.setdefault(m.group(1), [])
            continue
        if cur is None:
            continue
        text = line.split(";")[0].strip()
        if text.startswith(".Lfunc_end"):
            cur = None
        elif text and not text.startswith(".") and not text.endswith(":"):
            cur.append(BLOCK.sub(r".LBB_\1", text))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--prefix", default="_Z7k_seqdp")
    args = ap.parse_args()
    old, new = kernels(args.old, args.prefix), kernels(args.new, args.prefix)
    same, moved, bad = 0, set(), []
    for name, a in old.items():
        b = new.get(name)
        if b is None:
            bad.append((name, "missing from %s" % args.new))
        elif a == b:
            same += 1
        else:
            first = next((k for k, (x, y) in enumerate(zip(a, b)) if x != y and not offset_only(x, y)), None)
            if first is None and len(a) == len(b):
                same += 1
                moved.update((x, y) for x, y in zip(a, b) if x != y)
            else:
                first = min(len(a), len(b)) if first is None else first
                bad.append((name, "%d against %d instructions, first difference at instruction %d: %s"
                            % (len(a), len(b), first, " | ".join(v[first] for v in (a, b) if first < len(v)))))
    print("%d kernels in %s, %d in %s (%d only there)" % (len(old), args.old, len(new), args.new, len(set(new) - set(old))))
    print("%d the same instruction for instruction" % same + (", kernel-argument offsets aside:" if moved else ""))
    for x, y in sorted(moved):
        print("    %-40s -> %s" % (x, y))
    for name, why in bad:
        print("DIFFERENT %s: %s" % (name, why))
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()

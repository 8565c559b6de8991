"""Compare the kernels of two builds of the same translation units, from their device assembly.

usage: python scripts/compare_kernel_asm.py [--summary] PARENT_DIR CHANGE_DIR
Each directory holds one <unit>.s per translation unit (the Makefile's compile line of the unit plus
--cuda-device-only -S).  For every kernel of CHANGE_DIR/<unit>.s the script looks up the kernel of the same name in
PARENT_DIR/<unit>.s and compares
  * the instruction stream: the lines between the kernel's label and its .Lfunc_end, without comments and directives,
    with the function number in .LBB<n>_<m> labels dropped (it counts the functions before the kernel in the file);
  * the .amdhsa_ resource block (registers, scratch, LDS, ...), line by line.
It prints one line per kernel and a total, and exits with status 1 if a kernel is missing from the parent or differs.
Kernels that only the parent has are counted (the change compiles fewer), not listed.
With --summary, a kernel that differs is followed by what moved, parent -> change: the instruction counts, the
opcodes whose counts differ and the .amdhsa_ lines that differ.  The verdict lines and the exit status are the same."""
import collections
import os
import re
import sys


def kernels(path):
    """{kernel: (instruction lines, .amdhsa_ lines)} of one device assembly file."""
    body, res, cur, hsa = {}, {}, None, None
    for line in open(path):
        t = line.split(";")[0].strip()
        m = re.match(r"^\.amdhsa_kernel (\S+)$", t)  # (the block sits before the kernel's .Lfunc_end)
        if m:
            hsa = m.group(1)
            res[hsa] = []
        elif t == ".end_amdhsa_kernel":
            hsa = None
        elif hsa is not None:
            if t.startswith(".amdhsa_"):
                res[hsa].append(" ".join(t.split()))
        elif cur is None:
            m = re.match(r"^(_Z\w+):$", t)
            if m:
                cur = m.group(1)
                body[cur] = []
        elif t.startswith(".Lfunc_end"):
            cur = None
        elif t and (not t.startswith(".") or re.match(r"^\.LBB\w+:$", t)):
            body[cur].append(re.sub(r"\.LBB\d+_", ".LBB_", t))
    return {k: (body[k], res[k]) for k in res if k in body}


def opcodes(body):
    return collections.Counter(l.split()[0] for l in body if not l.endswith(":"))


def summary(old, new):
    """Lines that say how two (instruction lines, .amdhsa_ lines) differ."""
    a, b = opcodes(old[0]), opcodes(new[0])
    out = [f"    instructions {sum(a.values())} -> {sum(b.values())}"]
    moved = [f"{op} {a[op]} -> {b[op]}" for op in sorted(set(a) | set(b)) if a[op] != b[op]]
    out += ["    opcodes      " + (", ".join(moved) if moved else "the same histogram, another order or operands")]
    ra, rb = dict(l.split(None, 1) for l in old[1]), dict(l.split(None, 1) for l in new[1])
    out += [f"    {k} {ra.get(k, '-')} -> {rb.get(k, '-')}" for k in sorted(set(ra) | set(rb)) if ra.get(k) != rb.get(k)]
    return out


def main():
    args = [a for a in sys.argv[1:] if a != "--summary"]
    if len(args) != 2:
        raise SystemExit(__doc__)
    parent_dir, change_dir = args
    want_summary = "--summary" in sys.argv[1:]
    n = same = dropped = 0
    for unit in sorted(f for f in os.listdir(change_dir) if f.endswith(".s")):
        new = kernels(os.path.join(change_dir, unit))
        old = kernels(os.path.join(parent_dir, unit))
        dropped += len(set(old) - set(new))
        for name in sorted(new):
            n += 1
            if name not in old:
                verdict = "NOT IN PARENT"
            else:
                code = new[name][0] == old[name][0]
                regs = new[name][1] == old[name][1]
                verdict = "same" if code and regs else " ".join(
                    (["CODE DIFFERS"] if not code else []) + (["RESOURCES DIFFER"] if not regs else []))
                same += code and regs
            print(f"{unit[:-2]:9s} {len(new[name][0]):6d} instr  {verdict:13s} {name}")
            if want_summary and name in old and verdict != "same":
                print("\n".join(summary(old[name], new[name])))
    print(f"total: {n} kernels in the change, {same} the same as in the parent, {n - same} differ or are new; "
          f"{dropped} kernels of the parent no longer compiled")
    sys.exit(0 if n and same == n else 1)


if __name__ == "__main__":
    main()

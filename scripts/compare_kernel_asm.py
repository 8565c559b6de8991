r"""Compare the kernels of two builds of the same translation units, from their device assembly.

usage: python scripts/compare_kernel_asm.py [--summary] [--pair P=C ...] [--mask-kernarg] PARENT_DIR CHANGE_DIR
Each directory holds one <unit>.s per translation unit (the Makefile's compile line of the unit plus
--cuda-device-only -S).  For every kernel of CHANGE_DIR/<unit>.s the script looks up the kernel of the same name in
PARENT_DIR/<unit>.s and compares
  * the instruction stream: the lines between the kernel's label and its .Lfunc_end, without comments and directives,
    with the function number in .LBB<n>_<m> labels dropped (it counts the functions before the kernel in the file);
  * the .amdhsa_ resource block (registers, scratch, LDS, ...), line by line.
It prints one line per kernel and a total, and exits with status 1 if a kernel is missing from the parent or differs.
Kernels that only the parent has are counted (the change compiles fewer), not listed.
With --summary, a kernel that differs is followed by what moved, parent -> change: the instruction counts, the
opcodes whose counts differ and the .amdhsa_ lines that differ.  The verdict lines and the exit status are the same.

For a change that renames kernels or gives them other arguments (the mangled name holds both):
  --pair PARENT_REGEX=CHANGE_REGEX  (repeatable) a kernel of the change that has no namesake and that CHANGE_REGEX
      matches is compared with the one kernel of the parent that PARENT_REGEX matches with the same groups, e.g.
      --pair '20pmmh_adaptive_kernelI((?:Li\d+E)+)EEv=11pmmh_kernelI((?:Li\d+E)+)Lb1EEEv' (mangled names: a kernel
      that became the <.., true> instantiation of another template); its line is followed by the parent's name.
  --mask-kernarg  a kernel that differs from its parent only in the offset operands of its scalar loads from the
      kernarg segment pointer and in .amdhsa_kernarg_size (a longer or reordered argument list moves these and nothing
      else) gets the verdict `same but kernarg` and counts as passing; the total names the two counts apart."""
import argparse
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


def partner(name, old, pairs):
    """The parent's kernel for the change's kernel `name`: the one of that name, else, for the first --pair whose
    CHANGE_REGEX matches `name`, the one parent kernel that its PARENT_REGEX matches with the same groups."""
    if name in old:
        return name
    for parent_re, change_re in pairs:
        m = change_re.search(name)
        if m:
            found = [k for k in old if (p := parent_re.search(k)) and p.groups() == m.groups()]
            return found[0] if len(found) == 1 else None
    return None


def mask_kernarg(kernel):
    """(instruction lines, .amdhsa_ lines) without what the length and order of the kernel's argument list decide: the
    offset operand of the scalar loads from the kernarg segment pointer (the user SGPR pair that follows the private
    segment buffer, the dispatch pointer and the queue pointer, as the .amdhsa_user_sgpr_ lines enable them) and the
    .amdhsa_kernarg_size line."""
    body, res = kernel
    on = {k: v for k, v in (l.split(None, 1) for l in res)}
    first = 4 * int(on.get(".amdhsa_user_sgpr_private_segment_buffer", 0)) + \
        2 * int(on.get(".amdhsa_user_sgpr_dispatch_ptr", 0)) + 2 * int(on.get(".amdhsa_user_sgpr_queue_ptr", 0))
    load = re.compile(rf"^(s_load_\w+\s+\S+,\s*s\[{first}:{first + 1}\]),\s*\S+$")
    return ([load.sub(r"\1, <kernarg>", l) for l in body],
            [l for l in res if not l.startswith(".amdhsa_kernarg_size ")])


def main():
    ap = argparse.ArgumentParser(usage=__doc__)
    ap.add_argument("--summary", action="store_true")
    ap.add_argument("--pair", action="append", default=[], metavar="PARENT_REGEX=CHANGE_REGEX")
    ap.add_argument("--mask-kernarg", action="store_true")
    ap.add_argument("parent_dir")
    ap.add_argument("change_dir")
    args = ap.parse_args()
    pairs = [tuple(re.compile(r) for r in p.split("=", 1)) for p in args.pair]
    n = same = kernarg = dropped = 0
    for unit in sorted(f for f in os.listdir(args.change_dir) if f.endswith(".s")):
        new = kernels(os.path.join(args.change_dir, unit))
        old = kernels(os.path.join(args.parent_dir, unit))
        mate = {name: partner(name, old, pairs) for name in new}
        dropped += len(set(old) - set(mate.values()))
        for name in sorted(new):
            n += 1
            was = old.get(mate[name])
            if was is None:
                verdict = "NOT IN PARENT"
            else:
                code, regs = new[name][0] == was[0], new[name][1] == was[1]
                verdict = "same" if code and regs else " ".join(
                    (["CODE DIFFERS"] if not code else []) + (["RESOURCES DIFFER"] if not regs else []))
                same += code and regs
                if args.mask_kernarg and verdict != "same" and mask_kernarg(new[name]) == mask_kernarg(was):
                    verdict = "same but kernarg"
                    kernarg += 1
            print(f"{unit[:-2]:9s} {len(new[name][0]):6d} instr  {verdict:13s} {name}")
            if was is not None and mate[name] != name:
                print(f"    parent: {mate[name]}")
            if args.summary and was is not None and verdict != "same":
                print("\n".join(summary(was, new[name])))
    ok = same + kernarg
    print(f"total: {n} kernels in the change, {same} the same as in the parent, " +
          (f"{kernarg} the same but for kernarg offsets and size, " if args.mask_kernarg else "") +
          f"{n - ok} differ or are new; {dropped} kernels of the parent no longer compiled")
    sys.exit(0 if n and ok == n else 1)


if __name__ == "__main__":
    main()

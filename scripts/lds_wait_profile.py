"""Where a kernel's pair loop waits for the LDS: every `s_waitcnt lgkmcnt(n)` of the loop, from the device assembly.

usage: python scripts/lds_wait_profile.py UNIT.s KERNEL [--loop LABEL] [--latency CYCLES]
UNIT.s is a unit's device assembly (the Makefile's compile line of the unit plus --cuda-device-only -S); KERNEL is a
regular expression matched against the demangled kernel name in the short form of scripts/kernel_resources.py, e.g.
'flow5::bwd2_kernel<0,1,1,1,0>'.  Runs on a CPU host; nothing is compiled or run.

The loop: the innermost loop (the compiler's "in Loop: Header=" block comments) that holds the most MFMAs, unless
--loop names a header label (BB4_22).  Its blocks are walked in execution order -- from the header down, then the
latch blocks the compiler placed above the header -- twice, so that the operations in flight across the back edge are
known; the second walk is the one reported.  Branches inside the loop are not followed: the walk is the straight line
through every block.

For each wait the table gives
  * the operation it releases: the youngest LDS (or scalar-memory) operation that must have returned for the
    counter to reach n -- a wave's LDS operations return in order, so it is the one the wave waits longest for;
  * the issue cycles between that operation and the wait (VALU 4, transcendental 8, MFMA 8 per instruction, the
    counting of DESIGN.md §4.1; other instructions 0) and the instructions between them;
  * the first later instruction that reads the operation's destination registers, and whether it is an MFMA.
A wait that finds the counter at n already releases nothing ("-").  Only waits and LDS / scalar-memory operations are
interpreted; everything else is classed by its mnemonic alone.

Totals: the waits by n; the "exposed" sites -- an LDS read released by a wait with fewer than --latency (default 64)
issue cycles behind it whose next consumer is an MFMA -- and the issue cycles by which all waits on LDS reads fall
short of that latency; and a modelled stall: the walk keeps an issue clock, every LDS operation is back --latency
cycles after its issue (never before an older one), and a wait moves the clock to the return of the operation it
releases.  That is what one wave alone would stand parked; how much of it the partner wave on the SIMD hides is for
the counters to say (SQ_WAIT_ANY).
"""
import argparse
import re
import subprocess

TRANS = ("v_exp_", "v_log_", "v_rcp_", "v_rsq_", "v_sqrt_", "v_sin_", "v_cos_")
NO_DEST = ("ds_write", "ds_add", "ds_max", "ds_min", "global_store", "buffer_store", "scratch_store", "flat_store",
           "v_cmp", "v_cmpx", "s_")


def demangle(names):
    for tool in ("/opt/rocm/llvm/bin/llvm-cxxfilt", "llvm-cxxfilt", "c++filt"):
        try:
            return subprocess.run([tool], input="\n".join(names), capture_output=True, text=True,
                                  check=True).stdout.splitlines()
        except (OSError, subprocess.CalledProcessError):
            continue
    return list(names)


def short(name):
    name = re.sub(r"^void\s+", "", name)
    depth, end = 0, len(name)
    for i, ch in enumerate(name):
        depth += ch == "<"
        depth -= ch == ">"
        if ch == "(" and depth == 0:
            end = i
            break
    return name[:end].replace("vissm::", "").replace("false", "0").replace("true", "1").replace(", ", ",")


def kernel_lines(path, pattern):
    """(mangled name, [(line number, text)]) of the one kernel whose short demangled name matches."""
    lines = open(path).read().splitlines()
    starts = [(i, m.group(1)) for i, l in enumerate(lines) for m in [re.match(r"^(_Z\w+):", l)] if m]
    names = [short(d) for d in demangle([n for _, n in starts])]
    hits = [(i, n) for (i, n), s in zip(starts, names) if re.search(pattern, s) or re.search(pattern, n)]
    if len(hits) != 1:
        raise SystemExit(f"{len(hits)} kernels match {pattern!r}: " + ", ".join(
            s for s in names if re.search(pattern, s)) + " (of " + ", ".join(names) + ")" * (not hits))
    i, name = hits[0]
    body = []
    for j in range(i + 1, len(lines)):
        if lines[j].startswith(".Lfunc_end"):
            break
        body.append((j + 1, lines[j]))
    return name, body


def blocks_of(body):
    """[(label, loop header or None, [(line number, instruction text)])] in file order."""
    blocks = [("entry", None, [])]
    for k, (no, line) in enumerate(body):
        m = re.match(r"^\.L(BB\d+_\d+):\s*(?:;(.*))?$", line)
        if m:
            label, note = m.group(1), m.group(2) or ""
            for _, more in body[k + 1:]:  # the note's continuation lines: comments only
                if not more.strip().startswith(";"):
                    break
                note += more
            h = re.search(r"in Loop: Header=(BB\d+_\d+)", note)
            header = h.group(1) if h else (label if "Loop Header" in note else None)
            blocks.append((label, header, []))
            continue
        t = line.split(";")[0].strip()
        if t and not t.startswith(".") and not t.endswith(":"):
            blocks[-1][2].append((no, t))
    return blocks


def regs(operand):
    """The set of vector registers ('v5', 'a3') an operand names."""
    out = set()
    for f, lo, hi in re.findall(r"\b([va])\[(\d+):(\d+)\]", operand):
        out |= {f + str(i) for i in range(int(lo), int(hi) + 1)}
    for f, n in re.findall(r"\b([va])(\d+)\b", operand):
        out.add(f + n)
    return out


def split_inst(text):
    mnem, _, rest = text.partition(" ")
    ops = [o.strip() for o in rest.split(",")] if rest.strip() else []
    return mnem, ops


def cost(mnem):
    if mnem.startswith(("v_mfma", "v_smfmac")):
        return 8
    if mnem.startswith(TRANS):
        return 8
    return 4 if mnem.startswith("v_") else 0


def consumer(stream, start, dest):
    """The first instruction after index `start` that reads a register of `dest` (before it is overwritten)."""
    live = set(dest)
    for no, text in stream[start + 1:]:
        mnem, ops = split_inst(text)
        has_dest = bool(ops) and not mnem.startswith(NO_DEST)
        src = set().union(*[regs(o) for o in (ops[1:] if has_dest else ops)]) if ops else set()
        if src & live:
            return no, mnem
        if has_dest:
            live -= regs(ops[0])
            if not live:
                return None
    return None


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("asm")
    ap.add_argument("kernel")
    ap.add_argument("--loop", default="", help="header label of the loop to read (default: the innermost with most MFMAs)")
    ap.add_argument("--latency", type=int, default=64, help="LDS read latency in cycles for the totals (default 64)")
    args = ap.parse_args()
    name, body = kernel_lines(args.asm, args.kernel)
    blocks = blocks_of(body)
    count = {}
    for _, header, insts in blocks:
        if header:
            count[header] = count.get(header, 0) + sum(t.startswith("v_mfma") for _, t in insts)
    if not count:
        raise SystemExit("the kernel has no loop")
    header = args.loop or max(count, key=count.get)
    idx = [i for i, b in enumerate(blocks) if b[1] == header]
    hpos = next(i for i in idx if blocks[i][0] == header)
    order = [i for i in idx if i >= hpos] + [i for i in idx if i < hpos]
    once = [inst for i in order for inst in blocks[i][2]]
    n1 = len(once)
    stream = once + once + once  # walk 1 primes the queue, walk 2 is reported, walk 3 holds late consumers

    mix = {"VALU": 0, "trans": 0, "MFMA": 0, "LDS": 0, "waits on lgkmcnt": 0, "s_nop": 0, "scratch": 0, "other": 0}
    for _, t in once:
        m = t.split(" ")[0]
        k = ("MFMA" if m.startswith("v_mfma") else "trans" if m.startswith(TRANS) else "VALU" if m.startswith("v_")
             else "LDS" if m.startswith("ds_") else "waits on lgkmcnt" if m == "s_waitcnt" and "lgkmcnt" in t
             else "s_nop" if m == "s_nop" else "scratch" if m.startswith("scratch_") else "other")
        mix[k] += 1

    queue, rows = [], []  # queue: stream indices of the operations the counter still counts
    clock, back, last_back = 0, {}, 0  # the stall model: issue clock, return time of each operation (in order)
    for i, (no, text) in enumerate(stream[:2 * n1]):
        mnem, ops = split_inst(text)
        clock += cost(mnem)
        if mnem.startswith("ds_") or mnem.startswith(("s_load", "s_buffer_load")):
            queue.append(i)
            back[i] = last_back = max(clock + args.latency, last_back)
            continue
        m = re.search(r"lgkmcnt\((\d+)\)", text) if mnem == "s_waitcnt" else None
        if not m:
            continue
        n = int(m.group(1))
        released = queue[:len(queue) - n] if len(queue) > n else []
        queue = queue[len(queue) - n:] if n else []
        if i < n1:
            if released:
                clock = max(clock, back[released[-1]])
            continue
        row = {"line": no, "n": n, "op": None, "stall": 0}
        if released:
            j = released[-1]
            row["stall"] = max(0, back[j] - clock)
            clock = max(clock, back[j])
            jm, jops = split_inst(stream[j][1])
            between = stream[j + 1:i]
            dest = regs(jops[0]) if jops and jm.startswith("ds_read") else set()
            use = consumer(stream, i, dest) if dest else None
            row.update(op=jm, op_line=stream[j][0], dest=jops[0] if dest else "", ninst=len(between),
                       cycles=sum(cost(t.split(" ")[0]) for _, t in between), use=use, read=bool(dest),
                       nrel=len(released))
        rows.append(row)

    print(f"# {args.asm.split('/')[-1]}: {short(demangle([name])[0])}")
    print(f"# loop {header}: {n1} instructions -- " + ", ".join(f"{v} {k}" for k, v in mix.items()))
    print("wait@line  n  released operation (line, destination)                 ops  instr  cycles  stall  next consumer")
    for r in rows:
        head = f"{r['line']:9d} {r['n']:2d}  "
        if r["op"] is None:
            print(head + "-")
            continue
        use = "-" if not r["read"] else "none in the loop" if r["use"] is None else (
            f"{r['use'][1]} @{r['use'][0]}" + ("  MFMA" if r["use"][1].startswith("v_mfma") else ""))
        print(head + f"{r['op']:22s} @{r['op_line']:<6d} {r['dest']:14s} {r['nrel']:5d} {r['ninst']:6d} {r['cycles']:7d} {r['stall']:6d}  {use}")

    by_n = {}
    for r in rows:
        by_n[r["n"]] = by_n.get(r["n"], 0) + 1
    reads = [r for r in rows if r["op"] and r["read"]]
    mfma = [r for r in reads if r["use"] and r["use"][1].startswith("v_mfma")]
    exposed = [r for r in mfma if r["cycles"] < args.latency]
    exposed0 = [r for r in exposed if r["n"] == 0]
    print("totals")
    print(f"  waits on lgkmcnt: {len(rows)} (" + ", ".join(f"lgkmcnt({n}): {by_n[n]}" for n in sorted(by_n)) + ")")
    print(f"  waits that release an LDS read: {len(reads)}; next consumer an MFMA: {len(mfma)}")
    print(f"  exposed sites (LDS read -> wait -> MFMA, fewer than {args.latency} issue cycles between): {len(exposed)}, "
          f"of them at lgkmcnt(0): {len(exposed0)}")
    print(f"  modelled stall (every LDS operation back {args.latency} cycles after its issue, in order; one wave alone): "
          f"{sum(r['stall'] for r in rows)} cycles, before an MFMA: {sum(r['stall'] for r in mfma)}")
    print(f"  issue cycles short of {args.latency} over all waits on LDS reads: "
          f"{sum(max(0, args.latency - r['cycles']) for r in reads)} "
          f"(before an MFMA: {sum(max(0, args.latency - r['cycles']) for r in mfma)})")


if __name__ == "__main__":
    main()

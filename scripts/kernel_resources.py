"""Register, scratch and LDS use of every kernel instantiation of one translation unit of libvissm.

Compiles the unit's device code for gfx950 with the command line the Makefile uses for its object file (taken from
`make -n`, so per-file flags such as -fno-slp-vectorize or the register-pressure trackers are the build's own), plus
-Rpass-analysis=kernel-resource-usage, and prints the compiler's remarks as one table row per kernel.  Runs on a CPU
host; nothing is linked or run.

usage: python scripts/kernel_resources.py flow_v5.hip [--filter REGEX] [--make-arg VAR=VALUE ...]
(`make -C viforssms_amd/csrc resources` writes the tables of the four flow_v5 units to profiles/r08/resources/)
"""
import argparse
import os
import re
import shlex
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "viforssms_amd", "csrc")
FIELDS = (("VGPRs", "VGPRs"), ("AGPRs", "AGPRs"), ("ScratchSize [bytes/lane]", "scratch B/lane"),
          ("VGPRs Spill", "VGPR spill"), ("SGPRs Spill", "SGPR spill"), ("TotalSGPRs", "SGPRs"),
          ("Occupancy [waves/SIMD]", "occupancy"), ("LDS Size [bytes/block]", "LDS B/block"))


def compile_command(unit, make_args):
    """The Makefile's compile line for build/<unit>.o (make -n, with the source marked as changed)."""
    obj = "build/" + os.path.splitext(unit)[0] + ".o"
    out = subprocess.run(["make", "-C", CSRC, "-n", "-W", unit, obj] + make_args, check=True, capture_output=True,
                         text=True).stdout
    lines = [l for l in out.splitlines() if " -c " in l and unit in l]
    if not lines:
        raise SystemExit(f"no compile line for {obj} in `make -n`:\n{out}")
    return shlex.split(lines[-1])


def demangle(names):
    for tool in ("/opt/rocm/llvm/bin/llvm-cxxfilt", "llvm-cxxfilt", "c++filt"):
        try:
            out = subprocess.run([tool], input="\n".join(names), capture_output=True, text=True, check=True).stdout
            return out.splitlines()
        except (OSError, subprocess.CalledProcessError):
            continue
    return list(names)


def short(name):
    """vissm::flow5::bwd2_kernel<false, true, ...>(args) -> flow5::bwd2_kernel<0,1,...>"""
    name = re.sub(r"^void\s+", "", name)
    depth, end = 0, len(name)
    for i, ch in enumerate(name):  # cut the argument list: the first '(' outside the template brackets
        depth += ch == "<"
        depth -= ch == ">"
        if ch == "(" and depth == 0:
            end = i
            break
    name = name[:end].replace("vissm::", "")
    name = name.replace("false", "0").replace("true", "1").replace(", ", ",")
    return name


def parse(stderr):
    kernels, cur = [], None
    for line in stderr.splitlines():
        m = re.search(r"remark: (?:\S+: )?Function Name: (\S+)", line)
        if m:
            cur = {"name": m.group(1)}
            kernels.append(cur)
            continue
        m = re.search(r"remark: (?:\S+: )?\s*([A-Za-z][A-Za-z \[\]/]*?): (\S+) \[-Rpass-analysis", line)
        if m and cur is not None:
            cur[m.group(1).strip()] = m.group(2)
    return kernels


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("unit", help="a .hip file of viforssms_amd/csrc, e.g. flow_v5.hip")
    ap.add_argument("--filter", default="", help="only kernels whose demangled name matches this regex")
    ap.add_argument("--make-arg", action="append", default=[], help="VAR=VALUE passed to make (e.g. EXTRA=-DX=1)")
    args = ap.parse_args()
    cmd = compile_command(args.unit, args.make_arg)
    with tempfile.TemporaryDirectory() as tmp:
        i = cmd.index("-o")
        cmd[i + 1] = os.path.join(tmp, "unit.o")
        cmd += ["--cuda-device-only", "-Rpass-analysis=kernel-resource-usage"]
        r = subprocess.run(cmd, cwd=CSRC, capture_output=True, text=True)
    if r.returncode != 0:
        sys.stderr.write(r.stderr)
        raise SystemExit(f"compile failed: {' '.join(cmd)}")
    kernels = parse(r.stderr)
    for k, d in zip(kernels, demangle([k["name"] for k in kernels])):
        k["short"] = short(d)
    kernels = [k for k in kernels if re.search(args.filter, k["short"])]
    kernels.sort(key=lambda k: k["short"])
    flags = [a for a in cmd if a.startswith(("-O", "-f", "-D", "-m", "-amdgpu", "--offload-arch"))]
    print(f"# {args.unit}: {' '.join(flags)}")
    width = max([len(k["short"]) for k in kernels] + [6])
    print("  ".join(["kernel".ljust(width)] + [h for _, h in FIELDS]))
    for k in kernels:
        print("  ".join([k["short"].ljust(width)] + [str(k.get(f, "?")).rjust(len(h)) for f, h in FIELDS]))


if __name__ == "__main__":
    main()

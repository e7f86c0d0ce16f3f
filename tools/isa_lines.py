#!/usr/bin/env python3
"""tools/isa_lines.py -- static instruction counts of one kernel by source function and basic block (round 11).

    python tools/isa_lines.py --kernel k_plan_finish [--src starflate_amd/csrc/sf_kernels.hip] [--blocks]

For kernels without a round loop (k_plan_sort, k_plan_finish), where tools/isa_hist.py's phases per wave-round do not apply.
The source is compiled with `-S -gline-tables-only`; every instruction is attributed to the device function whose body
holds its source line (the innermost inlined frame the `.loc` names) and to its basic block.  The dynamic count of a
straight-line function is its static count; a loop's is its block count times the trips, which the caller supplies
(profiles/r11_notes.md writes them down).
"""
import argparse
import collections
import os
import re
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = ["-O3", "-std=c++17", "--offload-arch=gfx950", "-fPIC", "-S", "--cuda-device-only", "-gline-tables-only"]


def functions(src):
    """[(first_line, name)] of the __device__ / __global__ functions and SF_PLAN_KERNEL instantiations of the source"""
    out = []
    for i, ln in enumerate(open(src), 1):
        m = re.match(r"^(?:template\s*<[^>]*>\s*)?__(?:device|global)__.*?\b(\w+)\s*\($", ln) or re.match(r"^__(?:device|global)__[^;]*?\b(\w+)\s*\(", ln)
        if m and not ln.rstrip().endswith(";"):
            out.append((i, m.group(1)))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernel", required=True, help="regex on the mangled kernel name")
    ap.add_argument("--src", default=os.path.join(ROOT, "starflate_amd", "csrc", "sf_kernels.hip"))
    ap.add_argument("--include", default=os.path.join(ROOT, "include"))
    ap.add_argument("--blocks", action="store_true", help="one row per basic block and function")
    args = ap.parse_args()
    funcs = functions(args.src)
    base = os.path.basename(args.src)

    def func_of(line):
        cur = "?"
        for first, name in funcs:
            if first <= line:
                cur = name
            else:
                break
        return cur

    with tempfile.TemporaryDirectory() as td:
        asm = os.path.join(td, "k.s")
        subprocess.run(["/opt/rocm/bin/hipcc"] + FLAGS + ["-I", args.include, "-o", asm, args.src], check=True, stderr=subprocess.DEVNULL)
        rx, on, name = re.compile(args.kernel), False, None
        per_func = collections.defaultdict(collections.Counter)
        per_block = collections.OrderedDict()
        block, fn = "entry", "?"
        for ln in open(asm):
            if not on:
                m = re.match(r"^(_Z\w+):", ln)
                if m and rx.search(m.group(1)):
                    on, name = True, m.group(1)
                continue
            s = ln.strip()
            if s.startswith(".loc"):
                # a line of another file (a helper of sf_device.h, a HIP header) keeps the function of the instruction before it
                # (so does line 0, which the compiler gives to code of no line)
                if base in s.split("@[")[0] and int(s.split()[2]) > 0:
                    fn = func_of(int(s.split()[2]))
                continue
            m = re.match(r"^(\.LBB\d+_\d+):", ln)
            if m:
                block = m.group(1)
                continue
            if ln.startswith("\t") and re.match(r"^\t[a-z]", ln) and not s.startswith("."):
                op = s.split()[0]
                cls = ("valu" if op.startswith("v_") else "lds" if op.startswith("ds_") else "vmem" if op.startswith(("global_", "flat_", "buffer_"))
                       else "branch" if op.startswith(("s_cbranch", "s_branch")) else "salu" if op.startswith("s_") else "other")
                per_func[fn][cls] += 1
                per_block.setdefault((block, fn), collections.Counter())[cls] += 1
            elif ln.startswith(".Lfunc_end"):  # (not the first s_endpgm: a kernel has one per early return)
                break
    if name is None:
        raise SystemExit(f"no kernel matches {args.kernel!r}")
    print(f"kernel {name}")
    print(f"{'function':<28}{'VALU':>6}{'SALU':>6}{'LDS':>5}{'VMEM':>6}{'br':>5}")
    tot = collections.Counter()
    for fn, c in sorted(per_func.items(), key=lambda kv: -kv[1]["valu"]):
        print(f"{fn:<28}{c['valu']:>6}{c['salu']:>6}{c['lds']:>5}{c['vmem']:>6}{c['branch']:>5}")
        tot.update(c)
    print(f"{'total':<28}{tot['valu']:>6}{tot['salu']:>6}{tot['lds']:>5}{tot['vmem']:>6}{tot['branch']:>5}")
    if args.blocks:
        print()
        for (blk, fn), c in per_block.items():
            print(f"{blk:<12}{fn:<28}{c['valu']:>6}{c['salu']:>6}{c['lds']:>5}{c['vmem']:>6}{c['branch']:>5}")


if __name__ == "__main__":
    main()

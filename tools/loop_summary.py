#!/usr/bin/env python3
"""Per kernel of a HIP source: registers, LDS, private segment, and the instruction mix of every large inner loop -- without a GPU.

    tools/loop_summary.py eppm_amd/csrc/k_c2f_refine.hip [--filter k_c2f_refine_win] [--min-lines 150] [--flags="-DEPPM_TOL=1"]
    tools/loop_summary.py --asm dev.s            # an assembly file made earlier (hipcc FLAGS --cuda-device-only -S)

Compiles the device code to gfx950 assembly with the Makefile's FLAGS (as tools/kernel_isa.sh does).  An inner loop is the span from a
local label to a later branch back to it that holds no other such span.  Per loop of more than --min-lines lines, in the order of the
code: VALU instructions (v_*), LDS reads (ds_read*), s_waitcnt, those of them that wait for lgkmcnt(0) (a full drain of the LDS / scalar
queue: nothing of this wave is in flight behind it), and scalar loads (s_load*, s_buffer_load*).  The numbers describe one compiler's
schedule: they are recorded in profiles/, never asserted by a test.
"""
import argparse
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "eppm_amd", "csrc")


def device_asm(src, extra):
    flags = subprocess.check_output(["make", "-s", "-C", CSRC, "--eval=print-flags: ; @echo $(FLAGS)", "print-flags"], text=True).split()
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "dev.s")
        r = subprocess.run(["/opt/rocm/bin/hipcc", *flags, "--cuda-device-only", "-S", "-o", out, *extra, src], stderr=subprocess.PIPE, text=True)
        if r.returncode:
            sys.exit(r.stderr)
        return open(out).read()


def demangle(names):
    try:
        return subprocess.check_output(["c++filt", *names], text=True).split("\n")[:len(names)]
    except (OSError, subprocess.CalledProcessError):
        return names


def kernels(asm):
    """[(mangled name, body lines, {amdhsa key: value})] in the order of the file"""
    lines = asm.split("\n")
    names = [m.group(1) for m in (re.match(r"\s*\.amdhsa_kernel\s+(\S+)", l) for l in lines) if m]
    out = []
    for name in names:
        start = next(i for i, l in enumerate(lines) if l.split(";")[0].strip() == name + ":")
        end = i = next(i for i in range(start, len(lines)) if re.match(r"\s*\.amdhsa_kernel\s+" + re.escape(name) + r"\s*$", lines[i]))
        meta = {}
        while ".end_amdhsa_kernel" not in lines[i]:
            f = lines[i].split()
            if len(f) == 2 and f[0].startswith(".amdhsa_"):
                meta[f[0][8:]] = f[1]
            i += 1
        out.append((name, lines[start + 1:end], meta))
    return out


def instruction(line):
    s = line.split(";")[0].strip()
    if not s or s.startswith(".") or s.endswith(":"):
        return None
    return s


def inner_loops(body):
    """[(first line, last line)] of the spans label .. backward branch that hold no other such span"""
    label_at = {}
    spans = []
    for i, l in enumerate(body):
        m = re.match(r"(\.LBB\d+_\d+):", l)
        if m:
            label_at[m.group(1)] = i
            continue
        ins = instruction(l)
        if ins and re.match(r"s_c?branch", ins):
            t = ins.split()[-1]
            if t in label_at:
                spans.append((label_at[t], i))
    return [s for s in spans if not any(o != s and s[0] <= o[0] and o[1] <= s[1] for o in spans)]


def loop_counts(body, lo, hi):
    c = dict(lines=0, valu=0, ds_read=0, wait=0, drain=0, sload=0)
    for l in body[lo:hi + 1]:
        ins = instruction(l)
        if not ins:
            continue
        c["lines"] += 1
        op = ins.split()[0]
        if op.startswith("v_"):
            c["valu"] += 1
        elif op.startswith("ds_read") or op.startswith("ds_load"):
            c["ds_read"] += 1
        elif op == "s_waitcnt":
            c["wait"] += 1
            c["drain"] += "lgkmcnt(0)" in ins
        elif op.startswith("s_load") or op.startswith("s_buffer_load"):
            c["sload"] += 1
    return c


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("src", nargs="?", help="a HIP source of eppm_amd/csrc")
    ap.add_argument("--asm", help="read this assembly file instead of compiling")
    ap.add_argument("--filter", default="", help="only kernels whose demangled name contains this")
    ap.add_argument("--min-lines", type=int, default=150)
    ap.add_argument("--dump", type=int, default=0, help="with --filter: print the text of the filtered kernels' loop of this number")
    ap.add_argument("--flags", default="", help="extra hipcc flags, one string")
    a = ap.parse_args()
    if not a.asm and not a.src:
        ap.error("a source or --asm")
    extra = a.flags.split()
    asm = open(a.asm).read() if a.asm else device_asm(a.src, extra)
    ks = kernels(asm)
    names = demangle([k[0] for k in ks])
    for (_, body, meta), name in sorted(zip(ks, names), key=lambda t: t[1]):
        name = re.sub(r"\(.*\)$", "", name.replace("eppm::", "").replace("void ", ""))
        if a.filter not in name:
            continue
        print(f"{name}: vgpr {meta.get('next_free_vgpr')} (arch {meta.get('accum_offset')}) sgpr {meta.get('next_free_sgpr')} "
              f"lds {meta.get('group_segment_fixed_size')} private {meta.get('private_segment_fixed_size')}")
        n = 0
        for lo, hi in inner_loops(body):
            c = loop_counts(body, lo, hi)
            if c["lines"] <= a.min_lines:
                continue
            n += 1
            print(f"    loop {n}: lines {c['lines']:4d}  valu {c['valu']:4d}  ds_read {c['ds_read']:3d}  s_waitcnt {c['wait']:3d}  "
                  f"lgkmcnt(0) {c['drain']:3d}  s_load {c['sload']:3d}")
            if n == a.dump:
                print("\n".join(body[lo:hi + 1]))
    return 0


if __name__ == "__main__":
    sys.exit(main())

#!/usr/bin/env python3
"""Compile the translation units of libmcx with -save-temps and summarise one kernel: registers and the instruction
mix of its biggest loop.  usage: tools/kernel_asm.py <mangled-name-substring> [--dump]
       tools/kernel_asm.py --compare DIR_A DIR_B [UNIT ...]: two sets of <unit>.s files (the step kernels' units, or UNIT ...) (hipcc <Makefile's flags> --cuda-device-only -S),
       kernel by kernel: how many instruction streams are the same, and size / registers / LDS / scratch / occupancy of the rest

The biggest loop is the biggest INNERMOST one (a backward branch whose span holds no other): the hot kernels' step
loops sit inside an outer loop of passes (k_fused_fast's snapshot split), and the outer one would count the prologue and
the epilogue steps too.  tests/test_hot_loop_codegen_cpu.py uses the functions below."""
import collections
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TMP = "/tmp/mcx_asm"
# the Makefile's HIPFLAGS
FLAGS = ["-O3", "-std=c++17", "--offload-arch=gfx950", "-fPIC", "-ffp-contract=off", "-fno-fast-math",
         "-fno-gpu-flush-denormals-to-zero", "-I" + ROOT + "/include"]
VCOPY = re.compile(r"v_mov_b(32|64)(_e32|_e64)?\s+v(\[\d+:\d+\]|\d+),\s*v(\[\d+:\d+\]|\d+)\s*$")


def compile_tu(tu, tmp=TMP, hipcc="hipcc", device_only=False):
    """device assembly (gfx950) of mcpar_amd/csrc/<tu>.hip (device_only: without compiling the host side)"""
    os.makedirs(tmp, exist_ok=True)
    src = ROOT + "/mcpar_amd/csrc/%s.hip" % tu
    if device_only:
        out = os.path.join(tmp, tu + ".s")
        subprocess.check_call([hipcc] + FLAGS + ["--cuda-device-only", "-S", "-o", out, src], cwd=tmp, stderr=subprocess.DEVNULL)
        return open(out).read()
    subprocess.check_call([hipcc] + FLAGS + ["-c", "-save-temps", "-o", "x.o", src], cwd=tmp, stderr=subprocess.DEVNULL)
    return open(tmp + "/%s-hip-amdgcn-amd-amdhsa-gfx950.s" % tu).read()


def kernel_body(s, name):
    i = s.index("\n" + name + ":")
    j = s.index(".Lfunc_end", i)
    return s[i:j].split("\n")


def kernel_meta(s, name):
    meta = s[s.index(".name:           " + name):]
    return {k: re.search(k + r":\s+(\d+)", meta).group(1) for k in (".vgpr_count", ".sgpr_count", ".group_segment_fixed_size", ".private_segment_fixed_size")}


def biggest_loop(body):
    """(first, last) line of the biggest innermost loop, or None"""
    labels = {}
    for k, l in enumerate(body):
        m = re.match(r"^(\.LBB\d+_\d+):", l)
        if m:
            labels[m.group(1)] = k
    loops = []
    for k, l in enumerate(body):
        m = re.search(r"s_c?branch\w* (\.LBB\d+_\d+)", l)
        if m and m.group(1) in labels and labels[m.group(1)] < k:
            loops.append((labels[m.group(1)], k))
    inner = [a for a in loops if not any(b != a and a[0] <= b[0] and b[1] <= a[1] for b in loops)]
    return max(inner, key=lambda a: a[1] - a[0]) if inner else None


def loop_ops(body, loop):
    """instruction counts of the loop, and the number of VGPR-to-VGPR copies"""
    ops = collections.Counter()
    vcopies = 0
    for l in body[loop[0]:loop[1] + 1]:
        l = l.strip()
        if not l or l.startswith((".", ";")) or l.endswith(":"):
            continue
        ops[l.split()[0]] += 1
        vcopies += 1 if VCOPY.match(l) else 0
    return ops, vcopies


STEP_UNITS = ("mcx_k_fast", "mcx_k_fast_full", "mcx_k_fastb", "mcx_k_fastb_full", "mcx_k_pregen", "mcx_k_generic_burn",
              "mcx_k_generic_main", "mcx_k_persist")


KEYS = ("NumVgprs", "TotalNumSgprs", "LDSByteSize", "ScratchSize", "Occupancy")


def instruction_stream(body):
    """the instructions alone: no comments, directives or blank lines, every .LBB label one token"""
    out = []
    for l in body[1:]:
        l = re.sub(r"\.LBB\d+_\d+", ".LBB", l.split(";")[0].strip())
        if l and (not l.startswith(".") or l.startswith(".LBB")):
            out.append(l)
    return out


def compare(dir_a, dir_b, units=STEP_UNITS):
    """one markdown table per translation unit; returns the number of kernels with new scratch or lower occupancy"""
    bad = 0
    for tu in units:
        a, b = (open(os.path.join(d, tu + ".s")).read() for d in (dir_a, dir_b))
        names = re.findall(r"\.amdhsa_kernel (\w+)", a)
        assert names == re.findall(r"\.amdhsa_kernel (\w+)", b), tu + ": the two sets hold different kernels"
        rows = []
        for n in names:
            sa, sb = instruction_stream(kernel_body(a, n)), instruction_stream(kernel_body(b, n))
            if sa == sb:
                continue
            # (the resource comments that follow the kernel's code)
            ma, mb = ({k: re.search("; %s: (\\d+)" % k, t[t.index("\n" + n + ":"):]).group(1) for k in KEYS} for t in (a, b))
            flag = (ma["ScratchSize"] == "0" and mb["ScratchSize"] != "0") or int(mb["Occupancy"]) < int(ma["Occupancy"])
            bad += flag
            demangled = subprocess.run(["c++filt", n], capture_output=True, text=True).stdout.strip() or n
            rows.append("| `%s` | %d → %d | %s |%s" % (re.sub(r"^void mcx::|\(.*$", "", demangled), len(sa), len(sb),
                                                     " | ".join("%s → %s" % (ma[k], mb[k]) for k in KEYS), " **worse**" if flag else ""))
        print("\n`%s`: %d of %d kernels instruction-identical\n" % (tu, len(names) - len(rows), len(names)))
        if rows:
            print("| kernel | instructions | VGPRs | SGPRs | LDS bytes | scratch bytes | occupancy |\n|---|---|---|---|---|---|---|")
            print("\n".join(rows))
    return bad


def main():
    if sys.argv[1] == "--compare":
        return 1 if compare(sys.argv[2], sys.argv[3], tuple(sys.argv[4:]) or STEP_UNITS) else 0
    pat = sys.argv[1]
    s = ""
    for tu in ("mcx_k_fast", "mcx_k_fast_full", "mcx_k_fastb", "mcx_k_fastb_full", "mcx_k_pregen", "mcx_k_generic_main", "mcx_k_generic_burn", "mcx_engine"):
        if pat.startswith("k_fused_fast") and tu not in ("mcx_k_fast", "mcx_k_fast_full", "mcx_k_fastb", "mcx_k_fastb_full", "mcx_k_pregen"):
            continue
        s += compile_tu(tu)
    names = sorted(set(re.findall(r"^(_Z\w+):", s, flags=re.M)))
    hits = [n for n in names if pat in n]
    for name in hits:
        body = kernel_body(s, name)
        print(name, kernel_meta(s, name))
        best = biggest_loop(body)
        if best:
            ops, vcopies = loop_ops(body, best)
            tot = sum(ops.values())
            valu = sum(v for k, v in ops.items() if k.startswith("v_"))
            salu = sum(v for k, v in ops.items() if k.startswith("s_") and k != "s_nop")
            print("  biggest loop: %d instrs, %d VALU, %d VGPR copies, %d exec-mask regions, %d SALU (+ %d s_nop), %d branches"
                  % (tot, valu, vcopies, ops["s_and_saveexec_b64"], salu, ops["s_nop"], sum(v for k, v in ops.items() if "branch" in k)))
            print("  " + ", ".join("%s %d" % kv for kv in ops.most_common(40)))
            if "--dump" in sys.argv:
                print("\n".join(body[best[0]:best[1] + 1]))


if __name__ == "__main__":
    sys.exit(main())

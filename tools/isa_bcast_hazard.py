#!/usr/bin/env python3
"""Static hazard check of the pair kernel's fused broadcasts (uwvk_psp_dev.hpp
fmac_bc / fnmac_bc: v_fmac_f64_dpp written as inline assembly, where the
compiler's hazard recogniser does not look).

For every v_fmac_f64_dpp of every kernel body in the pair unit's gfx950
assembly, walking back over the straight-line text before it:
  * no VALU instruction within 2 wait states writes a register of the DPP
    source pair (src0).  The accumulator and the second factor are ordinary
    VALU operands, which the hardware interlocks (tools/probe_dpp64.hip runs
    two fused FMAs back to back behind the writes of both and compares the
    values); how many FMAs follow such a write that closely is only counted;
  * no v_cmpx (a VALU write of EXEC) within 5 wait states.
A VALU instruction is one wait state, s_nop N is N + 1; a label or a branch
ends the walk as a failure if the states are not yet covered (nothing is known
about the other path).  Prints the per-kernel counts; exit status 1 on a
violation.

usage: tools/isa_bcast_hazard.py [file.s]     (default: compile uwvk_psp_pair.hip)"""
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "slam-uwv_kalman_filters_amd")
REG = re.compile(r"v\[(\d+):(\d+)\]|v(\d+)")


def regs(tok):
    m = REG.search(tok)
    if not m:
        return set()
    if m.group(3) is not None:
        return {int(m.group(3))}
    return set(range(int(m.group(1)), int(m.group(2)) + 1))


def psp_flags():
    for ln in open(os.path.join(PKG, "Makefile")):
        if ln.startswith("PSP_FLAGS :="):
            return ln.split(":=", 1)[1].split()
    raise SystemExit("PSP_FLAGS not found in the Makefile")


def compile_pair(extra):
    d = tempfile.mkdtemp(prefix="isa_bcast_")
    out = os.path.join(d, "pair.s")
    subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "-O3", "-std=c++17", "--offload-arch=gfx950",
                    "--cuda-device-only", "-S", *psp_flags(), *extra,
                    os.path.join(PKG, "csrc", "uwvk_psp_pair.hip"), "-o", out], check=True)
    return out


def writes(ops):
    """VGPRs written by a VALU instruction: its first operand, and for
    v_permlane16_swap / v_swap also the second."""
    op = ops[0]
    args = [a.strip() for a in " ".join(ops[1:]).split(",")]
    w = regs(args[0]) if args else set()
    if op.startswith(("v_permlane16_swap", "v_permlane32_swap", "v_swap")) and len(args) > 1:
        w |= regs(args[1])
    if op.startswith(("v_cmp", "v_readlane", "v_readfirstlane")):
        w = set()
    return w


def check(path):
    bad = 0
    kernel, body = None, []
    stats = {}
    for raw in open(path):
        ln = raw.split(";")[0].rstrip()
        if not ln.strip():
            continue
        m = re.match(r"^(_Z\w*k_psp_epoch_pair\w*):", ln)
        if m:
            kernel, body = m.group(1), []
            stats[kernel] = [0, 0, 0]
            continue
        if kernel is None:
            continue
        t = ln.strip()
        if t.startswith("s_endpgm"):
            kernel = None
            continue
        if t.startswith("."):
            continue
        body.append(t)
        ops = t.split()
        if ops[0].startswith("v_permlane16_swap"):
            stats[kernel][1] += 1
        if not ops[0].startswith("v_fmac_f64_dpp"):
            continue
        stats[kernel][0] += 1
        args = [a.strip().split()[0].lstrip("-") for a in " ".join(ops[1:]).split(",")[:3]]
        src = regs(args[1])                    # the DPP source
        other = regs(args[0]) | regs(args[2])  # the accumulator and the second factor
        ws = 0
        for prev in reversed(body[:-1]):
            if ws >= 5:
                break
            p = prev.split()
            if prev.endswith(":") or p[0].startswith(("s_cbranch", "s_branch", "s_setpc", "s_swappc")):
                if ws < 2:
                    print("%s: `%s` %d wait states after `%s`: unknown path" % (kernel, t, ws, prev))
                    bad += 1
                break
            if p[0] == "s_nop":
                ws += int(p[1], 0) + 1
                continue
            if not p[0].startswith("v_"):
                if not p[0].startswith(("s_waitcnt", "s_setprio", "s_barrier")):
                    ws += 1  # any other instruction issues in at least one cycle
                continue
            if p[0].startswith("v_cmpx"):
                print("%s: `%s` %d wait states after `%s`" % (kernel, t, ws, prev))
                bad += 1
            if ws < 2 and (writes(p) & src):
                print("%s: `%s` %d wait states after `%s`" % (kernel, t, ws, prev))
                bad += 1
            if ws < 2 and (writes(p) & other):
                stats[kernel][2] += 1
            ws += 1
    for k, (n, s, o) in stats.items():
        print("%s: %d v_fmac_f64_dpp, %d v_permlane16_swap_b32; %d follow a write of their accumulator or second "
              "factor within 2 wait states" % (k, n, s, o))
    if not stats:
        print("no pair kernel body found")
        return 1
    return 1 if bad else 0


if __name__ == "__main__":
    a = sys.argv[1:]
    src = a[0] if a and a[0].endswith(".s") else compile_pair(a)
    sys.exit(check(src))

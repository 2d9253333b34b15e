#!/usr/bin/env python3
"""Static VALU mix per phase of k_psp_epoch<DOF> (diagnostic): compiles the PSP
translation unit with -DUWVK_STAMPS to gfx950 assembly and splits the kernel at
the s_memtime of every UWVK_STAMP (sched_barrier keeps phases apart).  Loops are
counted once (the rank-M blocks, the manifold-mean iterations).

usage: tools/isa_phases.py [DOF] [extra hipcc flags...]
       tools/isa_phases.py pair [extra hipcc flags...]

pair: k_psp_epoch_pair<1, 1, 1> (uwvk_psp_pair.hip).  The pair kernel carries no
Stamper, so the unit is compiled with -DUWVK_PHASE_MARKS (an assembler comment
per stamp site, no instruction) and the epoch loop's text is split at the
marks.  A segment is named after the mark that ends it, as a stamp charges the
time since the previous one: 20..26 the predict, a30..a35 the acceleration
update, d30..d35 the DVL update (one epoch in 200), `loop` the rest of the loop
(the epoch's fetch, the branches around the updates, the fold's call)."""
import collections
import os
import re
import subprocess
import sys

# UWVK_SR=0: the left-side instantiation (uwvk_psp_k.hip); default the right side
SR = os.environ.get("UWVK_SR", "1")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "slam-uwv_kalman_filters_amd")
dof = sys.argv[1] if len(sys.argv) > 1 else "53"
extra = sys.argv[2:]
out = "/tmp/psp_phases.s"
INT = re.compile(r"v_(add|sub|subrev|mul_lo|mul_hi|mad|lshl|lshr|ashr|and|or|xor|bfe|bfi|max|min|cvt|mul_u32|"
                 r"lshlrev|lshrrev|ashrrev|not|perm|alignbit|add3|lshl_add|lshl_or|and_or|or3|xad)_")
KEYS = ["valu", "f64", "int", "mov", "cnd", "lane", "dpp", "cmp", "other", "lds", "salu"]


def count(cur, t):
    op = t.split()[0]
    if op.startswith("v_"):
        cur["valu"] += 1
        if "f64" in op and not op.startswith("v_cmp"):
            cur["f64"] += 1
        elif op.startswith(("v_readlane", "v_writelane", "v_readfirstlane")):
            cur["lane"] += 1
        elif "dpp" in op or "dpp" in t:
            cur["dpp"] += 1
        elif op.startswith("v_cndmask"):
            cur["cnd"] += 1
        elif op.startswith("v_mov"):
            cur["mov"] += 1
        elif op.startswith("v_cmp"):
            cur["cmp"] += 1
        elif INT.match(op):
            cur["int"] += 1
        else:
            cur["other"] += 1
    elif op.startswith("ds_"):
        cur["lds"] += 1
        cur[op] += 1
    elif op.startswith("s_"):
        cur["salu"] += 1


def pair_table():
    subprocess.run(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "--cuda-device-only",
                    "-mllvm", "-disable-machine-licm", "-mllvm", "-amdgpu-mfma-vgpr-form", "-DUWVK_PHASE_MARKS", *extra,
                    "-S", "-o", out, os.path.join(PKG, "csrc", "uwvk_psp_pair.hip")], check=True, stderr=subprocess.DEVNULL)
    s = open(out).read().split("\n")
    name = "_ZN4uwvk4psp216k_psp_epoch_pairILi1ELi1ELi1EEEvNS_8PoseBufsENS_10PoseSharedENS_9EpochArgsE"
    st = [i for i, l in enumerate(s) if l.startswith(name + ":")][0]
    en = [i for i, l in enumerate(s) if i > st and l.startswith(".Lfunc_end")][0]
    body = s[st:en]
    # the epoch loop: the depth-2 loop with the longest span of text
    best = None
    for i, l in enumerate(body):
        if "Loop Header: Depth=2" in l:
            lab = next(re.match(r"^(\.LBB\d+_\d+):", body[j]).group(1) for j in range(i, -1, -1)
                       if re.match(r"^\.LBB\d+_\d+:", body[j]))
            bs = [j for j, x in enumerate(body) if x.strip().startswith(("s_branch", "s_cbranch")) and x.strip().endswith(" " + lab)]
            if bs and (best is None or max(bs) - i > best[1] - best[0]):
                best = (i, max(bs))
    segs, cur, seen30 = [], collections.Counter(), 0
    for l in body[best[0]:best[1] + 1]:
        t = l.strip()
        m = re.match(r"^; uwvk_phase (\d+)$", t)
        if m:
            ph = int(m.group(1))
            seen30 += ph == 30
            segs.append((("%d" % ph) if ph < 30 else ("ad"[min(seen30, 2) - 1] + "%d" % ph), cur))
            cur = collections.Counter()
            continue
        if not t or t.startswith((".", ";")) or t.endswith(":"):
            continue
        count(cur, t)
    segs.append(("loop", cur))
    ds = sorted({k for _, c in segs for k in c if k.startswith("ds_")})
    print("%-5s " % "seg" + " ".join("%6s" % k for k in KEYS) + "  " + " ".join(ds))
    tot = collections.Counter()
    for nm, c in segs:
        print("%-5s " % nm + " ".join("%6d" % c[k] for k in KEYS) + "  " + " ".join("%*d" % (len(k), c[k]) for k in ds))
        if not nm.startswith("d"):
            tot.update(c)
    print("%-5s " % "epoch" + " ".join("%6d" % tot[k] for k in KEYS) + "  " + " ".join("%*d" % (len(k), tot[k]) for k in ds)
          + "   (without the DVL update: a plain acceleration epoch, per wave = two instances)")


if dof == "pair":
    pair_table()
    sys.exit(0)
subprocess.run(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "--cuda-device-only",
                "-mllvm", "-disable-machine-licm", "-mllvm", "-amdgpu-mfma-vgpr-form", "-DUWVK_STAMPS", *extra, "-S", "-o", out,
                os.path.join(PKG, "csrc", "uwvk_psp_k_r.hip" if SR == "1" else "uwvk_psp_k.hip")], check=True, stderr=subprocess.DEVNULL)
s = open(out).read().split("\n")
name = "_ZN4uwvk3psp11k_psp_epochILi%sELi1ELi1ELi%sEEEvNS_8PoseBufsENS_10PoseSharedENS_9EpochArgsE" % (dof, SR)
st = [i for i, l in enumerate(s) if l.startswith(name + ":")][0]
en = [i for i, l in enumerate(s) if i > st and l.startswith(".Lfunc_end")][0]
INT = re.compile(r"v_(add|sub|subrev|mul_lo|mul_hi|mad|lshl|lshr|ashr|and|or|xor|bfe|bfi|max|min|cvt|mul_u32|"
                 r"lshlrev|lshrrev|ashrrev|not|perm|alignbit|add3|lshl_add|lshl_or|and_or|or3|xad)_")
segs, cur = [], collections.Counter()
for l in s[st:en + 1]:
    t = l.strip()
    if not t or t.startswith((".", ";")) or t.endswith(":"):
        continue
    op = t.split()[0]
    if op == "s_memtime":
        segs.append(cur)
        cur = collections.Counter()
        continue
    if op.startswith("v_"):
        cur["valu"] += 1
        if "f64" in op and not op.startswith("v_cmp"):
            cur["f64"] += 1
        elif op.startswith(("v_readlane", "v_writelane", "v_readfirstlane")):
            cur["lane"] += 1
        elif "dpp" in op or "dpp" in t:
            cur["dpp"] += 1
        elif op.startswith("v_cndmask"):
            cur["cnd"] += 1
        elif op.startswith("v_mov"):
            cur["mov"] += 1
        elif op.startswith("v_cmp"):
            cur["cmp"] += 1
        elif INT.match(op):
            cur["int"] += 1
        else:
            cur["other"] += 1
    elif op.startswith("ds_"):
        cur["lds"] += 1
    elif op.startswith("s_"):
        cur["salu"] += 1
segs.append(cur)
keys = ["valu", "f64", "int", "mov", "cnd", "lane", "dpp", "cmp", "other", "lds", "salu"]
print("%-4s " % "seg" + " ".join("%6s" % k for k in keys))
for i, c in enumerate(segs):
    print("%-4d " % i + " ".join("%6d" % c[k] for k in keys))

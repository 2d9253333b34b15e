"""Static checks on the ISA of the pair epoch kernel (CPU: hipcc cross-compile
only; the same compile, flags and cache as tests/test_kernel_resources.py).

k_psp_epoch_pair is bound by VALU issue, so instructions
the result does not need are kept out of its epoch loop:

* the per-half broadcast hbc (uwvk_psp_dev.hpp) moves a lane's value to every
  lane of its 16-lane row with row_newbcast under full row and bank masks.
  Every lane has a source, so the destination's old value is never read; an
  explicit zero `old` operand made the compiler emit `v_mov_b32 v, 0` before
  each such move (133 of the loop's 5,115 VALU instructions);
* the 26-in-53 index map pd_pidx (an IEEE sqrtf and integer fix-ups per slot)
  is tabulated once per wave, before the work-unit loop: no v_sqrt_f32 inside
  the epoch loop or anywhere in the per-unit path."""
import re

import pytest

from test_kernel_resources import HAVE_HIPCC, compile_asm, tu_flags

SRC = "csrc/uwvk_psp_pair.hip"
PREFIX = "_ZN4uwvk4psp216k_psp_epoch_pairILi"
NEWBCAST_FULL = re.compile(r"^v_mov_b32_dpp (v\d+), .*row_newbcast:\d+ row_mask:0xf bank_mask:0xf")
LOOKBACK = 6  # instructions before the DPP move in which a zeroing of its destination counts


def kernel_bodies(asm):
    """{mangled name: stripped non-empty lines} of every pair-kernel instantiation."""
    lines = asm.split("\n")
    out = {}
    for i, l in enumerate(lines):
        m = re.match(r"^(%s\w*):" % PREFIX, l)
        if m:
            en = next(j for j in range(i, len(lines)) if lines[j].startswith(".Lfunc_end"))
            out[m.group(1)] = [x.strip() for x in lines[i:en] if x.strip()]
    return out


def instructions(body):
    return [x for x in body if not x.startswith((";", ".")) and not x.split()[0].endswith(":")]


BLOCK = re.compile(r"^(?:\.L(BB\d+_\d+)|; %bb\.\d+):")


def blocks(body):
    """The kernel's basic blocks in layout order: (name or None, loop chain,
    instructions).  The loop chain is read from the compiler's block comments
    ("in Loop: Header=BB7_5 Depth=1"; on a header "This Loop Header: Depth=2"
    and its "Parent Loop" lines): the headers of the loops the block is in,
    innermost first.  Block placement does not matter (a loop's blocks need not
    be contiguous, nor end at its last back edge)."""
    raw, cur = [], None
    for x in body:
        m = BLOCK.match(x)
        if m:
            cur = {"name": m.group(1), "ann": [x], "ins": [], "open": True}
            raw.append(cur)
        elif cur is None:
            continue
        elif x.startswith(";") and cur["open"]:
            cur["ann"].append(x)
        elif not x.startswith((";", ".")) and not x.split()[0].endswith(":"):
            cur["open"] = False
            cur["ins"].append(x)
    parents = {}  # header -> enclosing headers, innermost first
    for b in raw:
        ann = " ".join(b["ann"])
        if "Loop Header: Depth=" in ann:
            ps = re.findall(r"Parent Loop (BB\d+_\d+) Depth=(\d+)", ann)
            parents[b["name"]] = [h for h, _ in sorted(ps, key=lambda hd: -int(hd[1]))]
    out = []
    for b in raw:
        ann = " ".join(b["ann"])
        m = re.search(r"in Loop: Header=(BB\d+_\d+) Depth=\d+", ann)
        if b["name"] in parents:
            chain = [b["name"]] + parents[b["name"]]
        elif m:
            chain = [m.group(1)] + parents[m.group(1)]
        else:
            chain = []
        out.append((b["name"], chain, b["ins"]))
    return out


def loop_instructions(blks, header):
    return [x for _, chain, ins in blks if header in chain for x in ins]


def unit_and_epoch_loop(blks):
    """(work-unit loop, epoch loop) instruction lists: the kernel's one depth-1
    loop, and the largest loop directly inside it."""
    outer = {chain[-1] for _, chain, _ in blks if chain}
    assert len(outer) == 1, outer
    inner = {chain[-2] for _, chain, _ in blks if len(chain) >= 2}
    epoch = max(inner, key=lambda h: len(loop_instructions(blks, h)))
    return loop_instructions(blks, outer.pop()), loop_instructions(blks, epoch)


def zeroed_newbcasts(ins):
    """Full-mask row_newbcast moves whose destination a `v_mov_b32 v, 0` wrote
    within the LOOKBACK instructions before (nothing else writing it between)."""
    bad = []
    for i, x in enumerate(ins):
        m = NEWBCAST_FULL.match(x)
        if not m:
            continue
        for y in reversed(ins[max(0, i - LOOKBACK):i]):
            if re.match(r"^v_mov_b32_e32 %s, 0$" % m.group(1), y):
                bad.append((y, x))
                break
            if re.match(r"^v_\S+ %s," % m.group(1), y):
                break
    return bad


def test_zeroed_newbcast_scan_catches_the_pattern():
    dead = ["v_mov_b32_e32 v7, 0", "v_add_f64 v[2:3], v[2:3], v[4:5]",
            "v_mov_b32_dpp v7, v12 row_newbcast:3 row_mask:0xf bank_mask:0xf"]
    assert len(zeroed_newbcasts(dead)) == 1
    assert not zeroed_newbcasts(dead[1:])
    assert not zeroed_newbcasts(["v_mov_b32_e32 v7, 0", "v_mov_b32_dpp v7, v12 row_bcast:15 row_mask:0xa bank_mask:0xf"])
    assert not zeroed_newbcasts(["v_mov_b32_e32 v7, 0", "v_mov_b32_e32 v7, v9",
                                 "v_mov_b32_dpp v7, v12 row_newbcast:3 row_mask:0xf bank_mask:0xf"])


@pytest.fixture(scope="module")
def bodies():
    if not HAVE_HIPCC:
        pytest.skip("no hipcc")
    b = kernel_bodies(compile_asm(SRC, tu_flags(SRC))[0])
    assert len(b) == 8, sorted(b)  # SR x EVS x PD
    return b


def test_no_dead_zero_in_front_of_a_row_newbcast(bodies):
    for name, body in bodies.items():
        ins = instructions(body)
        assert any(NEWBCAST_FULL.match(x) for x in ins), name  # hbc is still this DPP form
        bad = zeroed_newbcasts(ins)
        assert not bad, (name, len(bad), bad[:3])


def test_no_sqrt_in_the_epoch_loop(bodies):
    for name, body in bodies.items():
        unit, epoch = unit_and_epoch_loop(blocks(body))
        assert 5000 < len(epoch) < len(unit), (name, len(epoch), len(unit))  # the epoch loop, not a helper loop
        assert not [x for x in epoch if x.startswith("v_sqrt_f32")], name


def test_index_map_is_not_recomputed_per_unit(bodies):
    """pd_pidx's sqrtf: 11 slots per lane, once, before the work-unit loop
    (PD = 1); none at all in the 26-DOF handles' kernels (PD = 0)."""
    for name, body in bodies.items():
        pd = int(re.search(r"pairILi\dELi\dELi(\d)E", name).group(1))
        blks = blocks(body)
        unit, _ = unit_and_epoch_loop(blks)
        assert not [x for x in unit if x.startswith("v_sqrt_f32")], name
        outside = [x for _, chain, ins in blks if not chain for x in ins]
        assert len(outside) + len(unit) == len(instructions(body)), name  # every instruction is in a block
        assert sum(x.startswith("v_sqrt_f32") for x in outside) == (11 if pd else 0), name

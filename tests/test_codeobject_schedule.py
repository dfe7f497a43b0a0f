"""K-loop schedule of the aligned GEMM kernels in the SHIPPED gfx950 code object (CPU).

The GEMM main loop is a register-prefetch pipeline: the global loads of K-tile
t+1 are meant to issue before the MFMA phase of tile t and to be waited for
only after it, in front of the LDS writes.  Nothing in the source forces that:
the compiler is free to sink an unguarded load of a `const __restrict__`
kernel argument down to its first use, which puts a full global-load latency
in front of the workgroup barrier of every K-step (the aligned k_grad_w_t
variants were compiled like that).  This test reads the order back from the
disassembly of every aligned variant the launchers can take.

How the loop is read.  The compiler lays most of these loops out rotated: the
loop header is the first LDS read of the MFMA phase and the loads of the next
tile are the last instructions before the back edge, so "every load precedes
the first MFMA, walking from the header" is false for schedules that are
right and cannot be asserted literally.  The body is a cycle, and it is read
as one, starting at the first tile load after the barrier.  In that reading
  * `loads_after == 0` only says that the tile loads form one group that no
    MFMA splits; it holds for a lost prefetch as well (loads, wait, writes,
    barrier, then all the MFMAs) and discriminates nothing by itself;
  * `mfma_covered >= TBK-2`, the MFMAs between the last tile load and the
    first `s_waitcnt vmcnt` behind it, is the assertion that tells a kept
    prefetch from a lost one: it is the work a load's latency hides behind.
"""

import re

import pytest

from tests.test_codeobject import disasm  # noqa: F401  (module-scoped fixture)

# (kernel, TBK, TBN) of every ALIGNED instantiation sae_ops.hip can launch
VARIANTS = [(stem, tbk, tbn)
            for stem in ("k_enc_fwd_t", "k_dec_fwd_t", "k_gc_t", "k_gc_thresh_t", "k_grad_w_t")
            for tbk, tbn in ((16, 128), (32, 128), (16, 256))
            if not (stem == "k_gc_thresh_t" and tbn == 256)]

_INSN = re.compile(r"^\s+(\S+)\s*(.*?)\s*//\s*([0-9A-Fa-f]+):\s*[0-9A-Fa-f ]+?(?:<[^+>]+\+0x([0-9a-f]+)>)?\s*$")


def find_variant(sections, stem, tbk, tbn, aligned=True):
    """(name, body) of the one <tbk, *, tbn, aligned> instantiation of `stem`."""
    pat = re.compile(rf"^_Z{len(stem)}{stem}ILi{tbk}ELi\d+ELi{tbn}ELb{int(aligned)}EE")
    hits = [(n, b) for n, b in sections.items() if pat.match(n)]
    assert len(hits) == 1, f"{stem}<{tbk}, *, {tbn}, {aligned}>: found {[n for n, _ in hits]}"
    return hits[0]


def instructions(body):
    """[(address, mnemonic, operands, branch target offset in the kernel or None)]"""
    out = []
    for line in body.splitlines():
        m = _INSN.match(line)
        if m:
            out.append((int(m.group(3), 16), m.group(1), m.group(2),
                        int(m.group(4), 16) if m.group(4) else None))
    return out


def kloop(body, tbk):
    """The K-loop's instructions in program order from the loop header: the
    shortest backward-branch span that holds >= tbk MFMAs and an s_barrier."""
    ins = instructions(body)
    assert ins, "no instructions parsed from the disassembly"
    base = ins[0][0]
    index = {addr: i for i, (addr, _, _, _) in enumerate(ins)}
    best = None
    for i, (addr, op, _, target) in enumerate(ins):
        if not op.startswith(("s_cbranch", "s_branch")) or target is None:
            continue
        j = index.get(base + target)
        if j is None or j > i:
            continue
        span = ins[j:i + 1]
        ops = [o for _, o, _, _ in span]
        if sum(o.startswith("v_mfma") for o in ops) >= tbk and "s_barrier" in ops:
            if best is None or len(span) < len(best):
                best = span
    assert best is not None, "no loop with >= TBK MFMAs and a barrier"
    return best


def is_tile_load(op):
    return op == "global_load_dwordx4"


def schedule(loop):
    """Where a loop body's tile loads sit relative to its MFMAs.
    loads_before / loads_after: tile loads ahead of / behind the first MFMA;
    mfma_covered: MFMAs between the last tile load and the first vmcnt wait
    that follows it (the MFMAs a load's latency is hidden behind)."""
    ops = [(op, args) for _, op, args, _ in loop]
    # The compiler lays the loop out rotated (in most variants the loads of the
    # next tile are the last instructions before the back edge), so the body is
    # read as the cycle it is, starting at the first tile load after the barrier.
    barrier = max(i for i, (op, _) in enumerate(ops) if op == "s_barrier")
    ops = ops[barrier + 1:] + ops[:barrier + 1]
    start = next((i for i, (op, _) in enumerate(ops) if is_tile_load(op)), None)
    assert start is not None, "no tile loads in the K-loop"
    ops = ops[start:] + ops[:start]
    first_mfma = next(i for i, (op, _) in enumerate(ops) if op.startswith("v_mfma"))
    loads = [i for i, (op, _) in enumerate(ops) if is_tile_load(op)]
    assert loads, "no tile loads in the K-loop"
    waits = [i for i, (op, args) in enumerate(ops)
             if op == "s_waitcnt" and "vmcnt" in args and i > loads[-1]]
    end = waits[0] if waits else len(ops)
    return {
        "loads_before": sum(i < first_mfma for i in loads),
        "loads_after": sum(i > first_mfma for i in loads),
        "mfma_covered": sum(op.startswith("v_mfma") for op, _ in ops[loads[-1]:end]),
        "mfma": sum(op.startswith("v_mfma") for op, _ in ops),
        "waits_after_loads": len(waits),
    }


@pytest.mark.parametrize("stem,tbk,tbn", VARIANTS)
def test_next_tile_loads_issue_before_the_mfma_phase(disasm, stem, tbk, tbn):  # noqa: F811
    name, body = find_variant(disasm, stem, tbk, tbn)
    s = schedule(kloop(body, tbk))
    print(f"{name}: {s}")
    assert s["loads_after"] == 0, (
        f"{name}: {s['loads_after']} of {s['loads_before'] + s['loads_after']} tile loads issue "
        f"after the first MFMA of the K-loop (prefetch compiled away)")
    # the loads are consumed inside the loop (by the LDS writes), so there is a wait
    assert s["waits_after_loads"] >= 1, f"{name}: no vmcnt wait after the tile loads"
    assert s["mfma_covered"] >= tbk - 2, (
        f"{name}: only {s['mfma_covered']} MFMAs between the last tile load and its vmcnt wait, "
        f"want >= {tbk - 2}")

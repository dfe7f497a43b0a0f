"""The shapes of the sparse and Matryoshka kernel tests against the register
depths the launchers compile.

k_sparse_dec_gc and k_sparse_grad_w, plain and with levels, are templates over
DL; SPARSE_DISPATCH_DL (sae_ops.hip) lists the compiled depths and takes the
smallest one >= ceil(d / 64).  The GPU tests are written against that list:
every depth has to run full or nearly so, and every depth above 2 also at a d
whose ceil(d / 64) lies below it, where whole registers are past d.  A depth
added to the macro without shapes for it fails here, without a GPU.
"""

import os
import re

from tests import test_matryoshka_gpu as mat
from tests import test_topk_sparse_chain_gpu as plain

OPS = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                   "sparse_coding_amd", "ops", "hip", "sae_ops.hip")


def compiled_depths():
    """The integers of the LAUNCH(...) calls in the SPARSE_DISPATCH_DL macro."""
    with open(OPS) as f:
        text = f.read()
    body = re.search(r"#define SPARSE_DISPATCH_DL\(d, LAUNCH\)((?:.*\\\n)*.*\n)", text)
    assert body, "SPARSE_DISPATCH_DL not found"
    return tuple(int(v) for v in re.findall(r"\bLAUNCH\((\d+)\)", body.group(1)))


def depth_of(d, depths):
    """The macro's rule: the smallest compiled depth >= ceil(d / 64)."""
    need = (d + 63) // 64
    return min(D for D in depths if D >= need)


def test_the_tests_know_the_compiled_depths():
    depths = compiled_depths()
    assert depths == tuple(sorted(set(depths))) and len(depths) >= 2, depths
    assert depths == plain.DEPTHS


def test_every_compiled_depth_has_shapes_in_both_kernel_tests():
    depths = compiled_depths()
    lists = {"plain": [shape[2] for shape in plain.SHAPES], "matryoshka": [shape[2] for shape, _ in mat.CASES]}
    for name, ds in lists.items():
        assert all(1 <= d <= 64 * depths[-1] for d in ds), (name, ds)
        for D in depths:
            here = [d for d in ds if depth_of(d, depths) == D]
            assert here, f"{name}: no d dispatches to depth {D}"
            if D > 2:
                assert any((d + 63) // 64 < D for d in here), f"{name}: depth {D} is never entered from below"

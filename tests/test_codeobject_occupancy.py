"""Register, scratch and LDS budgets of the SHIPPED gfx950 code object (CPU).

The guard-free (ALIGNED) TBK=16 / TBN=128 variants of k_enc_fwd_t, k_gc_t and
k_grad_w_t are compiled with __launch_bounds__(512, 8): four 8-wave workgroups
per CU.  That only holds if a thread stays within 64 registers (512 per SIMD
lane / 8 waves), spills nothing, and four workgroups' LDS fits the CU's
160 KB.  The numbers come from the kernel metadata in the code object's notes.
"""

import os
import re
import subprocess

import pytest

from tests.test_codeobject import GEMM_KERNELS, SO_PATH, _extract_hsaco

READELF = "/opt/rocm/lib/llvm/bin/llvm-readelf"

FOUR_PER_CU = ["k_enc_fwd_t", "k_gc_t", "k_grad_w_t"]
LDS_PER_CU = 160 * 1024

_FIELDS = {"vgpr": ".vgpr_count", "agpr": ".agpr_count", "scratch": ".private_segment_fixed_size",
           "lds": ".group_segment_fixed_size", "dynstack": ".uses_dynamic_stack"}


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    """name -> {vgpr, agpr, scratch, lds, dynstack} for every kernel."""
    if not os.path.exists(SO_PATH):
        pytest.skip("extension not built (run python -m sparse_coding_amd.ops.build)")
    if not os.path.exists(READELF):
        pytest.skip("llvm-readelf not available")
    hsaco = _extract_hsaco(tmp_path_factory.mktemp("cobj_occ"))
    out = subprocess.run([READELF, "--notes", hsaco], capture_output=True, text=True, check=True).stdout
    meta = {}
    # one YAML list item per kernel under amdhsa.kernels: it starts at `  - `,
    # its own scalar fields sit at exactly four columns of indent (the nested
    # .args entries, which carry .name fields of their own, sit deeper)
    body = out[out.index("amdhsa.kernels:"):].split("\namdhsa.")[0]
    for item in re.split(r"\n  - ", body)[1:]:
        item = "    " + item
        fields = dict(re.findall(r"^ {4}(\.\w+): +(\S.*?) *$", item, flags=re.M))
        name = fields[".name"].strip("'\"")
        meta[name] = {k: (fields.get(f, "0") == "true" if k == "dynstack" else int(fields.get(f, 0)))
                      for k, f in _FIELDS.items()}
    assert meta, "no kernel metadata in the code object's notes"
    return meta


def _variants(kernels, stem):
    # template instantiations mangle as _Z<len><stem>IL...; the length prefix
    # keeps k_gc_t apart from k_gc_thresh_t
    tag = f"{len(stem)}{stem}I"
    return {n: m for n, m in kernels.items() if tag in n}


def _aligned_16_128(kernels, stem):
    # <TBK=16, MINW, TBN=128, ALIGNED=true>
    hits = {n: m for n, m in _variants(kernels, stem).items()
            if re.search(r"ILi16ELi\d+ELi128ELb1EE", n)}
    assert len(hits) == 1, f"{stem}: expected one aligned TBK=16/TBN=128 variant, found {sorted(hits)}"
    return next(iter(hits.items()))


@pytest.mark.parametrize("stem", FOUR_PER_CU)
def test_aligned_bk16_fits_four_workgroups_per_cu(kernels, stem):
    name, m = _aligned_16_128(kernels, stem)
    print(f"{name}: {m}")
    assert "ILi16ELi8ELi128ELb1EE" in name, f"{stem}: aligned TBK=16 variant is not compiled at 8 waves/SIMD"
    assert m["vgpr"] + m["agpr"] <= 64, f"{name}: {m['vgpr']} VGPRs + {m['agpr']} AGPRs > 64"
    assert m["vgpr"] <= 64
    assert m["scratch"] == 0 and not m["dynstack"], f"{name}: spills ({m['scratch']} B of scratch)"
    assert 4 * m["lds"] <= LDS_PER_CU, f"{name}: 4 x {m['lds']} B of LDS > 160 KB"


@pytest.mark.parametrize("stem", GEMM_KERNELS)
def test_no_gemm_variant_spills(kernels, stem):
    variants = _variants(kernels, stem)
    assert len(variants) >= 2, f"{stem}: variants missing from the code object"
    for name, m in variants.items():
        assert m["scratch"] == 0 and not m["dynstack"], f"{name}: {m['scratch']} B of scratch"


@pytest.mark.parametrize("stem", ["k_enc_fwd_t", "k_dec_fwd_t", "k_gc_t", "k_grad_w_t", "k_gc_thresh_t"])
def test_guarded_and_aligned_variants_present(kernels, stem):
    names = _variants(kernels, stem)
    for tbk in (16, 32):
        for aligned in (0, 1):
            pat = rf"ILi{tbk}ELi\d+ELi128ELb{aligned}EE"
            assert any(re.search(pat, n) for n in names), f"{stem}: no <{tbk}, *, 128, {bool(aligned)}> variant"

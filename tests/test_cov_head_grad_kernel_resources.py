"""The pullback kernels of csrc/cov_heads_grad.hip keep L, the accumulators (S of the log-density, W of the KL) and the solved vectors in
registers with compile-time indices (da is a template argument), as the forward kernels do.  Read off the gfx950 code object (the recipe
of tests/test_cov_head_kernel_resources.py).  CPU only.

  no scratch, no spilled VGPR      every instantiation
  the instantiation count          one per supported da = 1 ... 16 of each templated kernel (the log-density pullback: dense and fused)
  LDS                              none: no kernel of this file declares any
  workgroup bound                  256"""
import os
import re

import pytest

from test_rollout_kernel_resources import LLVM, ROOT, _kernel_meta

OBJ = os.path.join(ROOT, "reinforcementlearning.jl_amd", "build", "cov_heads_grad.o")
DAS = range(1, 17)
KERNELS = {
    "mvnormlogpdf_bwd_kernel": [f"ILi{da}ELi{fused}EE" for da in DAS for fused in (0, 1)],
    "mvnormkl_bwd_kernel": [f"ILi{da}EE" for da in DAS],
    "vec_to_tril_bwd_kernel": [""],
    "diagnormkl_bwd_kernel": [""],
    "normkl_bwd_kernel": [""],
}


@pytest.mark.skipif(not os.path.exists(f"{LLVM}/llvm-readelf"), reason="no llvm-readelf")
def test_cov_head_grad_kernels_keep_everything_in_registers(tmp_path):
    import __graft_entry__ as g

    g.build()
    meta = _kernel_meta(OBJ, str(tmp_path))
    assert len(meta) == 16 * 2 + 16 + 3, sorted(meta)
    bad = []
    for kernel, targs in KERNELS.items():
        mine = {k: v for k, v in meta.items() if re.search(r"\d+" + kernel + r"(I|E)", k)}
        assert len(mine) == len(targs), f"expected {len(targs)} instantiations of {kernel}, found {sorted(mine)}"
        for t in targs:
            assert [k for k in mine if f"{kernel}{t}" in k], f"{kernel}: no instantiation {t}"
        for name, m in mine.items():
            print(f"{name}: {m}")
            if m["scratch"] or m["vspill"]:
                bad.append(f"{name}: {m['scratch']} B of scratch, {m['vspill']} spilled VGPRs")
            if m["lds"] != 0:
                bad.append(f"{name}: {m['lds']} bytes of LDS, declared 0")
            if m["wg"] != 256:
                bad.append(f"{name}: workgroup bound {m['wg']}")
    assert not bad, "\n".join(bad)

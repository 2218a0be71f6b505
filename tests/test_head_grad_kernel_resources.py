"""The pullback kernels of csrc/heads_grad.hip are streaming kernels: one lane per (state, component) with two accumulators, the draw
regenerated in registers.  Read off the gfx950 code object (the recipe of tests/test_cov_head_grad_kernel_resources.py).  CPU only.

  no scratch, no spilled VGPR      every kernel
  the instantiation count          gaussian_head_bwd_kernel<SOFT, SAMPLE> for the four (soft, sampling) pairs, the sampling pullback's
                                   component-pair kernel for soft = 0 / 1, and the two density kernels
  LDS                              none: no kernel of this file declares any
  workgroup bound                  256"""
import os
import re

import pytest

from test_rollout_kernel_resources import LLVM, ROOT, _kernel_meta

OBJ = os.path.join(ROOT, "reinforcementlearning.jl_amd", "build", "heads_grad.o")
KERNELS = {
    "gaussian_head_bwd_kernel": [f"ILi{soft}ELi{sample}EE" for soft in (0, 1) for sample in (0, 1)],
    "gaussian_head_sample_bwd_pair_kernel": ["ILi0EE", "ILi1EE"],
    "normlogpdf_bwd_kernel": [""],
    "diagnormlogpdf_bwd_kernel": [""],
}


@pytest.mark.skipif(not os.path.exists(f"{LLVM}/llvm-readelf"), reason="no llvm-readelf")
def test_head_grad_kernels_keep_everything_in_registers(tmp_path):
    import __graft_entry__ as g

    g.build()
    meta = _kernel_meta(OBJ, str(tmp_path))
    assert len(meta) == 4 + 2 + 2, sorted(meta)
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

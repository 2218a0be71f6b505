"""The kernels of csrc/dqn_batch.hip, read off the gfx950 code object (the recipe of tests/test_head_grad_kernel_resources.py).  CPU only.

  no scratch, no spilled VGPR      every kernel: the gradient tile keeps x (<= 16 inputs) and its accumulators in registers
  the instantiation set            dqn_grad_batch_kernel<NSV, ACT> for NSV = ceil(ns / 4) in {2, 3, 4} x ACT in {0, 1};
                                   dqn_plan_obsn_kernel<ACT, STAGED> for ACT in {0, 1} x {the net staged in LDS, wave-uniform global
                                   loads}; one reduce kernel -- eleven kernels
  workgroup bounds                 1024 (gradient: 16 rows of 16 lanes x 4 = one 64-sample tile), 64 (the staged plan: one wave),
                                   256 (the other plan form, reduce)
  static LDS                       the gradient tile's LDS is dynamic (sized by h and NSV at the launch): 0 declared"""
import os
import re

import pytest

from test_rollout_kernel_resources import LLVM, ROOT, _kernel_meta

OBJ = os.path.join(ROOT, "reinforcementlearning.jl_amd", "build", "dqn_batch.o")
KERNELS = {
    "dqn_grad_batch_kernel": ([f"ILi{nsv}ELi{act}EE" for nsv in (2, 3, 4) for act in (0, 1)], 1024),
    "dqn_plan_obsn_kernel": ([f"ILi{act}ELb{staged}EE" for act in (0, 1) for staged in (0, 1)], {"Lb1E": 64, "Lb0E": 256}),
    "dqn_batch_reduce_kernel": ([""], 256),
}


@pytest.mark.skipif(not os.path.exists(f"{LLVM}/llvm-readelf"), reason="no llvm-readelf")
def test_dqn_batch_kernels_keep_everything_in_registers(tmp_path):
    import __graft_entry__ as g

    g.build()
    meta = _kernel_meta(OBJ, str(tmp_path))
    assert len(meta) == 6 + 4 + 1, sorted(meta)
    bad = []
    for kernel, (targs, wg) in KERNELS.items():
        mine = {k: v for k, v in meta.items() if re.search(r"\d+" + kernel + r"(I|E)", k)}
        assert len(mine) == len(targs), f"expected {len(targs)} instantiations of {kernel}, found {sorted(mine)}"
        for t in targs:
            assert [k for k in mine if f"{kernel}{t}" in k], f"{kernel}: no instantiation {t}"
        for name, m in mine.items():
            print(f"{name}: {m}")
            if m["scratch"] or m["vspill"]:
                bad.append(f"{name}: {m['scratch']} B of scratch, {m['vspill']} spilled VGPRs")
            want = wg if isinstance(wg, int) else next(v for k, v in wg.items() if k in name)
            if m["wg"] != want:
                bad.append(f"{name}: workgroup bound {m['wg']}, declared {want}")
            if kernel == "dqn_grad_batch_kernel" and (m["lds"] != 0 or m["vgpr"] + m["agpr"] > 128):
                bad.append(f"{name}: {m['lds']} B of static LDS (declared 0), {m['vgpr'] + m['agpr']} registers (16 waves per workgroup: <= 128)")
    assert not bad, "\n".join(bad)

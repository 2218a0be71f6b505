"""The kernels of csrc/sac_mlp3.hip, read off the gfx950 code object (the recipe of tests/test_td3_mlp3_kernel_resources.py).  CPU only.

  the instantiation set   sacm_plan_kernel, sacm_target_kernel and sacm_actor_grad_kernel <ACT> (two dW2 accumulator blocks per wave
                          at every h), sacm_critic_grad_kernel <ACT, NBW> (NBW = 2 / 4), one reduce kernel -- eleven kernels
  no scratch, no spills; at most 256 registers at 512 threads; static LDS plus the dynamic LDS of the envelope's corner (h = 256)
  inside 160 KB"""
import os
import re

import pytest

from test_rollout_kernel_resources import LLVM, ROOT, _kernel_meta
from test_td3_mlp3_kernel_resources import SLOT, TILE

OBJ = os.path.join(ROOT, "reinforcementlearning.jl_amd", "build", "sac_mlp3.o")
ACTS = [f"ILi{a}EE" for a in (0, 1)]
# kernel -> (template arguments, workgroup size, dynamic LDS at h = 256)
KERNELS = {"sacm_plan_kernel": (ACTS, 512, SLOT + 2 * TILE), "sacm_target_kernel": (ACTS, 512, 3 * SLOT + 2 * TILE),
           "sacm_critic_grad_kernel": ([f"ILi{a}ELi{b}EE" for a in (0, 1) for b in (2, 4)], 512, SLOT + 3 * TILE),
           "sacm_actor_grad_kernel": (ACTS, 512, 3 * SLOT + 3 * TILE), "sacm_reduce_kernel": ([""], 256, 0)}


@pytest.mark.skipif(not os.path.exists(f"{LLVM}/llvm-readelf"), reason="no llvm-readelf")
def test_sac_mlp3_kernels_keep_everything_in_registers_and_fit_the_lds(tmp_path):
    import __graft_entry__ as g

    g.build()
    meta = _kernel_meta(OBJ, str(tmp_path))
    assert len(meta) == 11, sorted(meta)
    bad = []
    for kernel, (targs, wg, dyn) in KERNELS.items():
        mine = {k: v for k, v in meta.items() if re.search(r"\d+" + kernel + r"(I|E)", k)}
        assert len(mine) == len(targs) and all([k for k in mine if f"{kernel}{t}" in k] for t in targs), f"{kernel}: found {sorted(mine)}"
        for name, m in mine.items():
            print(f"{name}: {m}")
            if m["scratch"] or m["vspill"] or m["wg"] != wg or m["lds"] + dyn > 163840 or (wg == 512 and m["vgpr"] + m["agpr"] > 256):
                bad.append(f"{name}: {m}")
    assert not bad, "\n".join(bad)

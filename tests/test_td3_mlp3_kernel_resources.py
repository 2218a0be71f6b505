"""The kernels of csrc/td3_mlp3.hip, read off the gfx950 code object (the recipe of tests/test_td3_kernel_resources.py).  CPU only.

  the instantiation set   td3m_plan_kernel <ACT>, td3m_target_kernel <ACT, NC>, td3m_critic_grad_kernel and td3m_actor_grad_kernel
                          <ACT, NBW> (NBW = 2 / 4 dW2 accumulator blocks per wave), one reduce kernel -- fifteen kernels
  no scratch, no spills; at most 256 registers at 512 threads; static LDS plus the dynamic LDS of the envelope's corner (h = 256)
  inside 160 KB"""
import os
import re

import pytest

from test_rollout_kernel_resources import LLVM, ROOT, _kernel_meta

OBJ = os.path.join(ROOT, "reinforcementlearning.jl_amd", "build", "td3_mlp3.o")
TILE = 4 * 32 * 257  # one 32 x (h + 1) tile at h = 256, bytes
SLOT = 4 * (8 * 256 + 4)  # one network slot
# kernel -> (template arguments, workgroup size, dynamic LDS at h = 256)
KERNELS = {"td3m_plan_kernel": ([f"ILi{a}EE" for a in (0, 1)], 512, SLOT + 2 * TILE),
           "td3m_target_kernel": ([f"ILi{a}ELi{nc}EE" for a in (0, 1) for nc in (1, 2)], 512, 3 * SLOT + 2 * TILE),
           "td3m_critic_grad_kernel": ([f"ILi{a}ELi{b}EE" for a in (0, 1) for b in (2, 4)], 512, SLOT + 3 * TILE),
           "td3m_actor_grad_kernel": ([f"ILi{a}ELi{b}EE" for a in (0, 1) for b in (2, 4)], 512, 2 * SLOT + 3 * TILE),
           "td3m_reduce_kernel": ([""], 256, 0)}


@pytest.mark.skipif(not os.path.exists(f"{LLVM}/llvm-readelf"), reason="no llvm-readelf")
def test_td3_mlp3_kernels_keep_everything_in_registers_and_fit_the_lds(tmp_path):
    import __graft_entry__ as g

    g.build()
    meta = _kernel_meta(OBJ, str(tmp_path))
    assert len(meta) == 15, sorted(meta)
    bad = []
    for kernel, (targs, wg, dyn) in KERNELS.items():
        mine = {k: v for k, v in meta.items() if re.search(r"\d+" + kernel + r"(I|E)", k)}
        assert len(mine) == len(targs), f"expected {len(targs)} instantiations of {kernel}, found {sorted(mine)}"
        for t in targs:
            assert [k for k in mine if f"{kernel}{t}" in k], f"{kernel}: no instantiation {t}"
        for name, m in mine.items():
            print(f"{name}: {m}")
            if m["scratch"] or m["vspill"] or m["wg"] != wg or m["lds"] + dyn > 163840 or (wg == 512 and m["vgpr"] + m["agpr"] > 256):
                bad.append(f"{name}: {m}")
    assert not bad, "\n".join(bad)

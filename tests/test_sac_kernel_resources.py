"""The kernels of csrc/sac.hip, read off the gfx950 code object (the recipe of tests/test_dqn_batch_kernel_resources.py).  CPU only.

  no scratch, no spilled VGPR      every kernel: a lane keeps its sample's inputs (<= 5) and its gradient chains in registers
  the instantiation set            sac_plan_kernel, sac_critic_grad_kernel, sac_actor_grad_kernel <NS, ACT> for NS in {2, 3, 4} x ACT in
                                   {0, 1}; one reduce kernel -- nineteen kernels
  workgroup bounds                 64 (plan: one wave per workgroup, the actor staged in LDS), 512 (the gradient tiles), 256 (reduce)
  LDS                              static, sized for h = 256: the critic launch stages five networks (the actor, Q1, Q2, Qt1, Qt2) and
                                   must stay inside the 64 KB a kernel gets without opting in, far inside the CU's 160 KB"""
import os
import re

import pytest

from test_rollout_kernel_resources import LLVM, ROOT, _kernel_meta

OBJ = os.path.join(ROOT, "reinforcementlearning.jl_amd", "build", "sac.o")
SHAPES = [f"ILi{ns}ELi{act}EE" for ns in (2, 3, 4) for act in (0, 1)]
KERNELS = {"sac_plan_kernel": (SHAPES, 64), "sac_critic_grad_kernel": (SHAPES, 512), "sac_actor_grad_kernel": (SHAPES, 512),
           "sac_reduce_kernel": ([""], 256)}


@pytest.mark.skipif(not os.path.exists(f"{LLVM}/llvm-readelf"), reason="no llvm-readelf")
def test_sac_kernels_keep_everything_in_registers_and_fit_the_lds(tmp_path):
    import __graft_entry__ as g

    g.build()
    meta = _kernel_meta(OBJ, str(tmp_path))
    assert len(meta) == 3 * 6 + 1, sorted(meta)
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
            if m["wg"] != wg:
                bad.append(f"{name}: workgroup bound {m['wg']}, declared {wg}")
            if m["lds"] > 64 * 1024:
                bad.append(f"{name}: {m['lds']} B of static LDS (more than 64 KB needs an opt-in the launches do not make)")
            if wg == 512 and m["vgpr"] + m["agpr"] > 256:
                bad.append(f"{name}: {m['vgpr'] + m['agpr']} registers (8 waves per workgroup are two per SIMD: <= 256)")
    assert not bad, "\n".join(bad)

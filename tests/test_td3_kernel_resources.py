"""The kernels of csrc/td3.hip, read off the gfx950 code object (the recipe of tests/test_sac_kernel_resources.py).  CPU only.

  the instantiation set   td3_plan_kernel and td3_actor_grad_kernel <NS, ACT>, td3_critic_grad_kernel <NS, ACT, NC> for NS in {2, 3, 4} x
                          ACT in {0, 1} x NC in {1, 2}; one reduce kernel -- twenty-five kernels
  workgroup bounds        64 (plan), 512 (the gradient tiles: 32 rows of 16 lanes), 256 (reduce)
  no scratch, no spills; at most 256 registers at 512 threads; static LDS (sized for h = 256, five staged networks) inside 64 KB"""
import os
import re

import pytest

from test_rollout_kernel_resources import LLVM, ROOT, _kernel_meta

OBJ = os.path.join(ROOT, "reinforcementlearning.jl_amd", "build", "td3.o")
SHAPES = [f"ILi{ns}ELi{act}E" for ns in (2, 3, 4) for act in (0, 1)]
KERNELS = {"td3_plan_kernel": ([s + "E" for s in SHAPES], 64), "td3_actor_grad_kernel": ([s + "E" for s in SHAPES], 512),
           "td3_critic_grad_kernel": ([f"{s}Li{nc}EE" for s in SHAPES for nc in (1, 2)], 512), "td3_reduce_kernel": ([""], 256)}


@pytest.mark.skipif(not os.path.exists(f"{LLVM}/llvm-readelf"), reason="no llvm-readelf")
def test_td3_kernels_keep_everything_in_registers_and_fit_the_lds(tmp_path):
    import __graft_entry__ as g

    g.build()
    meta = _kernel_meta(OBJ, str(tmp_path))
    assert len(meta) == 25, sorted(meta)
    bad = []
    for kernel, (targs, wg) in KERNELS.items():
        mine = {k: v for k, v in meta.items() if re.search(r"\d+" + kernel + r"(I|E)", k)}
        assert len(mine) == len(targs), f"expected {len(targs)} instantiations of {kernel}, found {sorted(mine)}"
        for t in targs:
            assert [k for k in mine if f"{kernel}{t}" in k], f"{kernel}: no instantiation {t}"
        for name, m in mine.items():
            print(f"{name}: {m}")
            if m["scratch"] or m["vspill"] or m["wg"] != wg or m["lds"] > 64 * 1024 or (wg == 512 and m["vgpr"] + m["agpr"] > 256):
                bad.append(f"{name}: {m}")
    assert not bad, "\n".join(bad)

"""The kernels of csrc/qrdqn.hip, read off the gfx950 code object (the recipe of tests/test_c51_kernel_resources.py).  CPU only.

  the instantiation set            qrdqn_plan_kernel<ACT> and qrdqn_grad_kernel<ACT> for ACT in {0, 1}; one reduce kernel -- five kernels
  workgroup bounds                 256 (plan: 16 envs per workgroup, thread = output row), 256 (the gradient tiles), 256 (reduce)
  no scratch, no spilled VGPR      every kernel; at most 256 registers (the weights in flight live in them): two workgroups per CU
  LDS                              static, sized for h = 256 and 256 rows, inside the 64 KB a kernel gets without opting in; the gradient
                                   kernel's at most 40 KB
The numbers are recorded in profiles/qrdqn.md."""
import os
import re

import pytest

from test_rollout_kernel_resources import LLVM, ROOT, _kernel_meta

OBJ = os.path.join(ROOT, "reinforcementlearning.jl_amd", "build", "qrdqn.o")
ACTS = [f"ILi{act}EE" for act in (0, 1)]
KERNELS = {"qrdqn_plan_kernel": (ACTS, 256), "qrdqn_grad_kernel": (ACTS, 256), "qrdqn_reduce_kernel": ([""], 256)}


@pytest.mark.skipif(not os.path.exists(f"{LLVM}/llvm-readelf"), reason="no llvm-readelf")
def test_qrdqn_kernels_keep_everything_in_registers_and_fit_the_lds(tmp_path):
    import __graft_entry__ as g

    g.build()
    meta = _kernel_meta(OBJ, str(tmp_path))
    assert len(meta) == 5, sorted(meta)
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
                bad.append(f"{name}: {m['lds']} B of static LDS (more than 64 KB needs an opt-in the launch does not make for static LDS)")
            if m["vgpr"] + m["agpr"] > 256:
                bad.append(f"{name}: {m['vgpr'] + m['agpr']} registers (two waves per SIMD: <= 256)")
    assert not bad, "\n".join(bad)
    assert all(m["lds"] <= 40 * 1024 for k, m in meta.items() if "qrdqn_grad_kernel" in k)

"""The DQN replay fold kernels are assembled from the forced-inline stages of csrc/fold_device.h; what the assembly must not cost is
read off the gfx950 code objects (the recipe of tests/test_rollout_kernel_resources.py: llvm-readelf on the kernel descriptors'
metadata).  CPU only.

  no scratch, no spilled VGPR      every instantiation: a spill in the window walk or the two-net forward is a scratch round trip on
                                   a dependent chain
  <= 128 VGPRs                     the two 1024-thread kernels: 16 waves per workgroup = 4 per SIMD, 512 / 4 registers per lane
                                   (profiles/fused_folds.md)
  LDS                              exactly the declared arrays: l_rec 2 x 256 x 48 = 24 576, the three record quarters 3 x 64 x 16 =
                                   3 072, the reward column 32 x 64 x 4 = 8 192 (a stage that made a private copy would show here)"""
import os

import pytest

from test_rollout_kernel_resources import LLVM, ROOT, _kernel_meta

BUILD = os.path.join(ROOT, "reinforcementlearning.jl_amd", "build")
L_REC, L_QUARTERS, L_REW = 2 * 256 * 3 * 16, 3 * 64 * 16, 32 * 64 * 4
# kernel -> (object, instantiations, 1024-thread tile kernel, LDS bytes by instantiation)
KERNELS = {
    "dqn_fold_double_kernel": ("dqn_double.o", 3 * 2, True, lambda name: L_REC + L_QUARTERS),
    # <NS, ACT, DBL>: the last template argument says whether the nets are staged
    "dqn_sample_fold_kernel": ("dqn_sample_fold.o", 3 * 2 * 2, True,
                               lambda name: L_QUARTERS + L_REW + (L_REC if "ELb1EE" in name else 0)),
    "per_sample_fold_nstep_kernel": ("per_nstep.o", 1, False, lambda name: L_REW),
    "fold_nstep_kernel": ("ring.o", 1, False, lambda name: 0),
    "fold_double_select_kernel": ("dqn_double.o", 1, False, lambda name: 0),
}


@pytest.mark.skipif(not os.path.exists(f"{LLVM}/llvm-readelf"), reason="no llvm-readelf")
@pytest.mark.parametrize("kernel", list(KERNELS))
def test_fold_kernels_keep_their_registers_and_lds(kernel, tmp_path):
    import __graft_entry__ as g

    g.build()
    obj, count, tiled, lds = KERNELS[kernel]
    meta = {k: v for k, v in _kernel_meta(os.path.join(BUILD, obj), str(tmp_path)).items() if kernel in k}
    assert len(meta) == count, f"expected {count} instantiations of {kernel}, found {sorted(meta)}"
    bad = []
    for name, m in meta.items():
        print(f"{name}: {m}")
        if m["scratch"] or m["vspill"]:
            bad.append(f"{name}: {m['scratch']} B of scratch, {m['vspill']} spilled VGPRs")
        if tiled and (m["wg"] != 1024 or m["vgpr"] + m["agpr"] > 128):
            bad.append(f"{name}: workgroup bound {m['wg']}, {m['vgpr'] + m['agpr']} registers per lane (4 waves per SIMD need <= 128)")
        if m["lds"] != lds(name):
            bad.append(f"{name}: {m['lds']} bytes of LDS, declared {lds(name)}")
    assert not bad, "\n".join(bad)

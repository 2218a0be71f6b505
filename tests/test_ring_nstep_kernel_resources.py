"""What the n-step gathers of csrc/ring_nstep.hip must not cost, read off the gfx950 code object (the recipe of
tests/test_fold_kernel_resources.py: llvm-readelf on the kernel descriptors' metadata).  CPU only.

  no scratch, no spilled VGPR   a dynamically indexed register array (the window's rewards) would show here: they wait in LDS
  LDS                           exactly the declared arrays (a private copy of a staged table would show here):
      gather_small_nstep_kernel<E>   l_ps, l_pn 2 x 256 x 8 = 4 096; the reward columns 32 x 256 x 4 = 32 768
      gather_frames_nstep_kernel     l_rew 32 x 4 = 128; l_next 2 x 8 = 16
      gather_stacked_nstep_kernel    l_rew 128; l_off 18 x 8 = 144; l_ks, l_kn 2 x 16 x 4 = 128"""
import os

import pytest

from test_rollout_kernel_resources import LLVM, ROOT, _kernel_meta

OBJ = os.path.join(ROOT, "reinforcementlearning.jl_amd", "build", "ring_nstep.o")
# kernel -> (instantiations, LDS bytes)
KERNELS = {
    "gather_small_nstep_kernel": (2, 2 * 256 * 8 + 32 * 256 * 4),
    "gather_frames_nstep_kernel": (1, 32 * 4 + 2 * 8),
    "gather_stacked_nstep_kernel": (1, 32 * 4 + 18 * 8 + 2 * 16 * 4),
}


@pytest.mark.skipif(not os.path.exists(f"{LLVM}/llvm-readelf"), reason="no llvm-readelf")
def test_nstep_gather_kernels_keep_their_registers_and_lds(tmp_path):
    import __graft_entry__ as g

    g.build()
    meta = _kernel_meta(OBJ, str(tmp_path))
    assert all(any(k in name for k in KERNELS) for name in meta), f"a kernel of ring_nstep.o this test does not know: {sorted(meta)}"
    bad = []
    for kernel, (count, lds) in KERNELS.items():
        mine = {k: v for k, v in meta.items() if kernel in k}
        assert len(mine) == count, f"expected {count} instantiations of {kernel}, found {sorted(mine)}"
        for name, m in mine.items():
            print(f"{name}: {m}")
            if m["scratch"] or m["vspill"]:
                bad.append(f"{name}: {m['scratch']} B of scratch, {m['vspill']} spilled VGPRs")
            if m["wg"] != 256:
                bad.append(f"{name}: workgroup bound {m['wg']}")
            if m["lds"] != lds:
                bad.append(f"{name}: {m['lds']} bytes of LDS, declared {lds}")
    assert not bad, "\n".join(bad)

"""The kernels of csrc/dist.hip, read off the gfx950 code object (the recipe of tests/test_c51_kernel_resources.py).  CPU only.

  the default build        dist_reduce_kernel alone: the reduction of the partial rows that the C51, QR-DQN and IQN gradient launches share
  the bounds build         dist_count_bad_actions_kernel beside it (RLHIP_BOUNDS_CHECK is named in dist.hip itself: build.py recompiles the
                           sources whose own text names the variant's macro)
  every kernel             workgroup bound 256, no scratch, no spilled VGPR, at most 256 registers, no LDS beyond 64 KB"""
import os
import re

import pytest

from test_rollout_kernel_resources import LLVM, ROOT, _kernel_meta

PKG = os.path.join(ROOT, "reinforcementlearning.jl_amd")
BUILDS = {"build": ["dist_reduce_kernel"], "build_bounds": ["dist_reduce_kernel", "dist_count_bad_actions_kernel"]}


@pytest.mark.skipif(not os.path.exists(f"{LLVM}/llvm-readelf"), reason="no llvm-readelf")
@pytest.mark.parametrize("build", list(BUILDS))
def test_dist_kernels_keep_everything_in_registers(build, tmp_path):
    import __graft_entry__ as g

    g.build()
    meta = _kernel_meta(os.path.join(PKG, build, "dist.o"), str(tmp_path))
    assert len(meta) == len(BUILDS[build]), sorted(meta)
    bad = []
    for kernel in BUILDS[build]:
        mine = {k: v for k, v in meta.items() if re.search(r"\d+" + kernel + r"E", k)}
        assert len(mine) == 1, f"expected one {kernel}, found {sorted(mine)}"
        for name, m in mine.items():
            print(f"{name}: {m}")
            if m["scratch"] or m["vspill"]:
                bad.append(f"{name}: {m['scratch']} B of scratch, {m['vspill']} spilled VGPRs")
            if m["wg"] != 256:
                bad.append(f"{name}: workgroup bound {m['wg']}, declared 256")
            if m["lds"] > 64 * 1024:
                bad.append(f"{name}: {m['lds']} B of static LDS")
            if m["vgpr"] + m["agpr"] > 256:
                bad.append(f"{name}: {m['vgpr'] + m['agpr']} registers (two waves per SIMD: <= 256)")
    assert not bad, "\n".join(bad)

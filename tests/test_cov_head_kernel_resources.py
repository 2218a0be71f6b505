"""The kernels of csrc/cov_heads.hip keep the lower triangle of L, the draws and the solved rows in registers with compile-time indices
(da is a template argument): a runtime-indexed private array would land in scratch, a round trip per element on a dependent chain.
Read off the gfx950 code object (the recipe of tests/test_fold_kernel_resources.py).  CPU only.

  no scratch, no spilled VGPR      every instantiation
  the instantiation count          one per supported da = 1 ... 16 of each templated kernel: a dropped da shows here
  LDS                              the head kernels: exactly the block's diagonals, da x 256 floats; the staged (state, action) kernels
                                   (da = 6 ... 12): the block's Cholesky vectors at an odd row stride, 256 (da <= 10) or 128 rows;
                                   nothing elsewhere"""
import os
import re

import pytest

from test_rollout_kernel_resources import LLVM, ROOT, _kernel_meta

OBJ = os.path.join(ROOT, "reinforcementlearning.jl_amd", "build", "cov_heads.o")
DAS = range(1, 17)
# kernel -> the template argument lists its instantiations must carry (Itanium mangling: ILi<da>E..., ILi<da>ELi<eval>EE)
KERNELS = {
    "cov_head_kernel": [f"ILi{da}ELi{ev}EE" for da in DAS for ev in (0, 1)],
    "cov_head_staged_kernel": [f"ILi{da}ELi1EE" for da in range(6, 13)],
    "mvnormlogpdf_kernel": [f"ILi{da}EE" for da in DAS],
    "mvnormkl_kernel": [f"ILi{da}EE" for da in DAS],
    "vec_to_tril_kernel": [""],
    "diagnormkl_kernel": [""],
    "normkl_kernel": [""],
}


@pytest.mark.skipif(not os.path.exists(f"{LLVM}/llvm-readelf"), reason="no llvm-readelf")
def test_cov_head_kernels_keep_everything_in_registers(tmp_path):
    import __graft_entry__ as g

    g.build()
    meta = _kernel_meta(OBJ, str(tmp_path))
    assert len(meta) == 16 * 2 + 7 + 16 + 16 + 3, sorted(meta)
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
            da = re.search(r"cov_head_kernelILi(\d+)E", name)
            lds, wg = int(da.group(1)) * 256 * 4 if da else 0, 256
            st = re.search(r"cov_head_staged_kernelILi(\d+)E", name)
            if st:
                nvp = (int(st.group(1)) * (int(st.group(1)) + 1) // 2) | 1
                wg = 256 if nvp * 4 * 256 <= 65536 else 128
                lds = nvp * 4 * wg
            if m["lds"] != lds:
                bad.append(f"{name}: {m['lds']} bytes of LDS, declared {lds}")
            if m["wg"] != wg:
                bad.append(f"{name}: workgroup bound {m['wg']}")
    assert not bad, "\n".join(bad)

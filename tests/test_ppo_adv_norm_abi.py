"""The ABI surface of PPO advantage normalisation (rlhip_ppo_cfg.normalize_advantage = 1, csrc/ppo_advnorm.hip), CPU only:
parameter and workspace sizes, the sharded entry points' refusal at world > 1, the binding of the new entry point in the
header, the Python and Julia glue and INTEGRATION.md, and the new kernels' resources read off the gfx950 code object."""
import ctypes as C
import os
import re
import subprocess
import types

import pytest

from rlhip import _lib
from rlhip.ppo import PPOPolicy, make_ppo_cfg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = "/opt/rocm/lib/llvm/bin"
SYM = "rlhip_ppo_adv_normalize_f32"


def _ws(kind, cfg, n, T):
    return int(_lib.lib.rlhip_ppo_workspace_bytes(kind, C.byref(cfg), n, T))


def _with_flag(w_off, n, T, nmb):
    """the size documented in include/rlhip.h: the flag-off size rounded up to 256, the plane, the scratch"""
    r256 = lambda b: (b + 255) // 256 * 256  # noqa: E731
    total, bm = n * T, n * T // nmb
    if nmb <= 64:
        s = r256(4 * total) + r256(8 * ((total + 1023) // 1024) * nmb + 16 * nmb) + 256
    else:
        s = r256(16 * nmb * ((bm + 2047) // 2048 + 1))
    return r256(w_off) + r256(4 * total) + s


@pytest.mark.parametrize("kind,cont,layers,hidden", [(0, 0, 2, 64), (0, 0, 2, 128), (0, 0, 2, 256), (1, 1, 2, 256),
                                                     (2, 0, 2, 64), (0, 0, 3, 128), (1, 1, 3, 128), (0, 0, 3, 256),
                                                     (1, 1, 3, 256)])
@pytest.mark.parametrize("n,T,nmb", [(256, 16, 4), (4096, 32, 4), (4096, 128, 4), (100, 7, 3), (1, 1, 1), (256, 16, 100),
                                     (97, 13, 5)])
def test_sizes_accept_the_flag_and_grow_by_the_documented_region(kind, cont, layers, hidden, n, T, nmb):
    off = make_ppo_cfg(continuous=cont, layers=layers, hidden=hidden, n_microbatches=nmb)
    on = make_ppo_cfg(continuous=cont, layers=layers, hidden=hidden, n_microbatches=nmb, normalize_advantage=1)
    np_off = int(_lib.lib.rlhip_ppo_nparams(kind, C.byref(off)))
    assert np_off > 0 and int(_lib.lib.rlhip_ppo_nparams(kind, C.byref(on))) == np_off
    w_off, w_on = _ws(kind, off, n, T), _ws(kind, on, n, T)
    assert w_off > 0
    assert w_on == _with_flag(w_off, n, T, nmb)


def test_flag_values_other_than_0_and_1_are_refused():
    bad = make_ppo_cfg(normalize_advantage=2)
    assert int(_lib.lib.rlhip_ppo_nparams(0, C.byref(bad))) < 0


def test_sharded_update_refuses_world_above_one_before_any_device_work():
    on = make_ppo_cfg(normalize_advantage=1)
    traj = _lib.PPOTraj()
    # every pointer NULL: the refusal comes before the argument checks, let alone a launch
    rc = _lib.lib.rlhip_ppo_update_p2p_f32(0, C.byref(on), 256, 16, C.byref(traj), None, None, None, None, 0, 0, None, None,
                                          None, 0, 2, None, 1 << 20, 0, 1000, None, None)
    assert rc == -1 and b"world > 1" in _lib.lib.rlhip_last_error()
    # world = 1 is allowed: it fails on the NULL pointers instead
    rc = _lib.lib.rlhip_ppo_update_p2p_f32(0, C.byref(on), 256, 16, C.byref(traj), None, None, None, None, 0, 0, None, None,
                                          None, 0, 1, None, 1 << 20, 0, 1000, None, None)
    assert rc == -1 and b"world > 1" not in _lib.lib.rlhip_last_error()


def test_python_host_refuses_a_process_group_of_world_above_one(monkeypatch):
    import torch.distributed as dist

    monkeypatch.setattr(dist, "get_world_size", lambda group=None: 2)
    env = types.SimpleNamespace(kind=0, continuous=False, seed=1, device="cpu")  # never reaches a device
    with pytest.raises(_lib.RLHipArgumentError, match="world > 1"):
        PPOPolicy(env, update_freq=8, process_group=object(), normalize_advantage=1)


def test_julia_host_refuses_a_communicator_of_world_above_one():
    src = open(os.path.join(ROOT, "reinforcementlearning.jl_amd", "julia", "RLHip.jl")).read()
    ctor = src[src.index("function HipPPOPolicy(env::HipVecEnv"):]
    ctor = ctor[:ctor.index("\nend\n")]
    refusal = ctor.index("normalize_advantage != 0 && comm !== nothing && comm.world > 1")
    assert refusal < ctor.index("DevBuf"), "the refusal must come before the first device allocation"
    assert f"ccall((:{SYM}, LIB)" in src


def test_entry_point_is_declared_bound_and_counted():
    syms = _lib.declared_symbols()
    assert SYM in syms and SYM in _lib._PROTOS and hasattr(_lib.lib, SYM)
    assert hasattr(PPOPolicy, "normalize_advantage_")
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert int(re.search(r"\((\d+) `extern \"C\"` entry points", text).group(1)) == len(syms)
    assert SYM in text
    hdr = open(os.path.join(ROOT, "include", "rlhip.h")).read()
    assert "reserved, must be 0" not in hdr


@pytest.mark.skipif(not os.path.exists(f"{LLVM}/llvm-readelf"), reason="no llvm-readelf")
def test_advnorm_kernels_have_no_scratch_or_spills(tmp_path):
    import __graft_entry__ as g

    g.build()
    obj = os.path.join(ROOT, "reinforcementlearning.jl_amd", "build", "ppo_advnorm.o")
    fat, co = str(tmp_path / "a.fatbin"), str(tmp_path / "a.co")
    subprocess.run([f"{LLVM}/llvm-objcopy", f"--dump-section=.hip_fatbin={fat}", obj], check=True, capture_output=True)
    subprocess.run([f"{LLVM}/clang-offload-bundler", "--type=o", "--unbundle", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
                    f"--input={fat}", f"--output={co}"], check=True, capture_output=True)
    notes = subprocess.run([f"{LLVM}/llvm-readelf", "--notes", co], check=True, capture_output=True, text=True).stdout
    seen = 0
    for blk in notes.split("  - .agpr_count")[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        if "ppo_advnorm" not in name:
            continue
        seen += 1
        num = lambda key: int(re.search(key + r":\s+(\d+)", blk).group(1))  # noqa: E731
        assert num(r"\.private_segment_fixed_size") == 0, name
        assert num(r"\.vgpr_spill_count") == 0 and num(r"\.sgpr_spill_count") == 0, name
    assert seen == 6  # the binned and the gather form, three passes each

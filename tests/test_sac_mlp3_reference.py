"""The judge of tests/test_gpu_sac_mlp3.py, with no device: for every case the Float32 and the Float64 run of tests/sac_mlp3_ref.py
take the same decisions (sel, the smaller target critic, the clamp's `pass` at s and s'), so that a case's Float32 floor measures
rounding and nothing else; every case with more than one sample selects both critics and holds a terminal transition, the clamp case
passes and clamps; the header's pullback lines are the derivative of the plain formulas; and the C boundary refuses the envelope's
edges before any launch."""
import ctypes as C

import pytest

import sac_mlp3_ref as R
import sac_ref
import td3_mlp3_ref as T
from test_iqn_abi import CTYPES, FAKE, _lib
from test_julia_glue_signatures import header_prototypes
from test_sac_reference import sample

SEED, STEP = 77, 5


@pytest.mark.parametrize("name", list(R.CASES))
def test_the_model_decides_alike_in_both_precisions_and_differentiates_the_plain_formulas(name):
    c = R.build(name)
    rec, (eps0, eps1) = T.records(c, c["idx"]), sac_ref.draw_pair(sample, c["batch"], SEED + 1, STEP)
    rc, ra, fl, same = R.floors(c, rec, eps0, eps1)
    print(f"sac_mlp3 {name}: Float32 floors " + ", ".join(f"{k} {v:.2e}" for k, v in fl.items()))
    assert same, f"{name}: the Float32 and Float64 models decide differently (pick another seed)"
    assert rec[3][0] != 0, "no terminal transition"
    if c["batch"] > 1:  # (one sample selects one critic)
        assert set(ra["sel"]) == {1, 2} and 0 < rec[3].sum() < c["batch"]
    if name == "clamp":
        assert 0 < ra["ok"].sum() < c["batch"] and 0 < rc["ok"].sum() < c["batch"]
    if c["h"] <= 96:  # (the formulas do not depend on the width)
        assert T.rel(R.actor_by_the_header(c, rec, eps1), ra["grad"]) <= 1e-12, "the header's pullback is not the gradient"


def test_the_entry_points_have_their_namesakes_signatures_and_refuse_the_envelope():
    lib, protos = _lib(), header_prototypes()
    for name in ("workspace_bytes", "plan_f32", "critic_grad_f32", "actor_grad_f32"):
        (ret, args), (res, argtypes) = protos["rlhip_sac_mlp3_" + name], lib._PROTOS["rlhip_sac_mlp3_" + name]
        assert protos["rlhip_sac_" + name] == (ret, args), "the signatures are those of the two-layer namesakes"
        assert res is CTYPES[ret] and [CTYPES[x] for x in args] == [C.c_void_p if issubclass(t, C._Pointer) else t for t in argtypes]
    ws = lib.lib.rlhip_sac_mlp3_workspace_bytes
    assert ws(3, 64, 64) > 0 and all(ws(*a) == -1 for a in ((1, 64, 64), (5, 64, 64), (3, 16, 64), (3, 48, 64), (3, 288, 64), (3, 64, 0)))
    ring = lib.Ring(capacity=8, n_env=4, obs_dim=3, len_rt=4, elem_bytes=4, layout=2, state=FAKE)
    with pytest.raises(lib.RLHipArgumentError, match="multiple of 32"):  # (before any launch: the pointers are never followed)
        lib.call("rlhip_sac_mlp3_actor_grad_f32", C.byref(ring), 48, 0, FAKE, FAKE, 64, FAKE, FAKE, 0.0, 1.0, 1.0, 1, 0, 0.0, 0.0, None, FAKE,
                 FAKE, FAKE, None, None, None)

"""The C boundary of the three-layer TD3 / DDPG entry points and the judge of their device tests, with no device: header, ctypes
table and library agree; every edge of the envelope is -1 from rlhip_td3_mlp3_workspace_bytes and RLHIP_EINVAL from the launching
entries before any launch (the pointers handed over are never followed); for every case of tests/test_gpu_td3_mlp3.py the Float32
and the Float64 run of tests/td3_mlp3_ref.py take the same decisions (the smaller target critic, the clamp of u', the sign of every
relu pre-activation of both hidden layers), so that the Float32 floor of the case measures rounding and nothing else."""
import ctypes as C

import numpy as np
import pytest

import heads_grad_ref as G
import td3_mlp3_ref as R
from test_iqn_abi import CTYPES, FAKE, _lib
from test_julia_glue_signatures import header_prototypes
from test_sac_reference import sample

ENTRIES = ("rlhip_td3_mlp3_workspace_bytes", "rlhip_td3_mlp3_plan_f32", "rlhip_td3_mlp3_critic_grad_f32", "rlhip_td3_mlp3_actor_grad_f32")
OK = dict(ns=3, h=64, nc=2, batch=64, layout=None, null=None)
EDGES = [dict(ns=1), dict(ns=5), dict(h=0), dict(h=16), dict(h=48), dict(h=288), dict(nc=0), dict(nc=3), dict(batch=0)]
SEED, STEP = 77, 5


def test_header_ctypes_table_and_library_agree():
    lib, protos = _lib(), header_prototypes()
    assert lib.lib.rlhip_abi_version() == 2
    for name in ENTRIES:
        assert name in protos and name in lib.declared_symbols() and hasattr(lib.lib, name), f"{name} is not declared and exported"
        (ret, args), (res, argtypes) = protos[name], lib._PROTOS[name]
        argtypes = [C.c_void_p if issubclass(t, C._Pointer) else t for t in argtypes]  # (POINTER(Ring) is a pointer to the header)
        assert res is CTYPES[ret] and [CTYPES[a] for a in args] == argtypes, f"{name}: the ctypes table differs from the header"


@pytest.mark.parametrize("kw", EDGES + [dict(layout=0)] +  # (0: RLHIP_RING_FRAMES)
                         [dict(null=k) for k in ("actor", "critics", "targets", "idx", "ws", "grad", "stats", "obs", "action")], ids=str)
def test_every_edge_of_the_envelope_is_refused_before_any_launch(kw):
    a, lib = dict(OK, **kw), _lib()
    ws = lib.lib.rlhip_td3_mlp3_workspace_bytes
    assert ws(OK["ns"], OK["h"], OK["nc"], OK["batch"]) > 0
    if kw.keys() & {"ns", "h", "nc", "batch"}:
        assert ws(a["ns"], a["h"], a["nc"], a["batch"]) == -1
    ring = lib.Ring(capacity=8, n_env=4, obs_dim=a["ns"], len_rt=4, elem_bytes=4, layout=2 if a["layout"] is None else a["layout"], state=FAKE)
    p = lambda k: None if a["null"] == k else FAKE  # noqa: E731
    plan = lambda: lib.call("rlhip_td3_mlp3_plan_f32", p("actor"), a["ns"], a["h"], 0, p("obs"), 8, 1.0, 0.1, -1.0, 1.0, 0, 1, 0, 0,  # noqa: E731
                            p("action"), None, None)
    critic = lambda: lib.call("rlhip_td3_mlp3_critic_grad_f32", C.byref(ring), a["h"], 0, a["nc"], p("actor"), p("critics"),  # noqa: E731
                              p("targets"), a["batch"], p("idx"), 0.99, 1.0, 0.2, 0.5, -1.0, 1.0, 1, 0, p("ws"), p("grad"), p("stats"),
                              None, None, None)
    actor = lambda: lib.call("rlhip_td3_mlp3_actor_grad_f32", C.byref(ring), a["h"], 0, p("actor"), p("critics"), a["batch"], p("idx"),  # noqa: E731
                             1.0, p("ws"), p("grad"), p("stats"), None)
    null = kw.get("null")
    entries = ([critic] if null not in ("obs", "action") else []) + ([actor] if "nc" not in kw and null not in ("targets", "obs", "action") else [])
    entries += [plan] if kw.keys() & {"ns", "h"} or null in ("actor", "obs", "action") else []
    for entry in entries:
        with pytest.raises(lib.RLHipArgumentError):
            entry()


@pytest.mark.parametrize("name", list(R.CASES))
def test_both_precisions_of_the_model_take_the_same_decisions(name):
    c = R.build(name)
    e = R.clipped(c, G.draws(sample, 1, c["batch"], 1, SEED + 1, 0, STEP)[0, 0])
    rc, ra, fl, same = R.floors(c, R.records(c, c["idx"]), e)
    print(f"td3_mlp3 {name}: Float32 floors " + ", ".join(f"{k} {v:.2e}" for k, v in fl.items()))
    assert same, f"{name}: the Float32 and Float64 models decide differently (pick another seed)"
    if name == "base":
        assert rc["u_raw"].max() > c["hi"] and rc["u_raw"].min() < c["lo"] and 0 < R.records(c, c["idx"])[3].sum() < c["batch"]

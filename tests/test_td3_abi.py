"""The C boundary of the TD3 / DDPG entry points, with no device: header, ctypes table and library agree; every edge of the envelope is
-1 from rlhip_td3_workspace_bytes and RLHIP_EINVAL from the launching entries before any launch (the pointers handed over are never
followed)."""
import ctypes as C

import pytest

from test_iqn_abi import CTYPES, FAKE, _lib
from test_julia_glue_signatures import header_prototypes

ENTRIES = ("rlhip_td3_workspace_bytes", "rlhip_td3_plan_f32", "rlhip_td3_critic_grad_f32", "rlhip_td3_actor_grad_f32")
OK = dict(ns=3, h=64, nc=2, batch=64, layout=None, null=None)
EDGES = [dict(ns=1), dict(ns=5), dict(h=0), dict(h=24), dict(h=272), dict(nc=0), dict(nc=3), dict(batch=0)]


def test_header_ctypes_table_and_library_agree():
    lib, protos = _lib(), header_prototypes()
    assert lib.lib.rlhip_abi_version() == 2
    for name in ENTRIES:
        assert name in protos and name in lib.declared_symbols() and hasattr(lib.lib, name), f"{name} is not declared and exported"
        (ret, args), (res, argtypes) = protos[name], lib._PROTOS[name]
        argtypes = [C.c_void_p if issubclass(t, C._Pointer) else t for t in argtypes]  # (POINTER(Ring) is a pointer to the header)
        assert res is CTYPES[ret] and [CTYPES[a] for a in args] == argtypes, f"{name}: the ctypes table differs from the header"


def _entries(a):
    lib = _lib()
    ring = lib.Ring(capacity=8, n_env=4, obs_dim=a["ns"], len_rt=4, elem_bytes=4, layout=2 if a["layout"] is None else a["layout"], state=FAKE)
    ptrs = {k: (None if a["null"] == k else FAKE) for k in ("actor", "critics", "idx", "grad")}
    plan = lambda: lib.call("rlhip_td3_plan_f32", ptrs["actor"], a["ns"], a["h"], 0, FAKE, 8, 1.0, 0.1, -1.0, 1.0, 0, 1, 0, 0, FAKE, None, None)  # noqa: E731
    critic = lambda: lib.call("rlhip_td3_critic_grad_f32", C.byref(ring), a["h"], 0, a["nc"], ptrs["actor"], ptrs["critics"], FAKE,  # noqa: E731
                              a["batch"], ptrs["idx"], 0.99, 1.0, 0.2, 0.5, -1.0, 1.0, 1, 0, FAKE, ptrs["grad"], FAKE, None, None, None)
    actor = lambda: lib.call("rlhip_td3_actor_grad_f32", C.byref(ring), a["h"], 0, ptrs["actor"], ptrs["critics"], a["batch"], ptrs["idx"],  # noqa: E731
                             1.0, FAKE, ptrs["grad"], FAKE, None)
    return plan, critic, actor


@pytest.mark.parametrize("kw", EDGES + [dict(layout=0)] +  # (0: RLHIP_RING_FRAMES)
                          [dict(null=k) for k in ("actor", "critics", "idx", "grad")], ids=str)
def test_every_edge_of_the_envelope_is_refused_before_any_launch(kw):
    a, lib = dict(OK, **kw), _lib()
    ws = lib.lib.rlhip_td3_workspace_bytes
    assert ws(OK["ns"], OK["h"], OK["nc"], OK["batch"]) > 0
    if kw.keys() & {"ns", "h", "nc", "batch"}:
        assert ws(a["ns"], a["h"], a["nc"], a["batch"]) == -1
    plan, critic, actor = _entries(a)
    entries = [critic] + ([actor] if "nc" not in kw else []) + ([plan] if kw.keys() & {"ns", "h"} or kw.get("null") == "actor" else [])
    for entry in entries:
        with pytest.raises(lib.RLHipArgumentError):
            entry()

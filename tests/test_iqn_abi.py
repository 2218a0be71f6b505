"""The C boundary of the IQN entry points, with no device: the prototypes of include/rlhip.h, rlhip/_lib.py and the built library agree;
rlhip_iqn_workspace_bytes is -1 and forward, plan and the gradient entry return RLHIP_EINVAL at every edge of the envelope, before any
launch (the pointers handed over are never followed); rlhip_iqn_nparams is the sum of the six blocks; the fused loops refuse an
IQNLearner by name."""
import ctypes as C
import types

import pytest

from test_julia_glue_signatures import header_prototypes

ENTRIES = ("rlhip_iqn_nparams", "rlhip_iqn_init_f32", "rlhip_iqn_forward_f32", "rlhip_iqn_plan_f32", "rlhip_iqn_workspace_bytes",
           "rlhip_iqn_grad_batch_f32")
CTYPES = {"ptr": C.c_void_p, "Int32": C.c_int32, "Int64": C.c_int64, "UInt32": C.c_uint32, "UInt64": C.c_uint64, "Float32": C.c_float,
          "Float64": C.c_double}
FAKE = 0x1000  # a non-NULL address no check may follow
OK = dict(ns=4, h=64, na=2, nc=64, N=32, Np=32, kappa=1.0)
EDGES = [dict(h=16), dict(h=288), dict(h=48), dict(nc=3), dict(nc=66), dict(nc=0), dict(na=5), dict(na=0), dict(N=0), dict(N=65), dict(ns=1),
         dict(ns=17)]


def _lib():
    from rlhip import _lib

    return _lib


def test_header_ctypes_table_and_library_agree():
    lib, protos = _lib(), header_prototypes()
    assert lib.lib.rlhip_abi_version() == 2
    for name in ENTRIES:
        assert name in protos, f"{name} is not declared in include/rlhip.h"
        assert name in lib.declared_symbols() and hasattr(lib.lib, name), f"{name} is not exported"
        ret, args = protos[name]
        res, argtypes = lib._PROTOS[name]
        assert res is CTYPES[ret] and [CTYPES[a] for a in args] == list(argtypes), f"{name}: the ctypes table differs from the header"
    # exactly the arrays of the QR-DQN entry, plus n_cos, N' (N takes n_quantiles' place), seed, draw_ctr and the two level outputs
    assert len(protos["rlhip_iqn_grad_batch_f32"][1]) == len(protos["rlhip_qrdqn_grad_batch_f32"][1]) + 6


def test_nparams_is_the_sum_of_the_six_blocks():
    f = _lib().lib.rlhip_iqn_nparams
    for ns, h, na, nc in ((4, 128, 2, 64), (2, 32, 1, 2), (16, 256, 4, 64)):
        assert f(ns, h, na, nc) == h * ns + h + h * nc + h + na * h + na


def _forward(a):
    _lib().call("rlhip_iqn_forward_f32", FAKE, a["ns"], a["h"], a["na"], a["nc"], a["N"], 0, FAKE, 8, 1, 0, 0, FAKE, None, None, None)


def _plan(a):
    _lib().call("rlhip_iqn_plan_f32", FAKE, a["ns"], a["h"], a["na"], a["nc"], a["N"], 0, FAKE, 8, 0.1, 1, 0, 0, FAKE, None, None, None)


def _grad(a):
    _lib().call("rlhip_iqn_grad_batch_f32", a["ns"], a["h"], a["na"], a["nc"], a["N"], a["Np"], 0, a["kappa"], *([FAKE] * 7), 8, 0.99, None, None,
                0, 1, 0, FAKE, FAKE, FAKE, None, None, None, None, None, None)


@pytest.mark.parametrize("kw", EDGES + [dict(Np=0), dict(Np=65), dict(kappa=0.0), dict(kappa=float("inf"))], ids=str)
def test_every_edge_of_the_envelope_is_refused_before_any_launch(kw):
    a = dict(OK, **kw)
    ws = _lib().lib.rlhip_iqn_workspace_bytes
    assert ws(OK["ns"], OK["h"], OK["na"], OK["nc"], OK["N"], OK["Np"], 32) > 0
    if "kappa" not in kw:
        assert ws(a["ns"], a["h"], a["na"], a["nc"], a["N"], a["Np"], 32) == -1
    for entry in (_grad,) if ("kappa" in kw or "Np" in kw) else (_forward, _plan, _grad):
        with pytest.raises(_lib().RLHipArgumentError):
            entry(a)


def test_the_fused_loops_refuse_an_iqn_learner_by_name():
    from rlhip import core

    IQNLearner = type("IQNLearner", (), {"plan_distributional_": None})
    agent = types.SimpleNamespace(policy=types.SimpleNamespace(learner=IQNLearner()), trajectory=None)
    for loop in (core.run_fused_dqn, core.run_fused_dqn_folded, core.run_fused_dqn_prioritized):
        with pytest.raises(NotImplementedError, match="IQNLearner"):
            loop(agent, None)

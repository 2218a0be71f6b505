"""The C boundary of the QR-DQN entry points, with no device: the prototypes of include/rlhip.h, rlhip/_lib.py and the built library
agree; rlhip_qrdqn_workspace_bytes is -1 at every edge of the envelope; forward and plan refuse every edge with RLHIP_EINVAL before any
launch (the pointers handed over are never followed).  The refusals of rlhip_qrdqn_grad_batch_f32 are in tests/test_gpu_qrdqn_kernels.py."""
import ctypes as C

import pytest

import qrdqn_ref as R
from qrdqn_cases import TILE
from test_julia_glue_signatures import header_prototypes

ENTRIES = ("rlhip_qrdqn_forward_f32", "rlhip_qrdqn_plan_f32", "rlhip_qrdqn_workspace_bytes", "rlhip_qrdqn_grad_batch_f32")
CTYPES = {"ptr": C.c_void_p, "Int32": C.c_int32, "Int64": C.c_int64, "UInt32": C.c_uint32, "UInt64": C.c_uint64, "Float32": C.c_float,
          "Float64": C.c_double}
FAKE = 0x1000  # a non-NULL address no check may follow


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
        assert res is CTYPES[ret], name
        assert [CTYPES[a] for a in args] == list(argtypes), f"{name}: the ctypes table differs from the header"
    assert len(protos["rlhip_qrdqn_grad_batch_f32"][1]) == 25 and protos["rlhip_qrdqn_grad_batch_f32"][1][5] == "Float32"  # kappa
    # the C51 entries with kappa in place of (v_min, v_max); forward has one nullable array where C51 has two
    assert len(protos["rlhip_c51_grad_batch_f32"][1]) == 26 and len(protos["rlhip_qrdqn_plan_f32"][1]) == len(protos["rlhip_c51_plan_f32"][1]) - 2


BAD_SHAPES = ((1, 64, 2, 51, 32), (17, 64, 2, 51, 32), (4, 0, 2, 51, 32), (4, 6, 2, 51, 32), (4, 260, 2, 51, 32), (4, 64, 0, 51, 32),
              (4, 64, 5, 51, 32), (4, 64, 2, 0, 32), (4, 64, 2, 65, 32), (4, 64, 2, 51, 0), (4, 64, 2, 51, -1), (-4, 64, 2, 51, 32))


def test_workspace_bytes():
    f = _lib().lib.rlhip_qrdqn_workspace_bytes
    row = R.nparams(4, 64, 2 * 51) + 1
    assert f(4, 64, 2, 51, 1) == f(4, 64, 2, 51, TILE) == row * 4 and f(4, 64, 2, 51, TILE + 1) == 2 * row * 4
    assert f(4, 64, 2, 51, 256 * TILE) == f(4, 64, 2, 51, 1 << 20) == 256 * row * 4  # the cap on the partial rows ...
    big = R.nparams(16, 256, 256)
    assert (16 << 20) // (4 * big) == 59 and f(16, 256, 4, 64, 1 << 20) == 59 * (big + 1) * 4  # ... and on their bytes
    assert f(2, 4, 1, 1, 1) == (R.nparams(2, 4, 1) + 1) * 4 and f(16, 256, 4, 64, 1) > 0  # the corners of the envelope are inside
    for bad in BAD_SHAPES:
        assert f(*bad) == -1, bad


OK = dict(ns=4, h=64, na=2, N=51, act=0)
EDGES = [(dict(ns=1), "obs dim must be 2..16"), (dict(ns=17), "obs dim must be 2..16"), (dict(h=0), "multiple of 4"), (dict(h=6), "multiple of 4"),
         (dict(h=260), "multiple of 4"), (dict(na=0), "na must be 1..4"), (dict(na=5), "na must be 1..4"), (dict(N=0), "n_quantiles must be 1..64"),
         (dict(N=65), "n_quantiles must be 1..64"), (dict(act=2), "act must be"), (dict(act=-1), "act must be")]


def _forward(n=8, params=FAKE, obs=FAKE, q=FAKE, **kw):
    a = dict(OK, **kw)
    _lib().call("rlhip_qrdqn_forward_f32", params, a["ns"], a["h"], a["na"], a["N"], a["act"], obs, n, q, None, None)


def _plan(n=8, params=FAKE, obs=FAKE, actions=FAKE, **kw):
    a = dict(OK, **kw)
    _lib().call("rlhip_qrdqn_plan_f32", params, a["ns"], a["h"], a["na"], a["N"], a["act"], obs, n, 0.1, 1, 0, 0, actions, None, None)


@pytest.mark.parametrize("entry", [_forward, _plan])
@pytest.mark.parametrize("kw,message", EDGES)
def test_forward_and_plan_refuse_every_envelope_edge_before_any_launch(entry, kw, message):
    with pytest.raises(_lib().RLHipArgumentError, match=message):
        entry(**kw)


@pytest.mark.parametrize("entry,kw,message", [(_forward, dict(n=-1), "env count"), (_plan, dict(n=-1), "env count"),
                                              (_forward, dict(params=None), "NULL"), (_forward, dict(obs=None), "NULL"), (_forward, dict(q=None), "NULL"),
                                              (_plan, dict(params=None), "NULL"), (_plan, dict(obs=None), "NULL"), (_plan, dict(actions=None), "NULL")])
def test_argument_checks(entry, kw, message):
    with pytest.raises(_lib().RLHipArgumentError, match=message):
        entry(**kw)


def test_empty_env_sets_are_no_ops():
    _forward(n=0), _plan(n=0)  # nothing is launched, no pointer is followed

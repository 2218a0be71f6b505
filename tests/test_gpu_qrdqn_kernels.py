"""The QR-DQN kernels (csrc/qrdqn.hip) on the device, through the C ABI, on every case of tests/qrdqn_cases.py.

  forward       quantiles byte for byte the replay's where the hidden layer is ReLU (the header's chains are the replay's; tanhf is the
                device's own), otherwise inside 2 x the rows' budget; q inside 2 x its derived budget
  plan!         q_out byte for byte rlhip_qrdqn_forward_f32, actions byte for byte rlhip_eps_greedy_select_f32 on those values, for
                eps 0, 0.3 and 1 and an env_id_base that wraps
  gradient      sel equal, T and ql inside 2 x budget of the replay, the gradient within GRAD_BAR of max|g| of the float64 model, the
                loss inside its derived bar; two calls give the same bytes; every nullable output NULL in one call; guards behind every
                output keep their bytes
  bad action    contributes nothing (the bytes of the same batch with that sample's weight at zero), ql = 0; the bounds-checked
                build refuses the batch and takes the valid one
  refusals      every edge of the envelope, kappa among them, is RLHIP_EINVAL before any launch"""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import qrdqn_cases as CC
import qrdqn_ref as R
from conftest import ROOT, assert_grad_close
from heads_ref import F32
from test_gpu_bench_shapes import dev, host, note
from test_qrdqn_abi import EDGES, FAKE, OK
from test_qrdqn_reference import GRAD_BAR, loss_bar

pytestmark = pytest.mark.gpu
SENTINEL, GUARD = 7.0, 8


def buf(n, dtype=torch.float32):
    return torch.full((n + GUARD,), SENTINEL, dtype=dtype, device="cuda")


def guard_ok(t, n):
    return bool((t[n:] == SENTINEL).all())


def net_args(c, key="params"):
    return dev(c[key]), c["ns"], c["h"], c["na"], c["N"], c["act"]


def grad(c, want=True, a=None):
    """-> dict(grad, loss, ql, T, sel) of one rlhip_qrdqn_grad_batch_f32 call (`want = False`: every nullable output NULL)"""
    from rlhip import qrdqn

    B, N, np_ = c["batch"], c["N"], c["params"].size
    g, loss, ql, T, sel = buf(np_), buf(1), buf(B), buf(N * B), buf(B, torch.int32)
    qrdqn.qrdqn_grad_batch(c["ns"], c["h"], c["na"], N, c["act"], c["kappa"], dev(c["params"]), dev(c["target"]), dev(c["s"]),
                           dev(c["a"] if a is None else a), dev(c["r"]), dev(c["term"]), dev(c["sn"]), c["gamma"],
                           None if c.get("n_used") is None else dev(c["n_used"]), None if c.get("weights") is None else dev(c["weights"]),
                           c["double"], None, g, loss, ql if want else None, T if want else None, sel if want else None)
    torch.cuda.synchronize()
    for t, n in ((g, np_), (loss, 1), (ql, B), (T, N * B), (sel, B)):
        assert guard_ok(t, n), "a write behind an output array"
    if not want:
        assert all(bool((t == SENTINEL).all()) for t in (ql, T, sel)), "a NULL output was written"
    return dict(grad=host(g)[:np_], loss=float(host(loss)[0]), ql=host(ql)[:B], T=host(T)[:N * B].reshape(N, B), sel=host(sel)[:B])


@pytest.mark.parametrize("name", CC.NAMES)
def test_gradient_against_replay_and_model(name):
    c = CC.case(name)
    rp, m, b = c["replays"]
    got = grad(c)
    assert np.array_equal(got["sel"], rp["sel"]), f"{name}: a* differs at {np.flatnonzero(got['sel'] != rp['sel'])}"
    worst_t = R.within(got["T"], rp["T"], b["T"], f"{name} T")
    worst_q = R.within(got["ql"], rp["ql"], b["ql"], f"{name} ql")
    print(f"{name}: T at {worst_t:.3g} x its bar, ql at {worst_q:.3g} x; gradient {R.rel(got['grad'], m['grad']):.3e} of max|g|, "
          f"loss {got['loss']!r} vs {m['loss']!r} (bar {loss_bar(c, rp, b):.3g})")
    assert_grad_close(got["grad"], m["grad"], GRAD_BAR, f"qrdqn kernel {name}")
    assert abs(got["loss"] - m["loss"]) <= loss_bar(c, rp, b)
    assert (got["ql"][~rp["known"]] == 0).all()
    again = grad(c)
    assert all(np.array_equal(got[k], again[k]) for k in ("grad", "ql", "T", "sel")) and got["loss"] == again["loss"], "two calls differ"
    bare = grad(c, want=False)
    assert np.array_equal(bare["grad"], got["grad"]) and bare["loss"] == got["loss"], "the nullable outputs change the gradient"
    note("qrdqn gradient", case=name, rel=R.rel(got["grad"], m["grad"]), T=worst_t, ql=worst_q)


@pytest.mark.parametrize("name", ["bad-action", "bad-action-frames"])
def test_an_out_of_range_action_contributes_nothing_and_the_bounds_build_refuses_it(name):
    import rlhip as rl

    c = CC.case(name)
    rp = c["replays"][0]
    assert (~rp["known"]).sum() == 1
    got = grad(c)
    i = int(np.flatnonzero(~rp["known"])[0])
    # the same batch with that sample's weight at zero and a valid action: the same bytes
    c0 = dict(c, a=np.where(rp["known"], c["a"], 0).astype(np.int32),
              weights=np.where(rp["known"], c["weights"] if c.get("weights") is not None else F32(1), F32(0)).astype(F32))
    ref = grad(c0)
    assert np.array_equal(got["grad"], ref["grad"]) and got["loss"] == ref["loss"]
    assert got["ql"][i] == 0 and ref["ql"][i] != 0
    so = os.path.join(ROOT, "reinforcementlearning.jl_amd", "lib", "librlhip_bounds.so")
    assert os.path.exists(so), "run python -c 'import __graft_entry__ as g; g.build()'"
    lib = C.CDLL(so)
    f = lib.rlhip_qrdqn_grad_batch_f32
    f.restype, f.argtypes = C.c_int32, rl._lib._PROTOS["rlhip_qrdqn_grad_batch_f32"][1]
    lib.rlhip_last_error.restype = C.c_char_p
    P = lambda x: C.c_void_p(x.data_ptr())  # noqa: E731
    B = c["batch"]
    p, pt, s, r, t, sn = (dev(c[x]) for x in ("params", "target", "s", "r", "term", "sn"))
    ws = rl.qrdqn_workspace(c["ns"], c["h"], c["na"], c["N"], B)
    g, loss = torch.zeros_like(p), torch.zeros(1, device="cuda")
    for acts, rc in ((c["a"], -1), (c0["a"], 0)):
        ad = dev(acts)
        got_rc = f(c["ns"], c["h"], c["na"], c["N"], c["act"], c["kappa"], P(p), P(pt), P(s), P(ad), P(r), P(t), P(sn), B, c["gamma"], None, None,
                   0, P(ws), P(g), P(loss), None, None, None, None)
        torch.cuda.synchronize()
        assert got_rc == rc, lib.rlhip_last_error()
        if rc:
            assert f"1 of {B} actions".encode() in lib.rlhip_last_error()


_FORWARD = ("plain", "largest", "double-nused-weights", "ns2-h4-act0-na1-n1-", "ns4-h64-act1-na1-n64-", "ns5-h256-act1-na4-n51-", "ns16-h256-act0-na2-n2-",
            "ns4-h64-act0-na4-n64-")
FORWARD_CASES = [n for n in CC.NAMES if n.startswith(_FORWARD) and n != "plain-kappa-quarter"]
assert len(FORWARD_CASES) == len(_FORWARD)


@pytest.mark.parametrize("name", FORWARD_CASES)
def test_forward_and_plan(name):
    from rlhip import ops, qrdqn

    c = CC.case(name)
    na, N = c["na"], c["N"]
    obs = np.concatenate([c["s"], c["sn"]], 1)  # n = 2 batch: up to nine workgroups of 16 envs, the last one ragged
    n = obs.shape[1]
    q, th = buf(na * n), buf(na * N * n)
    qrdqn.qrdqn_forward(*net_args(c), dev(obs), q, th)
    torch.cuda.synchronize()
    assert guard_ok(q, na * n) and guard_ok(th, na * N * n)
    gq, gth = host(q)[:na * n].reshape(na, n), host(th)[:na * N * n].reshape(na * N, n)
    rq, rth = R.forward_replay(c, obs)
    e_l = R.net_error(c["params"], c["ns"], c["h"], na * N, c["act"], obs)
    if c["act"] == 0:
        assert np.array_equal(gth, rth), "ReLU quantiles are the replay's chains, byte for byte"
    else:
        R.within(gth, rth, e_l, f"{name} quantiles")
    wq = R.within(gq, rq, R.mean_budget(rth, e_l, na, N), f"{name} q")
    # only q_out asked for: the same bytes
    q2 = buf(na * n)
    qrdqn.qrdqn_forward(*net_args(c), dev(obs), q2)
    assert torch.equal(q2, q)
    # plan! = forward then select, byte for byte
    dobs, qd = dev(obs), q[:na * n].reshape(na, n).contiguous()
    for eps, base, step in ((0.0, 0, 3), (0.3, 17, 4), (1.0, 0, 5), (0.3, 0xFFFFFFF0, 6)):
        actions, qp = buf(n, torch.int32), buf(na * n)
        qrdqn.qrdqn_plan(*net_args(c), dobs, eps, 99, base, step, actions, qp)
        want = ops.eps_greedy_select(qd, eps, 99, step, base, None, False)
        torch.cuda.synchronize()
        assert guard_ok(actions, n) and guard_ok(qp, na * n)
        assert torch.equal(qp, q), "plan's q_out is not forward's"
        assert torch.equal(actions[:n], want.to(torch.int32)), f"eps {eps} base {base:#x}: actions differ from the two-call composition"
        if eps == 0.0:
            assert np.array_equal(host(actions)[:n], np.argmax(gq, 0))
    note("qrdqn forward", case=name, q=wq)


def _grad_call(batch=32, null=None, kappa=1.0, **kw):
    from rlhip import _lib

    a = dict(OK, **kw)
    p = {k: FAKE for k in ("params", "target", "s", "a", "r", "term", "sn", "ws", "grad", "loss")}
    if null:
        p[null] = None
    _lib.call("rlhip_qrdqn_grad_batch_f32", a["ns"], a["h"], a["na"], a["N"], a["act"], kappa, p["params"], p["target"], p["s"], p["a"], p["r"],
              p["term"], p["sn"], batch, 0.99, None, None, 0, p["ws"], p["grad"], p["loss"], None, None, None, None)


GRAD_EDGES = [(kw, msg) for kw, msg in EDGES] + [(dict(kappa=k), "kappa must be finite and > 0") for k in (0.0, -1.0, float("inf"), float("nan"))] + \
    [(dict(batch=0), "batch must be"), (dict(batch=-3), "batch must be")] + \
    [(dict(null=k), "NULL") for k in ("params", "target", "s", "a", "r", "term", "sn", "ws", "grad", "loss")]


@pytest.mark.parametrize("kw,message", GRAD_EDGES)
def test_the_gradient_entry_refuses_every_edge_before_any_launch(kw, message):
    """the addresses handed over are never followed: a launch on them would fault"""
    from rlhip import _lib

    with pytest.raises(_lib.RLHipArgumentError, match=message):
        _grad_call(**kw)

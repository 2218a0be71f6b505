"""The C51 kernels (csrc/c51.hip) on the device, through the C ABI, on every case of tests/c51_cases.py.

  forward       logits byte for byte the replay's where the hidden layer is ReLU (the header's chains are the replay's; tanhf is the
                device's own), q and probs inside 2 x their derived budget (tests/c51_ref.py: expf is not numpy's exp)
  plan!         q_out byte for byte rlhip_c51_forward_f32, actions byte for byte rlhip_eps_greedy_select_f32 on those values, for
                eps 0, 0.3 and 1 and an env_id_base that wraps
  gradient      sel equal, proj and ce inside 2 x budget of the replay, the gradient and the loss within GRAD_BAR of max|g| of the float64
                model; two calls give the same bytes; every nullable output NULL in one call; guards behind every output keep their bytes
  bad action    contributes nothing (the gradient of the batch without that sample, byte for byte where the order allows: judged at
                GRAD_BAR), ce = 0; the bounds-checked build refuses the batch and takes the valid one"""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import c51_cases as CC
import c51_ref as R
from conftest import ROOT, assert_grad_close
from heads_ref import F32
from test_c51_reference import GRAD_BAR
from test_gpu_bench_shapes import dev, host, note

pytestmark = pytest.mark.gpu
SENTINEL, GUARD = 7.0, 8


def buf(n, dtype=torch.float32):
    return torch.full((n + GUARD,), SENTINEL, dtype=dtype, device="cuda")


def guard_ok(t, n):
    return bool((t[n:] == SENTINEL).all())


def net_args(c, key="params"):
    return dev(c[key]), c["ns"], c["h"], c["na"], c["n_atoms"], c["act"], c["v_min"], c["v_max"]


def grad(c, want=True, a=None):
    """-> dict(grad, loss, ce, proj, sel) of one rlhip_c51_grad_batch_f32 call (`want = False`: every nullable output NULL)"""
    from rlhip import c51

    B, K, np_ = c["batch"], c["n_atoms"], c["params"].size
    g, loss, ce, proj, sel = buf(np_), buf(1), buf(B), buf(K * B), buf(B, torch.int32)
    c51.c51_grad_batch(c["ns"], c["h"], c["na"], K, c["act"], c["v_min"], c["v_max"], dev(c["params"]), dev(c["target"]), dev(c["s"]),
                       dev(c["a"] if a is None else a), dev(c["r"]), dev(c["term"]), dev(c["sn"]), c["gamma"],
                       None if c.get("n_used") is None else dev(c["n_used"]), None if c.get("weights") is None else dev(c["weights"]),
                       c["double"], None, g, loss, ce if want else None, proj if want else None, sel if want else None)
    torch.cuda.synchronize()
    for t, n in ((g, np_), (loss, 1), (ce, B), (proj, K * B), (sel, B)):
        assert guard_ok(t, n), "a write behind an output array"
    if not want:
        assert all(bool((t == SENTINEL).all()) for t in (ce, proj, sel)), "a NULL output was written"
    return dict(grad=host(g)[:np_], loss=float(host(loss)[0]), ce=host(ce)[:B], proj=host(proj)[:K * B].reshape(K, B), sel=host(sel)[:B])


@pytest.mark.parametrize("name", CC.NAMES)
def test_gradient_against_replay_and_model(name):
    c = CC.case(name)
    rp, m, b = c["replays"]
    got = grad(c)
    assert np.array_equal(got["sel"], rp["sel"]), f"{name}: a* differs at {np.flatnonzero(got['sel'] != rp['sel'])}"
    worst_p = R.within(got["proj"], rp["proj"], b["proj"], f"{name} proj")
    worst_c = R.within(got["ce"], rp["ce"], b["ce"], f"{name} ce")
    print(f"{name}: proj at {worst_p:.3g} x its bar, ce at {worst_c:.3g} x; gradient {R.rel(got['grad'], m['grad']):.3e} of max|g|, "
          f"loss {got['loss']!r} vs {m['loss']!r}")
    assert_grad_close(got["grad"], m["grad"], GRAD_BAR, f"c51 kernel {name}")
    assert abs(got["loss"] - m["loss"]) <= 1e-6 * max(1.0, abs(m["loss"]))
    assert (got["ce"][~rp["known"]] == 0).all()
    again = grad(c)
    assert all(np.array_equal(got[k], again[k]) for k in ("grad", "ce", "proj", "sel")) and got["loss"] == again["loss"], "two calls differ"
    bare = grad(c, want=False)
    assert np.array_equal(bare["grad"], got["grad"]) and bare["loss"] == got["loss"], "the nullable outputs change the gradient"
    note("c51 gradient", case=name, rel=R.rel(got["grad"], m["grad"]), proj=worst_p, ce=worst_c)


@pytest.mark.parametrize("name", ["bad-action", "bad-action-frames"])
def test_an_out_of_range_action_contributes_nothing_and_the_bounds_build_refuses_it(name):
    import rlhip as rl

    c = CC.case(name)
    rp = c["replays"][0]
    assert (~rp["known"]).sum() == 1
    got = grad(c)
    i = int(np.flatnonzero(~rp["known"])[0])
    # the same batch with that sample's weight at zero and a valid action: the same gradient up to the sign of a zero
    c0 = dict(c, a=np.where(rp["known"], c["a"], 0).astype(np.int32),
              weights=np.where(rp["known"], c["weights"] if c.get("weights") is not None else F32(1), F32(0)).astype(F32))
    ref = grad(c0)
    assert np.array_equal(got["grad"], ref["grad"]) and got["loss"] == ref["loss"]
    assert got["ce"][i] == 0 and ref["ce"][i] != 0
    so = os.path.join(ROOT, "reinforcementlearning.jl_amd", "lib", "librlhip_bounds.so")
    assert os.path.exists(so), "run python -c 'import __graft_entry__ as g; g.build()'"
    lib = C.CDLL(so)
    f = lib.rlhip_c51_grad_batch_f32
    f.restype, f.argtypes = C.c_int32, rl._lib._PROTOS["rlhip_c51_grad_batch_f32"][1]
    lib.rlhip_last_error.restype = C.c_char_p
    P = lambda x: C.c_void_p(x.data_ptr())  # noqa: E731
    B = c["batch"]
    p, pt, s, r, t, sn = (dev(c[x]) for x in ("params", "target", "s", "r", "term", "sn"))
    ws = rl.c51_workspace(c["ns"], c["h"], c["na"], c["n_atoms"], B)
    g, loss = torch.zeros_like(p), torch.zeros(1, device="cuda")
    for acts, rc in ((c["a"], -1), (c0["a"], 0)):
        ad = dev(acts)
        got_rc = f(c["ns"], c["h"], c["na"], c["n_atoms"], c["act"], c["v_min"], c["v_max"], P(p), P(pt), P(s), P(ad), P(r), P(t), P(sn), B,
                   c["gamma"], None, None, 0, P(ws), P(g), P(loss), None, None, None, None)
        torch.cuda.synchronize()
        assert got_rc == rc, lib.rlhip_last_error()
        if rc:
            assert f"1 of {B} actions".encode() in lib.rlhip_last_error()


_FORWARD = ("plain", "largest", "double-nused-weights", "ns2-h4-act0-na1-k2-", "ns5-h64-act1-na1-k64-", "ns16-h256-act1-na4-k64-", "ns4-h256-act1-na4-k3-")
FORWARD_CASES = [n for n in CC.NAMES if n.startswith(_FORWARD)]
assert len(FORWARD_CASES) == len(_FORWARD)


@pytest.mark.parametrize("name", FORWARD_CASES)
def test_forward_and_plan(name):
    from rlhip import c51, ops

    c = CC.case(name)
    na, K = c["na"], c["n_atoms"]
    obs = np.concatenate([c["s"], c["sn"]], 1)  # n = 2 batch: up to nine workgroups of 16 envs, the last one ragged
    n = obs.shape[1]
    q, probs, logits = buf(na * n), buf(na * K * n), buf(na * K * n)
    c51.c51_forward(*net_args(c), dev(obs), q, probs, logits)
    torch.cuda.synchronize()
    assert guard_ok(q, na * n) and guard_ok(probs, na * K * n) and guard_ok(logits, na * K * n)
    gq, gp, gl = host(q)[:na * n].reshape(na, n), host(probs)[:na * K * n].reshape(na * K, n), host(logits)[:na * K * n].reshape(na * K, n)
    rq, rpb, rl_ = R.forward_replay(c, obs)
    e_l = R.net_error(c["params"], c["ns"], c["h"], na * K, c["act"], obs)
    if c["act"] == 0:
        assert np.array_equal(gl, rl_), "ReLU logits are the replay's chains, byte for byte"
    else:
        R.within(gl, rl_, e_l, f"{name} logits")
    b_p, b_q = R.softmax_budget(rl_, e_l, na, K, R.support(c)[1])
    wp = R.within(gp, rpb, b_p.reshape(na * K, n), f"{name} probs")
    wq = R.within(gq, rq, b_q, f"{name} q")
    # only q_out asked for: the same bytes
    q2 = buf(na * n)
    c51.c51_forward(*net_args(c), dev(obs), q2)
    assert torch.equal(q2, q)
    # plan! = forward then select, byte for byte
    dobs, qd = dev(obs), q[:na * n].reshape(na, n).contiguous()
    for eps, base, step in ((0.0, 0, 3), (0.3, 17, 4), (1.0, 0, 5), (0.3, 0xFFFFFFF0, 6)):
        actions, qp = buf(n, torch.int32), buf(na * n)
        c51.c51_plan(*net_args(c), dobs, eps, 99, base, step, actions, qp)
        want = ops.eps_greedy_select(qd, eps, 99, step, base, None, False)
        torch.cuda.synchronize()
        assert guard_ok(actions, n) and guard_ok(qp, na * n)
        assert torch.equal(qp, q), "plan's q_out is not forward's"
        assert torch.equal(actions[:n], want.to(torch.int32)), f"eps {eps} base {base:#x}: actions differ from the two-call composition"
        if eps == 0.0:
            assert np.array_equal(host(actions)[:n], np.argmax(gq, 0))
    note("c51 forward", case=name, probs=wp, q=wq)

"""The SAC kernels (csrc/sac.hip) on the device against the replay of tests/sac_ref.py on the cases of tests/sac_cases.py.

  plan!         mu_out / rho_out byte for byte rlhip_mlp2_forward_f32; raw_sigma_out inside 2 x the softplus budget (heads_ref.Q: 3 ulp
                expf, 2 ulp log1pf, first-order propagation); action_out / action_scale and logp_out byte for byte
                rlhip_gaussian_head_sample_f32(soft = 1) fed with the launch's own mu_out and raw_sigma_out
  per sample    sel_out equal to the replay's; y_out and logp_out inside 2 x their budget (sac_ref.target_budget / head_budget)
  gradients,    F32_GRAD_TOL of the largest element (tests/conftest.py) against the replay, whose batch sums are Float64
  losses
  determinism   two calls, the same bytes;  sentinels: what a call is not asked to write keeps its bytes;  the alpha step in place
  bounds        the bounds-checked build refuses an index outside the ring (only that build is ever handed one)"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import sac_cases as SC
import sac_ref as R
from conftest import F32_GRAD_TOL, assert_grad_close
from heads_ref import F32, Q
from test_gpu_heads_grad import HeadsDevice

pytestmark = pytest.mark.gpu
SENTINEL = 7.0
GUARD = 8


class SacDevice(HeadsDevice):
    def traces(self, c):
        import rlhip

        tr = rlhip.CircularArraySARTSTraces(SC.CAP, SC.N_ENV, c["ns"], action_dtype=torch.float32)
        return SC.fill(c, tr, torch)

    @staticmethod
    def buf(n, dtype=torch.float32):
        return torch.full((n + GUARD,), SENTINEL, dtype=dtype, device="cuda")

    def critic(self, c, tr, want_y=True):
        from rlhip import sac

        dev = lambda x: torch.tensor(np.asarray(x, F32), device="cuda")  # noqa: E731
        grad, loss, y = self.buf(c["critics"].size), self.buf(2), self.buf(c["batch"])
        sac.sac_critic_grad(tr, c["h"], c["act"], dev(c["actor"]), dev(c["critics"]), dev(c["targets"]), torch.tensor(c["idx"], device="cuda"),
                            dev([c["alpha"]]), c["gamma"], c["lo"], c["hi"], c["scale"], c["stream_seed"] + 1, c["step"], None, grad, loss,
                            y if want_y else None)
        return grad.cpu().numpy(), loss.cpu().numpy(), y.cpu().numpy()

    def actor(self, c, tr, alpha_lr=None, alias=False, want=True, alpha_out=True):
        from rlhip import sac

        dev = lambda x: torch.tensor(np.asarray(x, F32), device="cuda")  # noqa: E731
        grad, stats, logp = self.buf(c["actor"].size), self.buf(3), self.buf(c["batch"])
        sel = self.buf(c["batch"], torch.int32)
        alpha = dev([c["alpha"]])
        out = alpha if alias else self.buf(1)
        sac.sac_actor_grad(tr, c["h"], c["act"], dev(c["actor"]), dev(c["critics"]), torch.tensor(c["idx"], device="cuda"), alpha, c["lo"],
                           c["hi"], c["scale"], c["stream_seed"] + 1, c["step"], c["alpha_lr"] if alpha_lr is None else alpha_lr,
                           c["target_entropy"], out if alpha_out else None, None, grad, stats, sel if want else None, logp if want else None)
        return grad.cpu().numpy(), stats.cpu().numpy(), sel.cpu().numpy(), logp.cpu().numpy(), alpha.cpu().numpy(), out.cpu().numpy()


@pytest.fixture(scope="module")
def dev():
    import rlhip  # noqa: F401
    return SacDevice()


def guard_ok(a, n):
    return (a[n:] == SENTINEL).all()


# ------------------------------------------------------------------------------------------------------------------- plan!
@pytest.mark.parametrize("ns,h,act,scale,lo,hi", [(2, 4, 0, 1.0, 0.0, np.inf), (3, 20, 1, 2.0, 0.0, np.inf), (4, 64, 0, 2.0, 0.6, 0.75),
                                                  (3, 256, 1, 1.0, 0.0, np.inf), (4, 256, 0, 1.0, 0.65, np.inf), (2, 64, 1, 2.0, 0.0, 0.7)])
def test_plan_is_forward_then_head(dev, ns, h, act, scale, lo, hi):
    from rlhip import ops, sac

    n, seed, base, step = 301, 21, 1000, 9  # five workgroups of one wave, the last one ragged
    rng = np.random.default_rng(ns * 1000 + h)
    actor = torch.tensor(SC._net(rng, ns, h, 2), device="cuda")
    obs = torch.tensor(rng.normal(0, 1, (ns, n)).astype(F32), device="cuda")
    act_o, lp, mu, rho, raw = (dev.buf(n) for _ in range(5))
    sac.sac_plan(actor, ns, h, act, obs, lo, hi, scale, seed, base, step, action=act_o, logp=lp, mu=mu, rho=rho, raw_sigma=raw)
    fwd = ops.mlp2_forward(actor, ns, h, 2, act, obs)
    assert torch.equal(fwd[0], mu[:n]) and torch.equal(fwd[1], rho[:n]), "mu_out / rho_out are not rlhip_mlp2_forward_f32's bytes"
    worst = R.within(raw[:n].cpu().numpy(), R.softplus_q(Q(rho[:n].cpu().numpy())), "raw_sigma_out")
    a_ref, lp_ref = dev.empty(n, 1, 1), dev.empty(n, 1)
    dev.call("rlhip_gaussian_head_sample_f32", dev.ptr(mu), dev.ptr(raw), 1, n, 1, float(lo), float(hi), 1, 1, seed, base, step,
             dev.ptr(a_ref), dev.ptr(lp_ref), dev.sp())
    assert torch.equal(act_o[:n] / scale, a_ref.reshape(-1)), "action_out / action_scale is not the head's action"
    assert torch.equal(lp[:n].view(torch.int32), lp_ref.reshape(-1).view(torch.int32)), "logp_out is not the head's log-probability"
    rawh = raw[:n].cpu().numpy()
    print(f"plan ns={ns} h={h} act={act}: raw sigma worst {worst:.3g} x the bar; clamped low {int((rawh < lo).sum())}, high {int((rawh > hi).sum())}")
    for b in (act_o, lp, mu, rho, raw):
        assert guard_ok(b.cpu().numpy(), n)
    # nullable outputs, and the evaluation form: no draw, no log-probability
    act2, keep = dev.buf(n), dev.buf(n)
    sac.sac_plan(actor, ns, h, act, obs, lo, hi, scale, seed, base, step, action=act2)
    assert torch.equal(act2, act_o)
    det = dev.buf(n)
    sac.sac_plan(actor, ns, h, act, obs, lo, hi, scale, seed, base, step, deterministic=True, action=det, mu=keep)
    assert torch.equal(keep[:n], mu[:n])
    R.within((det[:n] / scale).cpu().numpy(), Q(mu[:n].cpu().numpy()).libm("tanh"), "deterministic action")
    from rlhip._lib import RLHipArgumentError

    with pytest.raises(RLHipArgumentError, match="logp_out must be NULL"):
        sac.sac_plan(actor, ns, h, act, obs, lo, hi, scale, seed, base, step, deterministic=True, action=det, logp=lp)
    before = det.clone()
    dev.call("rlhip_sac_plan_f32", dev.ptr(actor), ns, h, act, dev.ptr(obs), 0, lo, hi, scale, 0, seed, base, step, dev.ptr(det), None, None,
             None, None, dev.sp())  # n = 0: a no-op
    assert torch.equal(det, before)


# ------------------------------------------------------------------------------------------------------------- the gradients
@pytest.mark.parametrize("name", SC.NAMES)
def test_gradients_losses_and_per_sample_outputs(dev, name):
    c = SC.case(name, dev.sample)
    eps0, eps1, rc, ra = c["replays"]
    tr, B = dev.traces(c), c["batch"]
    # the Float32 views of what the ring stores (the actions are the pushed Float32 bits)
    s, a, r, t, sn = c["records"]()
    gs, ga, gr, gt, gsn = tr.gather(torch.tensor(c["idx"], device="cuda"))
    fm = (lambda x: x.cpu().numpy().T) if tr.frame_major else (lambda x: x.cpu().numpy())
    assert ga.dtype == torch.float32 and np.array_equal(ga.cpu().numpy(), a) and np.array_equal(fm(gs), s)
    assert np.array_equal(fm(gsn), sn) and np.array_equal(gt.cpu().numpy(), t) and np.array_equal(gr.cpu().numpy(), r)
    # ---- critic step
    grad, loss, y = dev.critic(c, tr)
    assert guard_ok(grad, c["critics"].size) and guard_ok(loss, 2) and guard_ok(y, B)
    yq, _ = R.target_budget(c, rc)
    wy = R.within(y[:B], yq, f"{name} y_out")
    assert_grad_close(grad[:c["critics"].size], rc["grad"], F32_GRAD_TOL, f"sac critic grad {name}")
    assert_grad_close(loss[:2], rc["loss"], F32_GRAD_TOL, f"sac critic loss {name}")
    grad2, loss2, y2 = dev.critic(c, tr)
    assert grad.tobytes() == grad2.tobytes() and loss.tobytes() == loss2.tobytes() and y.tobytes() == y2.tobytes(), "run to run"
    grad3, loss3, y3 = dev.critic(c, tr, want_y=False)
    assert grad.tobytes() == grad3.tobytes() and loss.tobytes() == loss3.tobytes() and (y3 == SENTINEL).all()
    # ---- actor step
    grad, stats, sel, logp, alpha, out = dev.actor(c, tr)
    na = c["actor"].size
    assert guard_ok(grad, na) and guard_ok(stats, 3) and guard_ok(sel, B) and guard_ok(logp, B) and guard_ok(out, 1)
    assert np.array_equal(sel[:B], ra["sel"]), f"{name}: sel_out differs at {int((sel[:B] != ra['sel']).sum())} samples"
    o, _, _ = R.forward(c["actor"], c["ns"], c["h"], 2, c["act"], s)
    e_o = R.net_error(c["actor"], c["ns"], c["h"], 2, c["act"], s)
    wl = R.within(logp[:B], R.head_budget(o[0], o[1], eps1, c["lo"], c["hi"], c["scale"], e_o[0], e_o[1])["logp"], f"{name} logp_out")
    assert_grad_close(grad[:na], ra["grad"], F32_GRAD_TOL, f"sac actor grad {name}")
    assert_grad_close(stats[:3], ra["stats"], F32_GRAD_TOL, f"sac actor stats {name}")
    print(f"{name}: y_out worst {wy:.3g} x bar, logp_out worst {wl:.3g} x bar")
    # the alpha step: from the launch's own mean log-probability, bit for bit; in place; not at all
    want = F32(F32(c["alpha"]) - F32(c["alpha_lr"]) * (F32(-stats[2]) - F32(c["target_entropy"])))
    assert alpha[0] == F32(c["alpha"]) and out[0] == want, (out[0], want)
    assert abs(float(out[0]) - float(ra["alpha_new"])) <= 1e-6 * max(1.0, abs(float(ra["alpha_new"])))
    g2, st2, sel2, lp2, alpha2, out2 = dev.actor(c, tr, alias=True)
    assert alpha2[0] == want and out2[0] == want
    assert grad.tobytes() == g2.tobytes() and stats.tobytes() == st2.tobytes() and sel.tobytes() == sel2.tobytes() and logp.tobytes() == lp2.tobytes()
    g3, st3, sel3, lp3, alpha3, out3 = dev.actor(c, tr, alpha_lr=0.0, want=False)
    assert out3[0] == SENTINEL and alpha3[0] == F32(c["alpha"]) and (sel3 == int(SENTINEL)).all() and (lp3 == SENTINEL).all()
    assert grad.tobytes() == g3.tobytes() and stats.tobytes() == st3.tobytes()
    g4, st4, _, _, alpha4, _ = dev.actor(c, tr, alias=True, alpha_out=False)
    assert alpha4[0] == F32(c["alpha"]) and grad.tobytes() == g4.tobytes()


def test_bounds_checked_build_refuses_a_bad_index():
    """lib/librlhip_bounds.so validates idx before either gradient launch; the default build is never handed a bad index"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    so = os.path.join(root, "reinforcementlearning.jl_amd", "lib", "librlhip_bounds.so")
    assert os.path.exists(so), "run python -c 'import __graft_entry__ as g; g.build()'"
    prog = r"""
import sys, numpy as np, torch
sys.path[:0] = [sys.argv[1], sys.argv[1] + "/reinforcementlearning.jl_amd", sys.argv[1] + "/tests"]
import rlhip
from rlhip import sac
from rlhip._lib import RLHipArgumentError, lib
assert lib.rlhip_ring_bounds_checked_build() == 1
tr = rlhip.CircularArraySARTSTraces(8, 4, 3, action_dtype=torch.float32)
z = lambda *s: torch.zeros(*s, device="cuda")
tr.push_state_(z(3, 4))
for _ in range(5):
    tr.push_transition_(z(3, 4), z(4), z(4), z(4).to(torch.uint8))
h = 8
actor, critics, alpha = z(3 * h + h + 2 * h + 2), z(2 * (4 * h + h + h + 1)), z(1)
good = torch.arange(16, device="cuda")
sac.sac_critic_grad(tr, h, 0, actor, critics, critics.clone(), good, alpha, 0.99, 0.0, float("inf"), 1.0, 1, 0)
sac.sac_actor_grad(tr, h, 0, actor, critics, good, alpha, 0.0, float("inf"), 1.0, 1, 0)
torch.cuda.synchronize()
bad = good.clone()
bad[7] = 5 * 4  # one past the newest stored transition
for f, args in ((sac.sac_critic_grad, (tr, h, 0, actor, critics, critics.clone(), bad, alpha, 0.99, 0.0, float("inf"), 1.0, 1, 0)),
                (sac.sac_actor_grad, (tr, h, 0, actor, critics, bad, alpha, 0.0, float("inf"), 1.0, 1, 0))):
    try:
        f(*args)
        print("refused: no")
    except RLHipArgumentError as e:
        print("refused:", "outside" in str(e) and "position 7" in str(e))
"""
    r = subprocess.run([sys.executable, "-c", prog, root], capture_output=True, text=True, timeout=300, env=dict(os.environ, RLHIP_LIB_PATH=so))
    assert r.returncode == 0, r.stdout + r.stderr
    assert [ln for ln in r.stdout.splitlines() if ln.startswith("refused")] == ["refused: True"] * 2, r.stdout

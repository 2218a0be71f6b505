"""The judges of the SAC kernels judged themselves, on the CPU, and the refusals of the new entry points that need no device.

  * every case of tests/sac_cases.py passes its census with no sample excluded and holds its planted rows;
  * the Float32 replay (a) of tests/sac_ref.py against the float64 autograd model (b) on every case: gradients and losses at the bar
    the device is held to (F32_GRAD_TOL of max|g|, tests/conftest.py), per-sample outputs inside 2 x their derived budget;
  * misreadings of the header's text planted in (b): each one moves a gradient, a loss or the entropy coefficient past that bar;
  * RLHIP_EINVAL before any launch: the pointers handed over are never followed;
  * the Python refusals of rlhip/sac.py and the Float32 view of the traces' action word, on CPU tensors."""
import ctypes as C
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

import oracle
import sac_cases as SC
import sac_ref as R
from conftest import F32_GRAD_TOL, assert_grad_close
from heads_ref import F32, SQUASH_SOFT

FAKE = 0x1000  # a non-NULL address no check may follow


def sample(mu, raw, K, lo, hi, family, seed, base, step):
    sq, soft = SQUASH_SOFT[family]
    return oracle.gaussian_head_sample(mu, raw, K, lo, hi, sq, soft, seed=seed, env_id_base=base, step=step)


def rel(a, b):
    a, b = np.asarray(a, np.float64).ravel(), np.asarray(b, np.float64).ravel()
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


def test_every_case_passes_its_census_with_nothing_excluded():
    seen = dict(sel2=0, sel_t2=0, sel1=0, sel_t1=0)
    for name in SC.NAMES:
        c = SC.case(name, sample)
        assert c["excluded"] == 0
        n_bad, holds, _ = SC.census(c, sample)
        assert n_bad == 0, name
        for k in SC.PLANTED.get(name, ()):
            assert holds[k] > 0, (name, k, holds)
        assert c["batch"] == 1 or holds["terminal"] > 0, name
        seen["sel2"] += holds["sel2"]
        seen["sel1"] += c["batch"] - holds["sel2"]
        seen["sel_t2"] += holds["sel_t2"]
        seen["sel_t1"] += c["batch"] - holds["sel_t2"]
        print(name, "tries", c["tries"], holds)
    assert min(seen.values()) > 100, seen  # both critics win often, in both steps
    assert {SC.SPEC[n]["alpha"] for n in SC.NAMES if "alpha" in SC.SPEC[n]} == {0.0} and SC.SPEC["scale2"]["scale"] == 2.0
    assert SC.PUSHES > SC.CAP  # every ring has wrapped


@pytest.mark.parametrize("name", SC.NAMES)
def test_replay_against_float64_autograd(name):
    c = SC.case(name, sample)
    eps0, eps1, rc, ra = c["replays"]
    m = R.torch_model(c, eps0, eps1, ra, rc)
    assert_grad_close(rc["grad"], m["critic_grad"], F32_GRAD_TOL, f"sac replay critic {name}")
    assert_grad_close(ra["grad"], m["actor_grad"], F32_GRAD_TOL, f"sac replay actor {name}")
    assert rel(rc["loss"], m["critic_loss"]) <= 1e-6 and rel(ra["stats"], m["actor_stats"]) <= 1e-6
    assert abs(float(ra["alpha_new"]) - m["alpha_new"]) <= 1e-7 * max(1.0, abs(m["alpha_new"]))
    y, hb = R.target_budget(c, rc)
    R.within(m["y"], y, f"{name} y")
    s = c["records"]()[0]
    o, _, _ = R.forward(c["actor"], c["ns"], c["h"], 2, c["act"], s)
    e_o = R.net_error(c["actor"], c["ns"], c["h"], 2, c["act"], s)
    R.within(m["logp"], R.head_budget(o[0], o[1], eps1, c["lo"], c["hi"], c["scale"], e_o[0], e_o[1])["logp"], f"{name} logp")
    # the planted rows do what they are planted for
    hd = ra["head"]
    assert np.isfinite(ra["grad"]).all() and np.isfinite(rc["grad"]).all()
    assert (ra["drho"][~hd["ok"]] == 0).all() and not np.signbit(ra["drho"][~hd["ok"]]).any()  # drho is +0 at a clamped sigma


def _variant(name, **kw):
    c = dict(SC.case(name, sample))
    c.update(kw)
    return c


@pytest.mark.parametrize("fault,name,what", [("max", "ns3-h64-act0-b64", "critic_grad"), ("no_cont", "ns3-h64-act0-b64", "critic_grad"),
                                             ("no_alpha_target", "ns3-h64-act0-b64", "critic_grad"),
                                             ("no_alpha_actor", "ns3-h64-act0-b64", "actor_grad"), ("no_scale_dact", "scale2", "actor_grad"),
                                             ("no_tanh_correction", "ns3-h64-act0-b64", "actor_grad"),
                                             ("y_differentiated", "ns3-h64-act0-b64", "critic_grad")])
def test_a_planted_misreading_is_caught(fault, name, what):
    assert fault in R.FAULTS
    c = SC.case(name, sample)
    if fault == "y_differentiated":  # targets equal to the critics: only the differentiation of y differs, every value is the same
        c = _variant(name, targets=c["critics"].copy())
        eps0, eps1 = c["replays"][:2]
        rc, ra = R.critic_replay(c, eps0), R.actor_replay(c, eps1)
    else:
        eps0, eps1, rc, ra = c["replays"]
    good, bad = R.torch_model(c, eps0, eps1, ra, rc), R.torch_model(c, eps0, eps1, ra, rc, fault=fault)
    ref = rc["grad"] if what == "critic_grad" else ra["grad"]
    assert rel(good[what], ref) <= F32_GRAD_TOL
    assert rel(bad[what], ref) > 100 * F32_GRAD_TOL, f"{fault}: moves {what} by {rel(bad[what], ref):.3e} of max|g| only"


def test_the_old_critics_and_the_wrong_draw_index_are_caught():
    c = SC.case("ns3-h64-act0-b64", sample)
    eps0, eps1, rc, ra = c["replays"]
    stepped = (c["critics"] - F32(3e-3) * np.sign(rc["grad"]).astype(F32)).astype(F32)  # one Adam step from zero moments moves lr sign(g)
    new = R.actor_replay(c, eps1, critics=stepped)
    assert rel(new["grad"], ra["grad"]) > 100 * F32_GRAD_TOL        # the actor step on the old critics
    wrong = R.actor_replay(c, eps0)
    assert rel(wrong["grad"], ra["grad"]) > 100 * F32_GRAD_TOL      # draw index 0 where 1 is due
    assert not np.array_equal(eps0, eps1)


# ------------------------------------------------------------------------------------------------ the C boundary, no device
def _lib():
    from rlhip import _lib

    return _lib


def _ring(layout=2, obs_dim=3, len_rt=8):
    rb = _lib().Ring()
    rb.capacity, rb.n_env, rb.obs_dim, rb.len_rt, rb.len_sa, rb.elem_bytes, rb.layout, rb.state = 24, 8, obs_dim, len_rt, len_rt + 1, 4, layout, FAKE
    return rb


def _critic(h=64, act=0, batch=32, null=None, **ring):
    p = {k: FAKE for k in ("actor", "critics", "targets", "idx", "alpha", "ws", "grad", "loss")}
    if null:
        p[null] = None
    rb = None if null == "rb" else C.byref(_ring(**ring))
    _lib().call("rlhip_sac_critic_grad_f32", rb, h, act, p["actor"], p["critics"], p["targets"], batch, p["idx"], p["alpha"], 0.99, 0.0,
                float("inf"), 1.0, 1, 0, p["ws"], p["grad"], p["loss"], None, None)


def _actor(h=64, act=0, batch=32, null=None, **ring):
    p = {k: FAKE for k in ("actor", "critics", "idx", "alpha", "ws", "grad", "stats")}
    if null:
        p[null] = None
    rb = None if null == "rb" else C.byref(_ring(**ring))
    _lib().call("rlhip_sac_actor_grad_f32", rb, h, act, p["actor"], p["critics"], batch, p["idx"], p["alpha"], 0.0, float("inf"), 1.0, 1, 0,
                3e-3, -1.0, None, p["ws"], p["grad"], p["stats"], None, None, None)


SHAPE_REFUSALS = [(dict(h=6), "multiple of 4"), (dict(h=260), "multiple of 4"), (dict(h=0), "multiple of 4"), (dict(act=2), "act must be"),
                  (dict(batch=0), "empty batch"), (dict(obs_dim=5), "obs_dim must be 2..4"), (dict(obs_dim=1), "obs_dim must be 2..4"),
                  (dict(layout=0), "frame rings"), (dict(len_rt=0), "empty trajectory")]


@pytest.mark.parametrize("kw,message", SHAPE_REFUSALS + [(dict(null=k), "NULL argument") for k in
                                                          ("rb", "actor", "critics", "targets", "idx", "alpha", "ws", "grad", "loss")])
def test_critic_grad_refuses_before_any_launch(kw, message):
    with pytest.raises(_lib().RLHipArgumentError, match=message):
        _critic(**kw)


@pytest.mark.parametrize("kw,message", SHAPE_REFUSALS + [(dict(null=k), "NULL argument") for k in
                                                          ("rb", "actor", "critics", "idx", "alpha", "ws", "grad", "stats")])
def test_actor_grad_refuses_before_any_launch(kw, message):
    with pytest.raises(_lib().RLHipArgumentError, match=message):
        _actor(**kw)


def _plan(ns=3, h=64, act=0, n=8, actor=FAKE, obs=FAKE, action=FAKE, deterministic=0, logp=None):
    _lib().call("rlhip_sac_plan_f32", actor, ns, h, act, obs, n, 0.0, float("inf"), 1.0, deterministic, 1, 0, 1, action, logp, None, None,
                None, None)


@pytest.mark.parametrize("kw,message", [(dict(ns=5), "obs dim must be 2..4"), (dict(ns=1), "obs dim must be 2..4"), (dict(h=6), "multiple of 4"),
                                        (dict(h=260), "multiple of 4"), (dict(act=3), "act must be"), (dict(n=-1), "negative env count"),
                                        (dict(actor=None), "NULL argument"), (dict(obs=None), "NULL argument"),
                                        (dict(action=None), "NULL argument"), (dict(deterministic=1, logp=FAKE), "logp_out must be NULL")])
def test_plan_refuses_before_any_launch(kw, message):
    with pytest.raises(_lib().RLHipArgumentError, match=message):
        _plan(**kw)


def test_plan_takes_an_empty_env_set_and_the_library_exports_the_entries():
    _plan(n=0)  # a no-op: nothing is launched, no pointer is followed
    lib = _lib()
    for name in ("rlhip_sac_plan_f32", "rlhip_sac_critic_grad_f32", "rlhip_sac_actor_grad_f32", "rlhip_sac_workspace_bytes"):
        assert hasattr(lib.lib, name) and name in lib.declared_symbols()
    assert lib.lib.rlhip_abi_version() == 2


def test_workspace_bytes():
    f = _lib().lib.rlhip_sac_workspace_bytes
    row = max(R.nparams(3, 64, 2), 2 * R.nparams(4, 64, 1)) + 4
    assert f(3, 64, 1) == f(3, 64, 64) == row * 4 and f(3, 64, 65) == 2 * row * 4
    assert f(3, 64, 64 * 256) == f(3, 64, 1 << 20) == 256 * row * 4
    for bad in ((1, 64, 32), (5, 64, 32), (3, 6, 32), (3, 260, 32), (3, 0, 32), (3, 64, 0)):
        assert f(*bad) == -1, bad


# ------------------------------------------------------------------------------------------------ Python, on CPU tensors
def test_traces_hand_the_action_word_back_as_float32():
    import rlhip as rl

    with pytest.raises(TypeError, match="action eltype"):
        rl.CircularArraySARTSTraces(4, 2, 3, device="cpu", action_dtype=torch.float64)
    def stub(action_dtype):  # the views and the push check need no device: the storage of a record ring, without its C struct
        tr = rl.CircularArraySARTSTraces.__new__(rl.CircularArraySARTSTraces)
        tr.__dict__.update(records_layout=True, records=torch.zeros(5, 2, 16), obs_dim=3, action_dtype=action_dtype)
        return tr

    tr = stub(torch.float32)
    assert tr.action.dtype == torch.float32 and tr.action.shape == (5, 2)
    tr.records.view(torch.int32)[1, 0, 4] = int(np.float32(-0.75).view(np.int32))
    assert float(tr.action[1, 0]) == -0.75
    assert stub(torch.int32).action.dtype == torch.int32  # the default is unchanged
    with pytest.raises(TypeError, match="Float32 actions"):
        tr.push_transition_(torch.zeros(3, 2), torch.zeros(2, dtype=torch.int32), torch.zeros(2), torch.zeros(2, dtype=torch.uint8))


def _env(continuous=True, is_f64=0, ns=3, lo=(-2.0,), hi=(2.0,)):
    return NS(continuous=continuous, is_f64=is_f64, device="cpu", n=4, env_id_base=0, action_space=lambda: NS(lo=list(lo), hi=list(hi), n=None),
              state=lambda: torch.zeros(ns, 4))


def test_the_policy_refuses_what_is_out_of_scope_by_name(monkeypatch):
    import rlhip as rl
    from rlhip import ops

    monkeypatch.setattr(ops, "mlp2_init", lambda ni, h, no, seed, net_id=0, device="cpu": torch.zeros(R.nparams(ni, h, no)))
    with pytest.raises(ValueError, match="continuous-action env"):
        rl.SACPolicy(_env(continuous=False))
    with pytest.raises(NotImplementedError, match="Float64 envs"):
        rl.SACPolicy(_env(is_f64=1))
    with pytest.raises(NotImplementedError, match="da > 1"):
        rl.SACPolicy(_env(lo=(-1.0, -1.0), hi=(1.0, 1.0)))
    with pytest.raises(NotImplementedError, match="obs_dim > 4"):
        rl.SACPolicy(_env(ns=6))
    with pytest.raises(NotImplementedError, match="three-layer and bf16"):
        rl.SACPolicy(_env(), hidden=512)
    pol = rl.SACPolicy(_env(), hidden=8, batchsize=4)
    assert pol.action_scale == 2.0 and pol.actor.numel() == R.nparams(3, 8, 2) and pol.critics.numel() == 2 * R.nparams(4, 8, 1)
    assert torch.equal(pol.targets, pol.critics) and pol.targets.data_ptr() != pol.critics.data_ptr()
    traj = lambda tr, sampler=NS(): NS(container=tr, sampler=sampler)  # noqa: E731
    ok = dict(records_layout=True, action_dtype=torch.float32, obs_dim=3)
    with pytest.raises(NotImplementedError, match="prioritized replay"):
        pol.optimise_(traj(NS(sample_prioritized=None, **ok)))
    with pytest.raises(NotImplementedError, match="frame-layout traces"):
        pol.optimise_(traj(NS(**dict(ok, records_layout=False))))
    with pytest.raises(TypeError, match="action_dtype = torch.float32"):
        pol.optimise_(traj(NS(**dict(ok, action_dtype=torch.int32))))
    with pytest.raises(ValueError, match="the networks take 3"):
        pol.optimise_(traj(NS(**dict(ok, obs_dim=2))))
    with pytest.raises(NotImplementedError, match="n-step replay"):
        pol.optimise_(traj(NS(**ok), sampler=NS(n=3)))
    assert pol.vec_steps == 0 and pol.n_updates == 0  # nothing moved
    agent = NS(policy=pol, trajectory=traj(NS(**ok)))
    for loop in ("run_fused_dqn", "run_fused_dqn_folded", "run_fused_dqn_prioritized"):
        with pytest.raises(NotImplementedError, match=r"fused vec-step for SACPolicy.*rlhip\.run"):
            getattr(rl, loop)(agent, _env(), None, None)

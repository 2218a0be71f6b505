"""Every instantiation of the two-layer Float32 learner kernels that the C ABI can reach, and one problem that reaches it.

Not a test module: tests/test_gpu_f32_learner_matrix.py runs one oracle comparison per row, and
tests/test_f32_learner_dispatch.py pins the host dispatch these rows were derived from (the LAUNCH_* macros and their
conditions in csrc/ppo_grad.hip, dqn.hip, ppo.hip, dqn_act.hip) so that a changed branch cannot leave a row stale.

Reachability is worked out from the host code, not from the template axes:
  * the env decides the observation dim NS (CartPole 4, Pendulum 3, MountainCar 2) and, for PPO, the head: make_desc
    (csrc/ppo_common.h) gives na = 1 (continuous), 2 (CartPole) or 3 (Pendulum, MountainCar), and nout_a = 2 * na
    (continuous: mu, log sigma) or na.  So nout_a is 2 or 3, and 3 only for a discrete Pendulum / MountainCar;
  * ppo_grad_kernel<NS, ACT, NO, NT>: NO = 3 iff nout_a > 2, NT = 2 iff the micro-batch has more than 256 tiles of 64
    samples (> 16 384 samples);
  * dqn_grad_kernel<NS, ACT, FUSE, UPL>: FUSE iff rlhip_dqn_update_f32 with <= DQN_FUSE_MAX_BLOCKS (32) tiles and at
    most 4096 parameters (every 2-layer net with h <= 256, NS <= 4, na <= 4 has at most 2308), UPL = 2 iff h <= 128;
  * plan / rollout / DQN plan: the wide kernels for h in {64, 128, 256} while n * 16 <= 2^22, the scalar kernels
    otherwise (any other hidden size, or n > 2^18);
  * dqn_act_kernel<P, H, L, ACT>: rlhip_dqn_act_supported admits h in {64, 128, 256} only.

Each row: kernel, inst (the instantiation as the source spells it), id (the test id), env, continuous, n_actions
(None: the env's default), hidden, act, n, T (PPO) or batch (DQN), n_microbatches (PPO gradient).
"""

ENVS = {"cartpole": 4, "pendulum": 3, "mountaincar": 2}  # env -> observation dim NS
ENV_OF_NS = {v: k for k, v in ENVS.items()}
ACT_NAME = {0: "relu", 1: "tanh"}
WIDE_L = {64: 4, 128: 8, 256: 16}  # hidden -> lanes per env of the wide kernels


def ppo_na(env, continuous):
    """make_desc: number of actions of the PPO policy head"""
    return 1 if continuous else (2 if env == "cartpole" else 3)


def ppo_nout(env, continuous):
    return 2 * ppo_na(env, continuous) if continuous else ppo_na(env, continuous)


def _row(kernel, inst, rid, env, continuous=False, n_actions=None, hidden=64, act=0, n=64, T=None, batch=None,
         n_microbatches=None, **extra):
    r = dict(kernel=kernel, inst=inst, id=rid, env=env, continuous=continuous, n_actions=n_actions, hidden=hidden, act=act,
             n=n, T=T, batch=batch, n_microbatches=n_microbatches)
    r.update(extra)
    return r


# --------------------------------------------------------------------------------------------------- ppo_grad_kernel
# (NS, NO) -> (env, continuous) that reaches it.  NS = 4 never has NO = 3: CartPole has 2 actions and (mu, log sigma) is 2.
PPO_GRAD_HEADS = {(4, 2): ("cartpole", False), (3, 2): ("pendulum", True), (3, 3): ("pendulum", False),
                  (2, 2): ("mountaincar", True), (2, 3): ("mountaincar", False)}
PPO_GRAD_UNREACHABLE = {"ppo_grad_kernel<4, ACT, 3, NT>": "CartPole: 2 actions (discrete) or (mu, log sigma) (continuous), "
                                                          "so nout_a = 2"}
# micro-batch shapes: NT = 1 up to 16 384 samples, NT = 2 beyond (num_tiles > 256)
_NT1_SHAPES = [dict(n=256, T=16, n_microbatches=4),   # 1024 samples, 16 tiles
               dict(n=100, T=7, n_microbatches=3)]    # ragged: 233 samples = 3 tiles + 41, one transition dropped
_NT2_SHAPES = [dict(n=2064, T=8, n_microbatches=1),   # 16 512 samples = 258 tiles: 129 workgroups of two teams
               dict(n=2056, T=8, n_microbatches=1)]   # ragged: 16 448 samples = 257 tiles, the last workgroup has one team idle
_HIDDEN = [256, 64, 128, 200, 96]                      # 200, 96: multiples of 8 but not powers of two


def _ppo_grad_rows():
    rows = []
    i = 0
    for (ns, no), (env, cont) in PPO_GRAD_HEADS.items():
        for act in (0, 1):
            for nt in (1, 2):
                shape = (_NT1_SHAPES if nt == 1 else _NT2_SHAPES)[i % 2]
                h = _HIDDEN[i % len(_HIDDEN)]
                i += 1
                rows.append(_row("ppo_grad_kernel", f"ppo_grad_kernel<{ns}, {act}, {no}, {nt}>",
                                 f"ppo_grad-ns{ns}-{ACT_NAME[act]}-no{no}-nt{nt}", env, cont, hidden=h, act=act, **shape))
    return rows


# ---------------------------------------------------------------------------------------------------- dqn_grad_kernel
# Every (NS, ACT, FUSE, UPL) is reachable; each (NS, ACT, UPL) row runs both legs: FUSE = false through rlhip_dqn_grad_f32,
# FUSE = true through rlhip_dqn_update_f32 (batch <= 2048).  The row lists both instantiations.
def _dqn_grad_rows():
    rows = []
    i = 0
    for ns in (4, 3, 2):
        for act in (0, 1):
            for upl in (2, 4):
                h = (64, 128, 100)[i % 3] if upl == 2 else (256, 200, 132)[i % 3]
                na = (2, 3, 4)[i % 3]
                batch = (700, 2048, 333)[i % 3]
                i += 1
                for fuse in ("false", "true"):
                    rows.append(_row("dqn_grad_kernel", f"dqn_grad_kernel<{ns}, {act}, {fuse}, {upl}>",
                                     f"dqn_grad-ns{ns}-{ACT_NAME[act]}-upl{upl}-fuse{fuse[0].upper()}", ENV_OF_NS[ns],
                                     n_actions=na, hidden=h, act=act, batch=batch, fuse=fuse == "true", upl=upl))
    return rows


# ------------------------------------------------------------------------------- plan_wide / plan_scalar (PPO plan!)
_SCALAR_HIDDEN = {4: 96, 3: 100, 2: 40}


def _ppo_plan_rows():
    rows = []
    i = 0
    for ns in (4, 3, 2):
        env = ENV_OF_NS[ns]
        for act in (0, 1):
            for h in (64, 128, 256):
                cont = bool(i % 2) if env != "cartpole" else False
                i += 1
                rows.append(_row("plan_wide_kernel", f"plan_wide_kernel<{ns}, {h}, {WIDE_L[h]}, {act}>",
                                 f"ppo_plan-ns{ns}-h{h}-{ACT_NAME[act]}", env, cont, hidden=h, act=act, n=2048 + 37))
            rows.append(_row("plan_scalar_kernel", f"plan_scalar_kernel<{ns}, {act}>", f"ppo_plan-ns{ns}-scalar-{ACT_NAME[act]}",
                             env, act == 1 and env != "cartpole", hidden=_SCALAR_HIDDEN[ns], act=act, n=1000))
    return rows


# ------------------------------------------------------------------------------- dqn_plan_wide / dqn_plan_scalar
def _dqn_plan_rows():
    rows = []
    i = 0
    for ns in (4, 3, 2):
        for act in (0, 1):
            for h in (64, 128, 256):
                i += 1
                rows.append(_row("dqn_plan_wide_kernel", f"dqn_plan_wide_kernel<{ns}, {h}, {WIDE_L[h]}, {act}>",
                                 f"dqn_plan-ns{ns}-h{h}-{ACT_NAME[act]}", ENV_OF_NS[ns], n_actions=(2, 3, 4)[i % 3], hidden=h,
                                 act=act, n=4096 + 5))
            rows.append(_row("dqn_plan_scalar_kernel", f"dqn_plan_scalar_kernel<{ns}, {act}>",
                             f"dqn_plan-ns{ns}-scalar-{ACT_NAME[act]}", ENV_OF_NS[ns], n_actions=(2, 3, 4)[(i + act) % 3],
                             hidden=_SCALAR_HIDDEN[ns], act=act, n=3000))
    return rows


# ---------------------------------------------------------------------- rollout_split_kernel / rollout_scalar_kernel
# LAUNCH_WIDE (csrc/ppo.hip), by (act, cont, na):
#   relu: (disc, 2) -> <0, 2, 2>   (cont, 1) -> <0, 2, 1>   (disc, 3) -> <0, MAXO, 3>   otherwise <0, MAXO, 0>
#   tanh: (disc, 2) -> <1, 2, 2>   (cont, 1) -> <1, 2, 1>   otherwise <1, MAXO, 0>
# na is 1 / 2 / 3 (make_desc), so the relu HEAD = 0 branch is unreachable, and tanh HEAD = 0 is what a discrete Pendulum or
# MountainCar reaches.  A discrete CartPole is na = 2, a discrete Pendulum / MountainCar na = 3.
ROLLOUT_HEADS = {  # (env, act, head) -> (continuous, NOA)
    ("cartpole", 0, 2): (False, "2"), ("cartpole", 0, 1): (True, "2"),
    ("cartpole", 1, 2): (False, "2"), ("cartpole", 1, 1): (True, "2"),
    ("pendulum", 0, 3): (False, "MAXO"), ("pendulum", 0, 1): (True, "2"),
    ("pendulum", 1, 0): (False, "MAXO"), ("pendulum", 1, 1): (True, "2"),
    ("mountaincar", 0, 3): (False, "MAXO"), ("mountaincar", 0, 1): (True, "2"),
    ("mountaincar", 1, 0): (False, "MAXO"), ("mountaincar", 1, 1): (True, "2"),
}
ROLLOUT_UNREACHABLE = {
    "rollout_split_kernel<P, H, L, 0, MAXO, 0>": "relu with a discrete head of na not in {2, 3}: make_desc gives na in {1, 2, 3}",
    "rollout_split_kernel<CartPole, H, L, ACT, MAXO, *>": "a discrete CartPole has 2 actions (head 2)",
    "rollout_split_kernel<Pendulum|MountainCar, H, L, ACT, 2, 2>": "their discrete policy heads have 3 actions",
    "discrete Pendulum with n_actions != 3": "refused by rlhip_ppo_rollout_f32 and PPOPolicy (the PPO head has 3 actions)",
}
_ENV_CLASS = {"cartpole": "CartPoleParams<float>", "pendulum": "PendulumParams<float>", "mountaincar": "MountainCarParams<float>"}


def _rollout_rows():
    rows = []
    i = 0
    for (env, act, head), (cont, noa) in ROLLOUT_HEADS.items():
        for h in (64, 128, 256):
            i += 1
            rows.append(_row("rollout_split_kernel", f"rollout_split_kernel<{_ENV_CLASS[env]}, {h}, {WIDE_L[h]}, {act}, {noa}, {head}>",
                             f"rollout-{env}-h{h}-{ACT_NAME[act]}-head{head}", env, cont, hidden=h, act=act,
                             n=(37, 130, 16, 300)[i % 4], T=(13, 17, 33)[i % 3]))
    scalar_cont = {("cartpole", 0): False, ("cartpole", 1): True, ("pendulum", 0): True, ("pendulum", 1): False,
                   ("mountaincar", 0): False, ("mountaincar", 1): True}
    for (env, act), cont in scalar_cont.items():
        rows.append(_row("rollout_scalar_kernel", f"rollout_scalar_kernel<{_ENV_CLASS[env]}, {act}>",
                         f"rollout-{env}-scalar-{ACT_NAME[act]}", env, cont, hidden=_SCALAR_HIDDEN[ENVS[env]], act=act, n=300,
                         T=17))
    return rows


# ------------------------------------------------------------------------------------------------------ dqn_act_kernel
def _dqn_act_rows():
    rows = []
    for env in ENVS:
        for h in (64, 128, 256):
            for act in (0, 1):
                rows.append(_row("dqn_act_kernel", f"dqn_act_kernel<{_ENV_CLASS[env]}, {h}, {WIDE_L[h]}, {act}>",
                                 f"dqn_act-{env}-h{h}-{ACT_NAME[act]}", env, n_actions=None, hidden=h, act=act, n=1000 + h))
    return rows


PPO_GRAD = _ppo_grad_rows()
DQN_GRAD = _dqn_grad_rows()
PPO_PLAN = _ppo_plan_rows()
DQN_PLAN = _dqn_plan_rows()
ROLLOUT = _rollout_rows()
DQN_ACT = _dqn_act_rows()
ROWS = PPO_GRAD + DQN_GRAD + PPO_PLAN + DQN_PLAN + ROLLOUT + DQN_ACT

# additional cases on instantiations already listed above: run-time branches off the default path, and the second way into
# a scalar kernel.  They are not rows of the table (each instantiation is listed once).
EXTRA = [
    _row("dqn_grad_kernel", "dqn_grad_kernel<3, 1, false, 2>", "dqn_grad_weighted-ns3-tanh", "pendulum", n_actions=3, hidden=96,
         act=1, batch=500, per_beta=0.4),
    _row("dqn_grad_kernel", "dqn_grad_kernel<2, 1, false, 4>", "dqn_grad_idx-ns2-tanh", "mountaincar", n_actions=3, hidden=160,
         act=1, batch=450),
    _row("dqn_plan_scalar_kernel", "dqn_plan_scalar_kernel<2, 1>", "dqn_plan_large_n-ns2-h128-tanh", "mountaincar", n_actions=3,
         hidden=128, act=1, n=(1 << 18) + 37),
]

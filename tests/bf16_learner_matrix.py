"""Every instantiation of the three-layer bf16 MFMA learner kernels that the C ABI can reach, and one problem that reaches it.

Not a test module: tests/test_gpu_bf16_learner_matrix.py runs one oracle comparison per row, and
tests/test_bf16_learner_dispatch.py pins the host dispatch these rows were derived from (the LAUNCH_* macros, their conditions
and thresholds in csrc/dqn3.hip, ppo3.hip and ppo3w.hip) so that a changed branch cannot leave a row stale.

Reachability is worked out from the host code, not from the template axes:
  * DQN: (ns, na) is (4, 2) CartPole, (2, 3) MountainCar or (3, 3) Pendulum (every other pair is refused); hidden is 128
    (dqn3.hip) or 256 (ppo3w.hip);
  * rlhip_dqn3_plan_f32, h = 128: mlp3_plan32_kernel<NS, NA, ACT, NoActTail> for n <= 2^15, mlp3_plan_kernel<NS, NA, ACT>
    beyond;
  * rlhip_dqn3_act_f32 (plan + act + push): mlp3_plan32_kernel<P::ODIM, NA, ACT, ActTail<P>>; rlhip_dqn3_act_supported
    admits h = 128, the env's own action count and n <= 2^15 only;
  * rlhip_dqn3_grad_f32 / _w_f32 / update_f32, h = 128: batch <= 8192 -> dqn3_grad32_kernel<NS, NA, ACT, 1>, 8192 < batch <
    65536 -> dqn3_grad_kernel<NS, NA, ACT> (one 128-row tile per workgroup), batch >= 65536 -> dqn3_grad32_kernel<NS, NA, ACT, 2>
    (persistent, D3_GRAD32_BLOCKS = 512 workgroups, many tiles each); batch <= D3_MAX_BLOCKS * TR = 131072;
  * rlhip_dqn3_update_f32 runs d3_apply_kernel after the gradient, unless its grid ((np + 255) / 256 = 69 workgroups at
    most) exceeds grid_barrier_capacity -- never on an MI355X (256 CUs), so the unfused tail is unreachable there;
  * PPO layers = 3: CartPole (discrete, 2 actions) and Pendulum (continuous) only (check3: nout_a == 2, kind 0 or 1);
    the rollout is ppo3_rollout32_kernel<P, 2, ACT> for n <= 2^15 envs, ppo3_rollout_kernel<P, 2, ACT> beyond;
  * the PPO gradient is ppo3_gradT_kernel<NS, 0, CONT> iff chained = act == 0 && !force128 (persistent: min(tiles,
    RLHIP_PPO3_WGS = 128) workgroups per net -- more than 128 tiles of 128 samples put several tiles on a workgroup), else
    ppo3_grad_kernel<NS, 2, ACT, CONT> (relu only through the rlhip_debug_ppo3_force128 hook);
  * hidden = 256 (ppo3w.hip): the rollout launches ppo3w_rollout_kernel<P, 2, ACT, false> and the value pass
    ppo3w_fwd_kernel<NS, 1, ACT, 0, 4>; the PPO gradient a gather (ppo3w_gather_kernel<NS, CONT>, or ppo3w_gather_rec_kernel<NS>
    on the record copy that rlhip_ppo_update_f32 builds with ppo3w_build_rec_kernel<NS, CONT>), ppo3w_fwd_kernel modes 0 / 1,
    ppo3w_bwd_kernel<NS, ACT, PAD> for each net and ppo3w_dw2_kernel<NS, ACT>; the DQN gradient dqn3w_gather_kernel<NS>,
    ppo3w_fwd_kernel<NS, NA, ACT, 0, 2 / 3>, ppo3w_bwd_kernel<NS, ACT, PAD>, ppo3w_dw2_kernel<NS, ACT>; the DQN plan
    dqn3w_plan_kernel<NS, NA, ACT>.  PAD is chosen per launch by w3_dzf_pad() (rlhip_debug_w3_dzf_pad forces it).

A launch sequence runs several instantiations; each row owns `inst` and the instantiations in `owns`, and each reachable
instantiation is owned by exactly one row.  The non-template kernels every sequence runs (packs, reductions, the PPO optimiser
tails) are not rows.  The decision-free ("tight") cases of each DQN gradient form are tests/test_gpu_bf16_tight.py.

Each row: kernel, inst (the instantiation as the source spells it, template arguments resolved), id (the test id), env, hidden,
act, n / T (PPO, plans) or batch (DQN), and the extra switches: force128, pad (LDS copy of the 256-wide backward kernel),
rec (record gather), after (the gradient kernel an update row follows).
"""

ENVS = {"cartpole": 4, "pendulum": 3, "mountaincar": 2}  # env -> observation dim NS
DQN_NA = {"cartpole": 2, "pendulum": 3, "mountaincar": 3}
ACT_NAME = {0: "relu", 1: "tanh"}
ENV_CLASS = {"cartpole": "CartPoleParams<float>", "pendulum": "PendulumParams<float>", "mountaincar": "MountainCarParams<float>"}
PPO_ENVS = {"cartpole": False, "pendulum": True}  # layers = 3: env -> continuous
D3_MAX_BATCH = 1024 * 128  # D3_MAX_BLOCKS * TR
DQN_SHAPES = [("cartpole", 0), ("cartpole", 1), ("mountaincar", 0), ("mountaincar", 1), ("pendulum", 0), ("pendulum", 1)]


def _row(kernel, inst, rid, env, hidden=128, act=0, owns=(), **extra):
    r = dict(kernel=kernel, inst=inst, id=rid, env=env, hidden=hidden, act=act, owns=tuple(owns))
    r.update(extra)
    return r


def _dqn_tag(env, act):
    return f"ns{ENVS[env]}-na{DQN_NA[env]}-{ACT_NAME[act]}"


# ------------------------------------------------------------------------------------------------------- dqn3.hip
# gradients: one batch per row, ragged where it can be; each form has a batch just past its lower threshold and the last
# form the largest batch one launch takes
_BATCH = {"grad32o1": [8192, 4097, 1000, 8191, 333, 6000],
          "grad128": [8193, 65535, 20001, 8193, 40000, 12345],
          "grad32o2": [65537, D3_MAX_BATCH, 65536, 98305, D3_MAX_BATCH, 65537]}


def _dqn3_grad_rows():
    rows = []
    for form, kern in (("grad32o1", "dqn3_grad32_kernel"), ("grad128", "dqn3_grad_kernel"), ("grad32o2", "dqn3_grad32_kernel")):
        for i, (env, act) in enumerate(DQN_SHAPES):
            ns, na = ENVS[env], DQN_NA[env]
            tail = {"grad32o1": ", 1", "grad128": "", "grad32o2": ", 2"}[form]
            rows.append(_row(kern, f"{kern}<{ns}, {na}, {act}{tail}>", f"dqn3_{form}-{_dqn_tag(env, act)}", env, act=act,
                             batch=_BATCH[form][i], isw=act == 1))
    return rows


def _dqn3_plan_rows():
    rows = []
    for i, (env, act) in enumerate(DQN_SHAPES):
        ns, na = ENVS[env], DQN_NA[env]
        rows.append(_row("mlp3_plan32_kernel", f"mlp3_plan32_kernel<{ns}, {na}, {act}, NoActTail>", f"dqn3_plan32-{_dqn_tag(env, act)}",
                         env, act=act, n=(1 << 15, 1000, 4097)[i % 3]))
        rows.append(_row("mlp3_plan_kernel", f"mlp3_plan_kernel<{ns}, {na}, {act}>", f"dqn3_plan128-{_dqn_tag(env, act)}", env,
                         act=act, n=(1 << 15) + 1, n2=(100003, 70001, 131201)[i % 3]))
    return rows


def _dqn3_act_rows():
    return [_row("mlp3_plan32_kernel", f"mlp3_plan32_kernel<{ENVS[env]}, {DQN_NA[env]}, {act}, ActTail<{ENV_CLASS[env]}>>",
                 f"dqn3_act-{env}-{ACT_NAME[act]}", env, act=act, n=(1000, 4096 + 37, 1 << 15)[i % 3])
            for i, (env, act) in enumerate(DQN_SHAPES)]


# the fused optimiser tail after each gradient form (the row's `after`): update == grad -> clip + Adam -> pack, bit for bit
DQN3_UPDATE = [
    _row("d3_apply_kernel", "d3_apply_kernel", "dqn3_update-grad32o1-ns2-na3-tanh", "mountaincar", act=1, batch=5000,
         after="dqn3_grad32_kernel<2, 3, 1, 1>"),
    _row("d3_apply_kernel", "d3_apply_kernel", "dqn3_update-grad128-ns3-na3-relu", "pendulum", act=0, batch=8193,
         after="dqn3_grad_kernel<3, 3, 0>"),
    _row("d3_apply_kernel", "d3_apply_kernel", "dqn3_update-grad32o2-ns4-na2-tanh", "cartpole", act=1, batch=65537,
         after="dqn3_grad32_kernel<4, 2, 1, 2>"),
]
DQN3_UNREACHABLE = {
    "d3_reduce_kernel -> rlhip_clip_adam_f32 -> rlhip_mlp3_pack_bf16 in rlhip_dqn3_update_f32":
        "runs only when (np + 255) / 256 > grid_barrier_capacity(d3_apply_kernel): np <= 17 410 is 69 workgroups, an MI355X "
        "holds 256 CUs x several workgroups",
    "mlp3_plan32_kernel<*, *, *, ActTail<*>> at h = 256 or n > 2^15": "rlhip_dqn3_act_supported refuses it (the per-step path runs)",
    "dqn3 gradient at batch > 131072": "refused: batch <= D3_MAX_BLOCKS * TR",
}


# ------------------------------------------------------------------------------------------------------- ppo3.hip
def _ppo3_rows():
    rows = []
    for env, cont in PPO_ENVS.items():
        P = ENV_CLASS[env]
        for act in (0, 1):
            rows.append(_row("ppo3_rollout32_kernel", f"ppo3_rollout32_kernel<{P}, 2, {act}>", f"ppo3_rollout32-{env}-{ACT_NAME[act]}",
                             env, act=act, n=200, T=6))
            rows.append(_row("ppo3_rollout_kernel", f"ppo3_rollout_kernel<{P}, 2, {act}>", f"ppo3_rollout128-{env}-{ACT_NAME[act]}",
                             env, act=act, n=(1 << 15) + 1, T=2))
        ns, c = ENVS[env], int(cont)
        # the chained tile with more tiles than persistent workgroups: > 128 tiles of 128 samples (ragged last tile)
        rows.append(_row("ppo3_gradT_kernel", f"ppo3_gradT_kernel<{ns}, 0, {c}>", f"ppo3_gradT-{env}-relu", env, act=0,
                         n=4100 if env == "cartpole" else 2051, T=4 if env == "cartpole" else 8, nmb=1, force128=False))
        rows.append(_row("ppo3_grad_kernel", f"ppo3_grad_kernel<{ns}, 2, 0, {c}>", f"ppo3_grad128-{env}-relu-force128", env, act=0,
                         n=96, T=9, nmb=2, force128=True))
        rows.append(_row("ppo3_grad_kernel", f"ppo3_grad_kernel<{ns}, 2, 1, {c}>", f"ppo3_grad128-{env}-tanh", env, act=1,
                         n=2050, T=9, nmb=1, force128=False))
    return rows


PPO3_UNREACHABLE = {
    "ppo3_gradT_kernel<NS, 1, CONT>": "chained = act == 0 && !force128: tanh never takes the chained tile",
    "MountainCar / a discrete Pendulum / a continuous CartPole at layers = 3": "check3 refuses nout_a != 2; ppo3_grad requires "
                                                                                 "CartPole discrete, Pendulum continuous",
}


# ------------------------------------------------------------------------------------------------------ ppo3w.hip
def _ppo3w_rows():
    rows = []
    for env, cont in PPO_ENVS.items():
        P, ns, c = ENV_CLASS[env], ENVS[env], int(cont)
        for act in (0, 1):
            a = ACT_NAME[act]
            rows.append(_row("ppo3w_rollout_kernel", f"ppo3w_rollout_kernel<{P}, 2, {act}, false>", f"ppo3w_rollout-{env}-{a}", env,
                             hidden=256, act=act, n=200, T=6, owns=[f"ppo3w_fwd_kernel<{ns}, 1, {act}, 0, 4>"]))
            for pad in (0, 1):
                owns = ([f"ppo3w_fwd_kernel<{ns}, 2, {act}, {c}, 0>", f"ppo3w_fwd_kernel<{ns}, 1, {act}, {c}, 1>"] if pad == 0
                        else [f"ppo3w_dw2_kernel<{ns}, {act}>"])
                if pad == 0 and act == 0:
                    owns.append(f"ppo3w_gather_kernel<{ns}, {c}>")
                shape = dict(n=96, T=9, nmb=2) if pad == 0 else dict(n=2048, T=9, nmb=1)  # 1 ragged tile / 288 tiles > 256 CUs
                rows.append(_row("ppo3w_bwd_kernel", f"ppo3w_bwd_kernel<{ns}, {act}, {'true' if pad else 'false'}>",
                                 f"ppo3w_grad-{env}-{a}-pad{pad}", env, hidden=256, act=act, pad=pad, owns=owns, **shape))
        rows.append(_row("ppo3w_gather_rec_kernel", f"ppo3w_gather_rec_kernel<{ns}>", f"ppo3w_update_rec-{env}-relu", env, hidden=256,
                         act=0, n=512, T=16, nmb=1, rec=True, owns=[f"ppo3w_build_rec_kernel<{ns}, {c}>"]))
    return rows


def _dqn3w_rows():
    rows = []
    for i, (env, act) in enumerate(DQN_SHAPES):
        ns, na = ENVS[env], DQN_NA[env]
        fwd = [f"ppo3w_fwd_kernel<{ns}, {na}, {act}, 0, 2>", f"ppo3w_fwd_kernel<{ns}, {na}, {act}, 0, 3>"]
        gather = [f"dqn3w_gather_kernel<{ns}>"] if act == 0 else []
        if ns == 2:  # MountainCar: the only DQN observation dim the PPO rows do not reach -- its backward kernels are owned here
            for pad in (0, 1):
                owns = fwd + gather if pad == 0 else [f"ppo3w_dw2_kernel<{ns}, {act}>"]
                rows.append(_row("ppo3w_bwd_kernel", f"ppo3w_bwd_kernel<{ns}, {act}, {'true' if pad else 'false'}>",
                                 f"dqn3w_grad-{_dqn_tag(env, act)}-pad{pad}", env, hidden=256, act=act, pad=pad, owns=owns,
                                 batch=(300, 20000)[pad]))
        else:
            rows.append(_row("ppo3w_fwd_kernel", fwd[0], f"dqn3w_grad-{_dqn_tag(env, act)}-pad{act}", env, hidden=256, act=act, pad=act,
                             owns=fwd[1:] + gather, batch=(20000, 777)[act]))
        rows.append(_row("dqn3w_plan_kernel", f"dqn3w_plan_kernel<{ns}, {na}, {act}>", f"dqn3w_plan-{_dqn_tag(env, act)}", env,
                         hidden=256, act=act, n=(70001, 1000, 33000)[i % 3]))
    return rows


DQN3_GRAD = _dqn3_grad_rows()
DQN3_PLAN = _dqn3_plan_rows()
DQN3_ACT = _dqn3_act_rows()
PPO3 = _ppo3_rows()
PPO3W = _ppo3w_rows()
DQN3W = _dqn3w_rows()
ROWS = DQN3_GRAD + DQN3_PLAN + DQN3_ACT + DQN3_UPDATE + PPO3 + PPO3W + DQN3W


def grad_form(inst):
    """the gradient form of a dqn3 gradient instantiation: the template with its (NS, NA, ACT) left open"""
    kern = inst.split("<")[0]
    return kern + ("<NS, NA, ACT, 2>" if inst.endswith(", 2>") else "<NS, NA, ACT, 1>" if inst.endswith(", 1>") and
                   kern == "dqn3_grad32_kernel" else "<NS, NA, ACT>")


def owned(row):
    """the instantiations a row owns (d3_apply_kernel once per gradient form it follows)"""
    first = row["inst"] + (f" after {grad_form(row['after'])}" if "after" in row else "")
    return (first,) + row["owns"]

"""The host dispatch of the two-layer Float32 learners decides which template instantiation a problem reaches;
tests/f32_learner_matrix.py lists every reachable one with a problem that reaches it, and tests/test_gpu_f32_learner_matrix.py
compares each with the oracle.  A changed LAUNCH_* line, branch condition or threshold would leave a row stale (testing some
other instantiation than it names) without any GPU test failing -- this test fails instead (CPU only: it reads the source).
It also models the dispatch in Python and checks that every row reaches the instantiation it names, that the table lists each
reachable instantiation exactly once, and that each row is a test id of the GPU file."""
import os
import re

import f32_learner_matrix as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "reinforcementlearning.jl_amd", "csrc")

# (file, exact text, count): every dispatch line the table depends on, exactly as often as the source has it today
PINNED = [
    # ppo_grad.hip: NO = 3 iff nout_a > 2, NT = 2 iff more than 256 tiles of TILE = 64 samples
    ("ppo_grad_tile.h", "constexpr int TILE = 64;", 1),
    ("ppo_grad.hip", "out->nt = g.num_tiles > 256 ? 2 : 1;", 1),
    ("ppo_grad.hip", "g.num_tiles = (int)((bm + TILE - 1) / TILE);", 1),
    ("ppo_grad.hip", "if (L.nt == 2) {", 1),
    ("ppo_grad.hip", "if (L.g.pd.nout_a > 2) LAUNCH_GK(NS_, ACT_, 3, 2);", 1),
    ("ppo_grad.hip", "else LAUNCH_GK(NS_, ACT_, 2, 2);", 1),
    ("ppo_grad.hip", "} else if (L.g.pd.nout_a > 2) LAUNCH_GK(NS_, ACT_, 3, 1);", 1),
    ("ppo_grad.hip", "else LAUNCH_GK(NS_, ACT_, 2, 1);", 1),
    ("ppo_grad.hip", "if (L.ns == 4) { if (a == 0) LAUNCH_G(4, 0); else LAUNCH_G(4, 1); }", 1),
    ("ppo_grad.hip", "else if (L.ns == 3) { if (a == 0) LAUNCH_G(3, 0); else LAUNCH_G(3, 1); }", 1),
    ("ppo_grad.hip", "else { if (a == 0) LAUNCH_G(2, 0); else LAUNCH_G(2, 1); }", 1),
    ("ppo_grad.hip", "int ns = kind == 0 ? 4 : (kind == 1 ? 3 : 2);", 2),
    ("ppo_common.h", "static inline int64_t env_na(int kind, int cont) { return cont ? 1 : (kind == 0 ? 2 : 3); }", 1),
    ("ppo_common.h", "pd->nout_a = pd->cont ? 2 * pd->na : pd->na;", 1),
    # dqn.hip: FUSE iff an apply tail and <= DQN_FUSE_MAX_BLOCKS tiles; UPL = 2 iff h <= 128; update fuses up to 4096 params
    ("dqn.hip", "constexpr int DQN_FUSE_MAX_BLOCKS = 32;", 1),
    ("dqn.hip", "constexpr int DTILE = 64;", 1),
    ("dqn.hip", "g.num_tiles = (int)((batch + DTILE - 1) / DTILE);", 1),
    ("dqn.hip", "const bool fuse = apply != nullptr && nb <= DQN_FUSE_MAX_BLOCKS && !RLHIP_ENV_FLAG(\"RLHIP_DQN_NO_FUSE\");", 1),
    ("dqn.hip", "if (h <= 128) hipLaunchKernelGGL((dqn_grad_kernel<NS_, ACT_, FUSE_, 2>)", 1),
    ("dqn.hip", "else hipLaunchKernelGGL((dqn_grad_kernel<NS_, ACT_, FUSE_, 4>)", 1),
    ("dqn.hip", "if (fuse) LAUNCH_DG4(NS_, ACT_, true);", 1),
    ("dqn.hip", "else LAUNCH_DG4(NS_, ACT_, false);", 1),
    ("dqn.hip", "if (ns == 4) { if (act == 0) LAUNCH_DG(4, 0); else LAUNCH_DG(4, 1); }", 1),
    ("dqn.hip", "else if (ns == 3) { if (act == 0) LAUNCH_DG(3, 0); else LAUNCH_DG(3, 1); }", 1),
    ("dqn.hip", "else { if (act == 0) LAUNCH_DG(2, 0); else LAUNCH_DG(2, 1); }", 1),
    ("dqn.hip", "if (np > 4096) {", 1),
    # the wide condition of the plan / rollout / DQN plan kernels, and their H -> L table
    ("ppo.hip", "bool wide = (pd.h == 256 || pd.h == 128 || pd.h == 64) && n * 16 <= (int64_t)1 << 22;", 2),
    ("dqn.hip", "bool wide = (h == 256 || h == 128 || h == 64) && n * 16 <= (int64_t)1 << 22;", 1),
    ("ppo.hip", "if (wide && pd.h == 256) LAUNCH_WIDE(256, 16);", 1),
    ("ppo.hip", "else if (wide && pd.h == 128) LAUNCH_WIDE(128, 8);", 1),
    ("ppo.hip", "else if (wide && pd.h == 64) LAUNCH_WIDE(64, 4);", 1),
    ("ppo.hip", "if (wide && pd.h == 256) LAUNCH_PW(256, 16);", 1),
    ("ppo.hip", "else if (wide && pd.h == 128) LAUNCH_PW(128, 8);", 1),
    ("ppo.hip", "else if (wide && pd.h == 64) LAUNCH_PW(64, 4);", 1),
    ("dqn.hip", "if (wide && h == 256) LAUNCH_QW(256, 16);", 1),
    ("dqn.hip", "else if (wide && h == 128) LAUNCH_QW(128, 8);", 1),
    ("dqn.hip", "else if (wide && h == 64) LAUNCH_QW(64, 4);", 1),
    ("ppo.hip", "hipLaunchKernelGGL((rollout_scalar_kernel<P, 0>)", 1),
    ("ppo.hip", "hipLaunchKernelGGL((rollout_scalar_kernel<P, 1>)", 1),
    ("ppo.hip", "hipLaunchKernelGGL((plan_scalar_kernel<NS, 0>)", 1),
    ("ppo.hip", "hipLaunchKernelGGL((plan_scalar_kernel<NS, 1>)", 1),
    ("ppo.hip", "hipLaunchKernelGGL((plan_wide_kernel<NS, H, L, 0>)", 1),
    ("ppo.hip", "hipLaunchKernelGGL((plan_wide_kernel<NS, H, L, 1>)", 1),
    ("dqn.hip", "hipLaunchKernelGGL((dqn_plan_scalar_kernel<NS, 0>)", 1),
    ("dqn.hip", "hipLaunchKernelGGL((dqn_plan_scalar_kernel<NS, 1>)", 1),
    ("dqn.hip", "hipLaunchKernelGGL((dqn_plan_wide_kernel<NS, H, L, 0>)", 1),
    ("dqn.hip", "hipLaunchKernelGGL((dqn_plan_wide_kernel<NS, H, L, 1>)", 1),
    # the head conditions of LAUNCH_WIDE (ppo.hip)
    ("ppo.hip", "if (pd.act == 0 && !pd.cont && pd.na == 2) LAUNCH_WIDE_AS(H, L, 0, 2, 2);", 1),
    ("ppo.hip", "else if (pd.act == 0 && pd.cont && pd.na == 1) LAUNCH_WIDE_AS(H, L, 0, 2, 1);", 1),
    ("ppo.hip", "else if (pd.act == 0 && !pd.cont && pd.na == 3) LAUNCH_WIDE_AS(H, L, 0, MAXO, 3);", 1),
    ("ppo.hip", "else if (pd.act == 0) LAUNCH_WIDE_AS(H, L, 0, MAXO, 0);", 1),
    ("ppo.hip", "else if (!pd.cont && pd.na == 2) LAUNCH_WIDE_AS(H, L, 1, 2, 2);", 1),
    ("ppo.hip", "else if (pd.cont && pd.na == 1) LAUNCH_WIDE_AS(H, L, 1, 2, 1);", 1),
    ("ppo.hip", "else LAUNCH_WIDE_AS(H, L, 1, MAXO, 0);", 1),
    ("ppo.hip", "if (kind == 0) return plan_impl<4>(", 1),
    ("ppo.hip", "if (kind == 1) return plan_impl<3>(", 1),
    ("ppo.hip", "return plan_impl<2>(", 1),
    ("dqn.hip", "if (ns == 4) return dqn_plan_impl<4>(", 1),
    ("dqn.hip", "if (ns == 3) return dqn_plan_impl<3>(", 1),
    ("dqn.hip", "return dqn_plan_impl<2>(", 1),
    # dqn_act.hip: h -> (H, L), the activation, and what rlhip_dqn_act_supported admits
    ("dqn_act.hip", "hipLaunchKernelGGL((dqn_act_kernel<P, H_, L_, 0>)", 1),
    ("dqn_act.hip", "hipLaunchKernelGGL((dqn_act_kernel<P, H_, L_, 1>)", 1),
    ("dqn_act.hip", "if (act == 0)", 1),
    ("dqn_act.hip", "if (h == 256) LAUNCH_A(256, 16);", 1),
    ("dqn_act.hip", "else if (h == 128) LAUNCH_A(128, 8);", 1),
    ("dqn_act.hip", "else LAUNCH_A(64, 4);", 1),
    ("dqn_act.hip", "(h == 256 || h == 128 || h == 64) && n >= 1 && n * 16 <= ((int64_t)1 << 22)", 1),
]

LAUNCH_MACRO_USES = {  # file -> number of LAUNCH_* invocations (a new branch adds one)
    "ppo_grad.hip": 10, "dqn.hip": 11, "ppo.hip": 13, "dqn_act.hip": 3,
}


def _src(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def test_dispatch_lines_match_the_instantiation_table():
    moved = [(f, s, n, _src(f).count(s)) for f, s, n in PINNED if _src(f).count(s) != n]
    assert not moved, ("a dispatch line of the two-layer Float32 learners changed -- update tests/f32_learner_matrix.py (and "
                       f"the GPU matrix) so that every instantiation is still reached, then this list: {moved}")
    # a new or removed LAUNCH_* call (outside the #define lines) is a changed instantiation set as well
    uses = {f: len(re.findall(r"(?<!define )\bLAUNCH_[A-Z0-9_]*\(", _src(f))) for f in LAUNCH_MACRO_USES}
    assert uses == LAUNCH_MACRO_USES, uses


# ------------------------------------------------------------------ the dispatch, restated from the pinned lines above
MAXO = "MAXO"
ENV_CLASS = {"cartpole": "CartPoleParams<float>", "pendulum": "PendulumParams<float>", "mountaincar": "MountainCarParams<float>"}


def ppo_grad_inst(env, cont, act, bm):
    ns, nout = M.ENVS[env], M.ppo_nout(env, cont)
    nt = 2 if (bm + 63) // 64 > 256 else 1
    return f"ppo_grad_kernel<{ns}, {act}, {3 if nout > 2 else 2}, {nt}>"


def dqn_grad_insts(ns, act, h, batch):
    upl = 2 if h <= 128 else 4
    fused = (batch + 63) // 64 <= 32
    return [f"dqn_grad_kernel<{ns}, {act}, false, {upl}>"] + ([f"dqn_grad_kernel<{ns}, {act}, true, {upl}>"] if fused else [])


def _wide(h, n):
    return h in (64, 128, 256) and n * 16 <= 1 << 22


def plan_inst(ns, h, act, n, dqn=False):
    pre = "dqn_plan" if dqn else "plan"
    return f"{pre}_wide_kernel<{ns}, {h}, {h // 16}, {act}>" if _wide(h, n) else f"{pre}_scalar_kernel<{ns}, {act}>"


def rollout_inst(env, cont, h, act, n):
    P = ENV_CLASS[env]
    if not _wide(h, n):
        return f"rollout_scalar_kernel<{P}, {act}>"
    na = M.ppo_na(env, cont)
    if act == 0:
        noa, head = ((2, 2) if (not cont and na == 2) else (2, 1) if (cont and na == 1) else (MAXO, 3) if (not cont and na == 3)
                     else (MAXO, 0))
    else:
        noa, head = (2, 2) if (not cont and na == 2) else (2, 1) if (cont and na == 1) else (MAXO, 0)
    return f"rollout_split_kernel<{P}, {h}, {h // 16}, {act}, {noa}, {head}>"


def dqn_act_inst(env, h, act):
    hh = h if h in (128, 256) else 64
    return f"dqn_act_kernel<{ENV_CLASS[env]}, {hh}, {hh // 16}, {act}>"


def test_every_row_reaches_the_instantiation_it_names():
    for r in M.PPO_GRAD:
        bm = r["n"] * r["T"] // r["n_microbatches"]
        assert ppo_grad_inst(r["env"], r["continuous"], r["act"], bm) == r["inst"], r["id"]
        assert r["hidden"] % 8 == 0 and r["hidden"] <= 256
    for r in M.DQN_GRAD:
        insts = dqn_grad_insts(M.ENVS[r["env"]], r["act"], r["hidden"], r["batch"])
        assert r["inst"] == insts[1 if r["fuse"] else 0], r["id"]
        assert oracle_free_nparams(M.ENVS[r["env"]], r["hidden"], r["n_actions"]) <= 4096
    for r in M.PPO_PLAN:
        assert plan_inst(M.ENVS[r["env"]], r["hidden"], r["act"], r["n"]) == r["inst"], r["id"]
    for r in M.DQN_PLAN:
        assert plan_inst(M.ENVS[r["env"]], r["hidden"], r["act"], r["n"], dqn=True) == r["inst"], r["id"]
    for r in M.ROLLOUT:
        assert rollout_inst(r["env"], r["continuous"], r["hidden"], r["act"], r["n"]) == r["inst"], r["id"]
    for r in M.DQN_ACT:
        assert r["hidden"] in (64, 128, 256) and dqn_act_inst(r["env"], r["hidden"], r["act"]) == r["inst"], r["id"]
    for r in M.EXTRA:
        ns = M.ENVS[r["env"]]
        got = (dqn_grad_insts(ns, r["act"], r["hidden"], r["batch"])[0] if r["kernel"] == "dqn_grad_kernel"
               else plan_inst(ns, r["hidden"], r["act"], r["n"], dqn=True))
        assert got == r["inst"], r["id"]


def oracle_free_nparams(ns, h, na):
    return h * ns + h + na * h + na


def test_the_table_lists_every_reachable_instantiation_exactly_once():
    reach = {"ppo_grad_kernel": set(), "dqn_grad_kernel": set(), "plan": set(), "dqn_plan": set(), "rollout": set(),
             "dqn_act_kernel": set()}
    heads = [(e, c) for e in M.ENVS for c in (False, True)]
    hiddens = (64, 96, 128, 200, 256)
    for env, cont in heads:
        for act in (0, 1):
            for bm in (1024, 16385):
                reach["ppo_grad_kernel"].add(ppo_grad_inst(env, cont, act, bm))
            for h in hiddens:
                for n in (1000, (1 << 18) + 1):
                    reach["plan"].add(plan_inst(M.ENVS[env], h, act, n))
                    reach["dqn_plan"].add(plan_inst(M.ENVS[env], h, act, n, dqn=True))
                    reach["rollout"].add(rollout_inst(env, cont, h, act, n))
                for batch in (64, 2048, 2049):
                    reach["dqn_grad_kernel"].update(dqn_grad_insts(M.ENVS[env], act, h, batch))
            for h in (64, 128, 256):
                reach["dqn_act_kernel"].add(dqn_act_inst(env, h, act))
    every = set().union(*reach.values())
    listed = [r["inst"] for r in M.ROWS]
    assert len(listed) == len(set(listed)), "an instantiation is listed twice"
    assert set(listed) == every, (sorted(every - set(listed)), sorted(set(listed) - every))
    assert len(reach["ppo_grad_kernel"]) == 20 and len(reach["dqn_grad_kernel"]) == 24
    assert len(reach["rollout"]) == 42 and len(reach["dqn_act_kernel"]) == 18
    assert not any(", 0, MAXO, 0>" in i for i in listed), "the relu HEAD = 0 branch is not reachable (na is 1, 2 or 3)"
    assert len({r["id"] for r in M.ROWS + M.EXTRA}) == len(M.ROWS) + len(M.EXTRA)


def test_every_row_is_a_test_id_of_the_gpu_matrix():
    import test_gpu_f32_learner_matrix as G

    seen = []
    for name in dir(G):
        fn = getattr(G, name)
        if not name.startswith("test_") or not callable(fn):
            continue
        for mark in getattr(fn, "pytestmark", []):
            if mark.name == "parametrize":
                seen += list(mark.kwargs["ids"])
    ids = [r["id"] for r in M.ROWS]
    assert sorted(i for i in seen if i in ids) == sorted(ids), sorted(set(ids) - set(seen))
    assert all(r["id"] in seen for r in M.EXTRA)

"""The host dispatch of the three-layer bf16 MFMA learners decides which template instantiation a problem reaches;
tests/bf16_learner_matrix.py lists every reachable one with a problem that reaches it, and tests/test_gpu_bf16_learner_matrix.py
compares each with the oracle.  A changed LAUNCH_* line, branch condition or threshold would leave a row stale (testing some
other instantiation than it names) without any GPU test failing -- this test fails instead (CPU only: it reads the source).
It also models the dispatch in Python and checks that every row reaches the instantiation it names, that the table lists each
reachable instantiation exactly once, and that each row is a test id of the GPU file."""
import os
import re

import bf16_learner_matrix as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "reinforcementlearning.jl_amd", "csrc")

# (file, exact text, count): every dispatch line the table depends on, exactly as often as the source has it today
PINNED = [
    # tile sizes and limits
    ("mlp3_device.h", "constexpr int TR = 128;", 1),
    ("dqn3.hip", "constexpr int D3_MAX_BLOCKS = 1024;", 1),
    ("dqn3.hip", "constexpr int P32 = 32;", 1),
    ("dqn3.hip", "constexpr int G32 = 32;", 1),
    ("dqn3.hip", "constexpr int D3_GRAD32_BLOCKS = 512;", 1),
    ("ppo3.hip", "constexpr int R32 = 32;", 1),
    # dqn3.hip: width, (ns, na), plan / act / gradient dispatch
    ("dqn3.hip", "RLHIP_REQUIRE(h == H3 || h == HWIDE, \"the MFMA Q-network path is built for hidden = 128 or 256\");", 3),
    ("dqn3.hip", "RLHIP_REQUIRE((ns == 4 && na == 2) || (ns == 2 && na == 3) || (ns == 3 && na == 3),", 1),
    ("dqn3.hip", "RLHIP_REQUIRE((rb->obs_dim == 4 && na == 2) || (rb->obs_dim == 2 && na == 3) || (rb->obs_dim == 3 && na == 3),", 1),
    ("dqn3.hip", "if (h == HWIDE) return dqn3w_plan(", 1),
    ("dqn3.hip", "if (h == HWIDE) {", 1),
    ("dqn3.hip", "const bool small = n <= (1 << 15);", 1),
    ("dqn3.hip", "hipLaunchKernelGGL((mlp3_plan32_kernel<NS_, NA_, ACT_, NoActTail>), grid32,", 1),
    ("dqn3.hip", "hipLaunchKernelGGL((mlp3_plan_kernel<NS_, NA_, ACT_>), grid,", 1),
    ("dqn3.hip", "if (ns == 4 && na == 2) { if (act == 0) LAUNCH_P(4, 2, 0); else LAUNCH_P(4, 2, 1); }", 1),
    ("dqn3.hip", "else if (ns == 2 && na == 3) { if (act == 0) LAUNCH_P(2, 3, 0); else LAUNCH_P(2, 3, 1); }", 1),
    ("dqn3.hip", "else { if (act == 0) LAUNCH_P(3, 3, 0); else LAUNCH_P(3, 3, 1); }", 1),
    ("dqn3.hip", "return (kind >= 0 && kind <= 2 && h == H3 && na == want && n >= 1 && n <= (1 << 15)) ? 1 : 0;", 1),
    ("dqn3.hip", "const int64_t want = kind == 0 ? 2 : 3;", 1),
    ("dqn3.hip", "hipLaunchKernelGGL((mlp3_plan32_kernel<P::ODIM, NA, 0, ActTail<P>>), grid32,", 1),
    ("dqn3.hip", "hipLaunchKernelGGL((mlp3_plan32_kernel<P::ODIM, NA, 1, ActTail<P>>), grid32,", 1),
    ("dqn3.hip", "return dqn3_act_impl<CartPoleParams<float>, 2>(", 1),
    ("dqn3.hip", "return dqn3_act_impl<PendulumParams<float>, 3>(", 1),
    ("dqn3.hip", "return dqn3_act_impl<MountainCarParams<float>, 3>(", 1),
    ("dqn3.hip", "RLHIP_REQUIRE(batch <= (int64_t)D3_MAX_BLOCKS * TR, \"batch too large for one launch\");", 1),
    ("dqn3.hip", "const bool small = batch <= 8192 || batch >= 65536;", 1),
    ("dqn3.hip", "if (batch >= 65536) {", 1),
    ("dqn3.hip", "hipLaunchKernelGGL((dqn3_grad32_kernel<NS_, NA_, ACT_, 2>), dim3(nb),", 1),
    ("dqn3.hip", "hipLaunchKernelGGL((dqn3_grad32_kernel<NS_, NA_, ACT_, 1>), dim3(nb),", 1),
    ("dqn3.hip", "hipLaunchKernelGGL((dqn3_grad_kernel<NS_, NA_, ACT_>), dim3(nb),", 1),
    ("dqn3.hip", "const int nb = small ? (int)(tiles32 < D3_GRAD32_BLOCKS ? tiles32 : D3_GRAD32_BLOCKS) : (int)((batch + TR - 1) / TR);", 1),
    ("dqn3.hip", "if (ns == 4 && na == 2) { if (act == 0) LAUNCH_G(4, 2, 0); else LAUNCH_G(4, 2, 1); }", 1),
    ("dqn3.hip", "else if (ns == 2 && na == 3) { if (act == 0) LAUNCH_G(2, 3, 0); else LAUNCH_G(2, 3, 1); }", 1),
    ("dqn3.hip", "else { if (act == 0) LAUNCH_G(3, 3, 0); else LAUNCH_G(3, 3, 1); }", 1),
    ("dqn3.hip", "if ((np + 255) / 256 <= cap) {", 1),
    # ppo3.hip: which envs, the rollout split, chained vs the 128-row tile, the persistent workgroup cap
    ("ppo3.hip", "RLHIP_REQUIRE(pd->nout_a == 2, \"layers = 3 supports CartPole (discrete, 2 actions) and Pendulum (continuous)\");", 1),
    ("ppo3.hip", "RLHIP_REQUIRE(kind == 0 || kind == 1, \"layers = 3 supports CartPole and Pendulum\");", 3),
    ("ppo3.hip", "if (cfg->hidden == HWIDE)", 3),
    ("ppo3.hip", "const bool small = n <= (1 << 15);", 1),
    ("ppo3.hip", "hipLaunchKernelGGL((ppo3_rollout32_kernel<P, 2, ACT_>), grid,", 1),
    ("ppo3.hip", "hipLaunchKernelGGL((ppo3_rollout_kernel<P, 2, ACT_>), grid,", 1),
    ("ppo3.hip", "if (pd.act == 0) LAUNCH_R3(0);", 1),
    ("ppo3.hip", "else LAUNCH_R3(1);", 1),
    ("ppo3.hip", "const bool chained = pd.act == 0 && !g_ppo3_force128;", 1),
    ("ppo3.hip", "t3_wg_cap = e ? atoi(e) : 128;", 1),
    ("ppo3.hip", "const int nwg = ntiles < t3_wg_cap ? ntiles : t3_wg_cap;", 1),
    ("ppo3.hip", "const int64_t nb = (bm + TR - 1) / TR;", 1),
    ("ppo3.hip", "hipLaunchKernelGGL((ppo3_gradT_kernel<NS_, 0, CONT_>), dim3(2 * nwg),", 1),
    ("ppo3.hip", "hipLaunchKernelGGL((ppo3_grad_kernel<NS_, 2, ACT_, CONT_>), dim3((int)nb),", 1),
    ("ppo3.hip", "if (chained) LAUNCH_G3T(4, 0);", 1),
    ("ppo3.hip", "else if (pd.act == 0) LAUNCH_G3(4, 0, 0);", 1),
    ("ppo3.hip", "else LAUNCH_G3(4, 1, 0);", 1),
    ("ppo3.hip", "if (chained) LAUNCH_G3T(3, 1);", 1),
    ("ppo3.hip", "else if (pd.act == 0) LAUNCH_G3(3, 0, 1);", 1),
    ("ppo3.hip", "else LAUNCH_G3(3, 1, 1);", 1),
    # ppo3w.hip: rollout, PPO gradient (gather / gather_rec), DQN gradient and plan at hidden = 256, the backward LDS copy
    ("ppo3w.hip", "hipLaunchKernelGGL((ppo3w_rollout_kernel<P, 2, ACT_, false>), grid,", 1),
    ("ppo3w.hip", "hipLaunchKernelGGL((ppo3w_fwd_kernel<NS, 1, ACT_, 0, 4>), dim3(nwg),", 1),
    ("ppo3w.hip", "if (pd.act == 0) LAUNCH_RW(0);", 1),
    ("ppo3w.hip", "else LAUNCH_RW(1);", 1),
    ("ppo3w.hip", "g.rec = (tail != nullptr && tail->rec_ready) ? (const float*)(ws + L.off_rec) : nullptr;", 1),
    ("ppo3w.hip", "const P3WTail tail{params, m, v, beta_pow, true};", 1),
    ("ppo3w.hip", "if (g.rec != nullptr) {", 1),
    ("ppo3w.hip", "if (kind == 0) hipLaunchKernelGGL((ppo3w_gather_rec_kernel<4>), dim3(gb),", 1),
    ("ppo3w.hip", "else hipLaunchKernelGGL((ppo3w_gather_rec_kernel<3>), dim3(gb),", 1),
    ("ppo3w.hip", "if (kind == 0) hipLaunchKernelGGL((ppo3w_gather_kernel<4, 0>), dim3(gb),", 1),
    ("ppo3w.hip", "else hipLaunchKernelGGL((ppo3w_gather_kernel<3, 1>), dim3(gb),", 1),
    ("ppo3w.hip", "if (kind == 0) hipLaunchKernelGGL((ppo3w_build_rec_kernel<4, 0>), dim3(gb),", 1),
    ("ppo3w.hip", "else hipLaunchKernelGGL((ppo3w_build_rec_kernel<3, 1>), dim3(gb),", 1),
    ("ppo3w.hip", "hipLaunchKernelGGL((ppo3w_fwd_kernel<NS_, 2, ACT_, CONT_, 0>), dim3(nrowsS),", 1),
    ("ppo3w.hip", "hipLaunchKernelGGL((ppo3w_fwd_kernel<NS_, 1, ACT_, CONT_, 1>), dim3(nrowsS),", 1),
    ("ppo3w.hip", "hipLaunchKernelGGL((ppo3w_dw2_kernel<NS_, ACT_>), dim3(2 * nsr, 2),", 1),
    ("ppo3w.hip", "hipLaunchKernelGGL((ppo3w_dw2_kernel<NS_, ACT_>), dim3(2 * nsr), dim3(NTW), DW2W_LDS, s, g, 0, nsr);", 1),
    ("ppo3w.hip", "W3_LAUNCH_BWD(NS_, ACT_, 0);", 2),
    ("ppo3w.hip", "W3_LAUNCH_BWD(NS_, ACT_, 1);", 1),
    ("ppo3w.hip", "if (w3_dzf_pad()) {", 1),
    ("ppo3w.hip", "hipLaunchKernelGGL((ppo3w_bwd_kernel<NS_, ACT_, true>), dim3(nrowsS),", 1),
    ("ppo3w.hip", "hipLaunchKernelGGL((ppo3w_bwd_kernel<NS_, ACT_, false>), dim3(nrowsS),", 1),
    ("ppo3w.hip", "if (pd.act == 0) LAUNCH_GW(4, 0, 0);", 1),
    ("ppo3w.hip", "else LAUNCH_GW(4, 1, 0);", 1),
    ("ppo3w.hip", "if (pd.act == 0) LAUNCH_GW(3, 0, 1);", 1),
    ("ppo3w.hip", "else LAUNCH_GW(3, 1, 1);", 1),
    ("ppo3w.hip", "hipLaunchKernelGGL((dqn3w_gather_kernel<NS_>), dim3(gb),", 1),
    ("ppo3w.hip", "hipLaunchKernelGGL((ppo3w_fwd_kernel<NS_, NA_, ACT_, 0, 2>), dim3(nrowsS),", 1),
    ("ppo3w.hip", "hipLaunchKernelGGL((ppo3w_fwd_kernel<NS_, NA_, ACT_, 0, 3>), dim3(nrowsS),", 1),
    ("ppo3w.hip", "if (ns == 4 && na == 2) { if (act == 0) LAUNCH_DW(4, 2, 0); else LAUNCH_DW(4, 2, 1); }", 1),
    ("ppo3w.hip", "else if (ns == 2 && na == 3) { if (act == 0) LAUNCH_DW(2, 3, 0); else LAUNCH_DW(2, 3, 1); }", 1),
    ("ppo3w.hip", "else { if (act == 0) LAUNCH_DW(3, 3, 0); else LAUNCH_DW(3, 3, 1); }", 1),
    ("ppo3w.hip", "hipLaunchKernelGGL((dqn3w_plan_kernel<NS_, NA_, ACT_>), grid,", 1),
    ("ppo3w.hip", "if (ns == 4 && na == 2) { if (act == 0) LAUNCH_PW(4, 2, 0); else LAUNCH_PW(4, 2, 1); }", 1),
    ("ppo3w.hip", "else if (ns == 2 && na == 3) { if (act == 0) LAUNCH_PW(2, 3, 0); else LAUNCH_PW(2, 3, 1); }", 1),
    ("ppo3w.hip", "else { if (act == 0) LAUNCH_PW(3, 3, 0); else LAUNCH_PW(3, 3, 1); }", 1),
]

LAUNCH_MACRO_USES = {  # file -> number of LAUNCH_* invocations (a new branch adds one)
    "dqn3.hip": 12, "ppo3.hip": 8, "ppo3w.hip": 21,
}
KERNEL_LAUNCHES = {  # file -> number of hipLaunchKernelGGL calls (a new launch site is a new row or an unlisted kernel)
    "dqn3.hip": 13, "ppo3.hip": 6, "ppo3w.hip": 26,
}


def _src(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def test_dispatch_lines_match_the_instantiation_table():
    moved = [(f, s, n, _src(f).count(s)) for f, s, n in PINNED if _src(f).count(s) != n]
    assert not moved, ("a dispatch line of the three-layer bf16 learners changed -- update tests/bf16_learner_matrix.py (and "
                       f"the GPU matrix) so that every instantiation is still reached, then this list: {moved}")
    uses = {f: len(re.findall(r"(?<!define )\b(?:W3_)?LAUNCH_[A-Z0-9_]*\(", _src(f))) for f in LAUNCH_MACRO_USES}
    assert uses == LAUNCH_MACRO_USES, uses
    launches = {f: _src(f).count("hipLaunchKernelGGL(") for f in KERNEL_LAUNCHES}
    assert launches == KERNEL_LAUNCHES, launches


# ------------------------------------------------------------------ the dispatch, restated from the pinned lines above
NSNA = {4: 2, 2: 3, 3: 3}


def dqn3_plan_insts(ns, na, act, n, h=128):
    if h == 256:
        return [f"dqn3w_plan_kernel<{ns}, {na}, {act}>"]
    return [f"mlp3_plan32_kernel<{ns}, {na}, {act}, NoActTail>" if n <= 1 << 15 else f"mlp3_plan_kernel<{ns}, {na}, {act}>"]


def dqn3_act_insts(env, act, n, h=128):
    ns, na = M.ENVS[env], M.DQN_NA[env]
    assert h == 128 and 1 <= n <= 1 << 15, "rlhip_dqn3_act_supported refuses it"
    return [f"mlp3_plan32_kernel<{ns}, {na}, {act}, ActTail<{M.ENV_CLASS[env]}>>"]


def dqn3_grad_insts(ns, na, act, batch, h=128, pad=0, update=False):
    if h == 256:
        return [f"dqn3w_gather_kernel<{ns}>", f"ppo3w_fwd_kernel<{ns}, {na}, {act}, 0, 2>",
                f"ppo3w_fwd_kernel<{ns}, {na}, {act}, 0, 3>", f"ppo3w_bwd_kernel<{ns}, {act}, {'true' if pad else 'false'}>",
                f"ppo3w_dw2_kernel<{ns}, {act}>"]
    assert 1 <= batch <= 1024 * 128, "refused: batch too large for one launch"
    if batch <= 8192:
        g = f"dqn3_grad32_kernel<{ns}, {na}, {act}, 1>"
    elif batch >= 65536:
        g = f"dqn3_grad32_kernel<{ns}, {na}, {act}, 2>"
    else:
        g = f"dqn3_grad_kernel<{ns}, {na}, {act}>"
    return [g] + ([f"d3_apply_kernel after {M.grad_form(g)}"] if update else [])


def ppo3_rollout_insts(env, act, n, h=128):
    P, ns = M.ENV_CLASS[env], M.ENVS[env]
    if h == 256:
        return [f"ppo3w_rollout_kernel<{P}, 2, {act}, false>", f"ppo3w_fwd_kernel<{ns}, 1, {act}, 0, 4>"]
    return [f"ppo3_rollout32_kernel<{P}, 2, {act}>" if n <= 1 << 15 else f"ppo3_rollout_kernel<{P}, 2, {act}>"]


def ppo3_grad_insts(env, act, h=128, force128=False, pad=0, rec=False):
    ns, c = M.ENVS[env], int(M.PPO_ENVS[env])
    if h == 256:
        gather = f"ppo3w_gather_rec_kernel<{ns}>" if rec else f"ppo3w_gather_kernel<{ns}, {c}>"
        return ([f"ppo3w_build_rec_kernel<{ns}, {c}>"] if rec else []) + [
            gather, f"ppo3w_fwd_kernel<{ns}, 2, {act}, {c}, 0>", f"ppo3w_fwd_kernel<{ns}, 1, {act}, {c}, 1>",
            f"ppo3w_bwd_kernel<{ns}, {act}, {'true' if pad else 'false'}>", f"ppo3w_dw2_kernel<{ns}, {act}>"]
    chained = act == 0 and not force128
    return [f"ppo3_gradT_kernel<{ns}, 0, {c}>" if chained else f"ppo3_grad_kernel<{ns}, 2, {act}, {c}>"]


def launched(r):
    """what the row's problem launches, by the model above"""
    env, act, h = r["env"], r["act"], r["hidden"]
    ns = M.ENVS[env]
    k = r["kernel"]
    if r["id"].startswith("dqn3_act"):
        return dqn3_act_insts(env, act, r["n"], h)
    if k in ("mlp3_plan32_kernel", "mlp3_plan_kernel", "dqn3w_plan_kernel"):
        out = dqn3_plan_insts(ns, NSNA[ns], act, r["n"], h)
        if "n2" in r:
            assert dqn3_plan_insts(ns, NSNA[ns], act, r["n2"], h) == out, r["id"]
        return out
    if r["id"].startswith("dqn3"):
        return dqn3_grad_insts(ns, NSNA[ns], act, r.get("batch", 1), h, r.get("pad", 0), update=k == "d3_apply_kernel")
    if "rollout" in r["id"]:
        return ppo3_rollout_insts(env, act, r["n"], h)
    return ppo3_grad_insts(env, act, h, r.get("force128", False), r.get("pad", 0), r.get("rec", False))


def test_every_row_reaches_the_instantiation_it_names():
    for r in M.ROWS:
        got = launched(r)
        for inst in M.owned(r):
            assert inst in got, (r["id"], inst, got)
    for r in M.DQN3_UPDATE:
        assert launched(r)[0] == r["after"], r["id"]
    # the thresholds each gradient form is pinned at: just past each lower one, and the largest batch one launch takes
    batches = {r["inst"].split("<")[0] + ("<2>" if r["inst"].endswith(", 2>") else ""): set() for r in M.DQN3_GRAD}
    for r in M.DQN3_GRAD:
        batches[r["inst"].split("<")[0] + ("<2>" if r["inst"].endswith(", 2>") else "")].add(r["batch"])
    assert 8192 in batches["dqn3_grad32_kernel"] and 8193 in batches["dqn3_grad_kernel"] and 65535 in batches["dqn3_grad_kernel"]
    assert {65536, 65537, 1024 * 128} <= batches["dqn3_grad32_kernel<2>"]
    # the chained tile with more tiles than persistent workgroups (RLHIP_PPO3_WGS caps them at 128 per net)
    for r in M.PPO3:
        if r["kernel"] == "ppo3_gradT_kernel":
            assert (r["n"] * r["T"] // r["nmb"] + 127) // 128 > 128, r["id"]
        if r["kernel"] == "ppo3_rollout_kernel":
            assert r["n"] > 1 << 15
    for r in M.DQN3_PLAN:
        if r["kernel"] == "mlp3_plan_kernel":
            assert r["n"] == (1 << 15) + 1 and r["n2"] > r["n"] and r["n2"] % 128 != 0


def _reachable():
    every = set()
    for ns, na in NSNA.items():
        for act in (0, 1):
            for n in (1, 1 << 15, (1 << 15) + 1):
                every.update(dqn3_plan_insts(ns, na, act, n))
            every.update(dqn3_plan_insts(ns, na, act, 1, h=256))
            for batch in (1, 8192, 8193, 65535, 65536, 1024 * 128):
                every.update(dqn3_grad_insts(ns, na, act, batch, update=True))
            for pad in (0, 1):
                every.update(dqn3_grad_insts(ns, na, act, 1, h=256, pad=pad))
    for env in M.ENVS:
        for act in (0, 1):
            every.update(dqn3_act_insts(env, act, 1))
    for env in M.PPO_ENVS:
        for act in (0, 1):
            for n in (1, (1 << 15) + 1):
                every.update(ppo3_rollout_insts(env, act, n))
            every.update(ppo3_rollout_insts(env, act, 1, h=256))
            for force in (False, True):
                every.update(ppo3_grad_insts(env, act, force128=force))
            for pad in (0, 1):
                for rec in (False, True):
                    every.update(ppo3_grad_insts(env, act, h=256, pad=pad, rec=rec))
    return every


def test_the_table_lists_every_reachable_instantiation_exactly_once():
    listed = [i for r in M.ROWS for i in M.owned(r)]
    assert len(listed) == len(set(listed)), sorted(i for i in set(listed) if listed.count(i) > 1)
    every = _reachable()
    assert set(listed) == every, (sorted(every - set(listed)), sorted(set(listed) - every))
    plain = {i.split(" after ")[0] for i in every}
    assert sum(i.startswith("mlp3_plan_kernel<") for i in plain) == 6
    assert sum(i.startswith("dqn3_grad_kernel<") for i in plain) == 6
    assert sum(i.startswith("dqn3_grad32_kernel<") for i in plain) == 12
    assert sum("ActTail<" in i for i in plain) == 6
    assert sum(i.startswith("ppo3_rollout_kernel<") for i in plain) == 4
    assert sum(i.startswith("ppo3_rollout32_kernel<") for i in plain) == 4
    assert sum(i.startswith("ppo3_grad_kernel<") for i in plain) == 4
    assert sum(i.startswith("ppo3w_bwd_kernel<") for i in plain) == 12
    assert not any(i.startswith("ppo3_gradT_kernel<") and ", 1, " in i[17:21] for i in plain)
    assert len({r["id"] for r in M.ROWS}) == len(M.ROWS)


def test_every_row_is_a_test_id_of_the_gpu_matrix():
    import test_gpu_bf16_learner_matrix as G

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

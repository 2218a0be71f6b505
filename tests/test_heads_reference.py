"""tests/heads_ref.py (float64 model + derived error budget) against the oracle (oracle/rlo_heads.c, Float32 on glibc): every case
that tests/test_gpu_heads.py runs on the device is run here on the oracle's own output, which shows that the 2 x budget bar and
the left-out caps are satisfiable by the reference alone; a handful of planted faults show that the bar is not satisfiable by a
wrong head -- including the ones the bar it replaces, `(err < 1e-3 + tol).mean() > 0.97 and err.max() < 0.5`, let through."""
import numpy as np
import pytest

import heads_ref as H
import oracle


class OracleHeads:
    @staticmethod
    def sample(mu, raw, K, lo, hi, family, seed, base, step):
        sq, soft = H.SQUASH_SOFT[family]
        return oracle.gaussian_head_sample(mu, raw, K, lo, hi, sq, soft, seed=seed, env_id_base=base, step=step)

    @staticmethod
    def logp(mu, raw, a, lo, hi, family):
        sq, soft = H.SQUASH_SOFT[family]
        return oracle.gaussian_head_logp(mu, raw, a, lo, hi, sq, soft)


O = OracleHeads


@pytest.mark.parametrize("family", H.FAMILIES)
def test_oracle_lies_within_the_budget_on_every_shape(family):
    res = []
    for d, n, K in H.SHAPES:
        res += H.run_shape(O, O, family, d, n, K)
    for d, n, K in H.SCALED_SHAPES:
        res += H.run_shape(O, O, family, d, n, K, scale=3.0)
    assert H.pooled_left_out(res) <= H.EVAL_CAP
    if family == "tanh":      # mu x 3 saturates tanhf: the +Inf samples are there and were matched
        assert sum(r["non_finite"] for r in res if "x 3" in r["tag"]) >= 20
    if family != "tanh":      # nothing but GaussianNetwork tanh evaluation leaves a sample out
        assert all(r["left_out"] == 0 for r in res)


@pytest.mark.parametrize("family", ["tanh", "soft"])
def test_oracle_lies_within_the_budget_on_the_action_grid(family):
    assert H.run_grid(O, family)["left_out"] == 0


@pytest.mark.parametrize("name", sorted(H.edge_cases()))
@pytest.mark.parametrize("family", H.FAMILIES)
def test_oracle_lies_within_the_budget_on_the_edges(family, name):
    H.run_edge(O, O, family, name, H.edge_cases()[name])


def test_glibc_tanhf_on_the_sweep():
    x = H.tanh_sweep()[None, :]
    a, _ = O.sample(x, np.ones_like(x), 1, 0.0, 0.0, "tanh", 1, 0, 0)
    assert H.check_tanh_sweep(x[0], a[0, 0]) <= H.E["tanh"]


def test_normlogpdf_models_hold_the_oracle():
    rng = np.random.default_rng(5)
    n = 1000
    mu, x, sg = rng.standard_normal(n).astype(np.float32), rng.standard_normal(n).astype(np.float32), rng.uniform(0.1, 3, n).astype(np.float32)
    sg[:10] = 0.0
    o = np.array([oracle.normlogpdf(float(a), float(b), float(c)) for a, b, c in zip(mu, sg, x)], np.float32)
    assert H.judge(o, *H.normlogpdf(mu, sg, x), tag="normlogpdf")["worst_over_bar"] <= 1
    for d in (1, 3, 64, 200):
        MU, SG, X = (rng.standard_normal((d, 33)).astype(np.float32), rng.uniform(0.2, 2, (d, 33)).astype(np.float32),
                     rng.standard_normal((d, 33)).astype(np.float32))
        H.judge(oracle.diagnormlogpdf(MU, SG, X), *H.diagnormlogpdf(MU, SG, X), tag=f"diagnormlogpdf d={d}")


# ------------------------------------------------------------------------------------------------------------ planted faults
def _old_bar(lp, lpo, d):
    """the assertion this budget replaces (tests/test_gpu_heads.py before: tanh sampling and every squashed evaluation)"""
    with np.errstate(invalid="ignore"):
        err = np.abs(lp - lpo)
        tol = 2e-5 + 2e-6 * np.abs(lpo) * d
        return bool((err < 1e-3 + tol).mean() > 0.97 and err.max() < 0.5)


def _fails_budget(family, mu, raw, z, a, lp):
    try:
        H.judge_sampling(family, mu, raw, H.LO, H.HI, z, a, lp)
    except AssertionError:
        return True
    return False


def test_wrong_heads_fail_the_budget_and_some_passed_the_old_bar():
    d, n, K = 6, 1000, 3
    mu, raw = H.inputs(d, n, seed=d)
    sg = H.clamp(raw, H.LO, H.HI)
    z, lpi = O.sample(mu, raw, K, H.LO, H.HI, "identity", H.SEED, H.BASE, H.STEP)
    t, lpo = O.sample(mu, raw, K, H.LO, H.HI, "tanh", H.SEED, H.BASE, H.STEP)
    assert not _fails_budget("tanh", mu, raw, z, t, lpo) and _old_bar(lpo, lpo, d)
    u = (np.float32(1) - t * t).astype(np.float64)               # the Float32 replay of 1 - t^2
    base = H.gaussian_sample(mu, sg, z)[0]                       # diagnormlogpdf part (float64 centre)
    with np.errstate(all="ignore"):
        corr = np.log(u).sum(0)
        wrong = {
            "eps_1e-7": base - np.log(u + 1e-7).sum(0),          # SAC-style log(1 - t^2 + eps)
            "eps_1e-6": base - np.log(u + 1e-6).sum(0),
            "wrong_sign": base + corr,                           # lp + corr instead of lp + (-corr)
            "unclamped_sigma": H.gaussian_sample(mu, raw, z, t)[0],
            "log2pi_once": base - corr + 0.5 * (d - 1) * float(H.LOG2PI),
        }
    # draw k + d j rounded down to even: both halves of a Philox pair (q / 2, q & 1) replaced by the first
    flat, _ = O.sample(np.zeros((1, n), np.float32), np.ones((1, n), np.float32), d * K, 1.0, 1.0, "identity", H.SEED, H.BASE, H.STEP)
    q = np.arange(d)[:, None] + d * np.arange(K)[None, :]
    assert np.array_equal(mu[:, None, :] + sg[:, None, :] * flat[0][q], z)
    noise = flat[0][q & ~1]                                      # (d, K, n)
    z_even = (mu[:, None, :] + sg[:, None, :] * noise).astype(np.float32)
    t_even = np.tanh(z_even.astype(np.float64)).astype(np.float32)
    passed_old = {}
    for name, lp in wrong.items():
        lp = lp.astype(np.float32)
        assert _fails_budget("tanh", mu, raw, z, t, lp), name
        passed_old[name] = _old_bar(lp, lpo, d)
    lp_even = H.gaussian_sample(mu, sg, z_even, t_even)[0].astype(np.float32)
    assert _fails_budget("tanh", mu, raw, z, t_even, lp_even) and _fails_budget("tanh", mu, raw, z, t, lp_even)
    passed_old["even_draw_index"] = _old_bar(lp_even, lpo, d)
    # the old bar: share 0.995 / max 1.0e-1 for eps = 1e-7 -- it passed; the budget has 24 % of its samples beyond the bar, by up to 7400 x
    assert passed_old == {"eps_1e-7": True, "eps_1e-6": False, "wrong_sign": False, "unclamped_sigma": False, "log2pi_once": False,
                          "even_draw_index": False}, passed_old
    exp, bud, _ = H.gaussian_sample(mu, sg, z, t)
    over = np.abs(wrong["eps_1e-7"].astype(np.float32) - exp) / (2 * bud)
    assert 0.15 < (over > 1).mean() < 0.3 and over.max() > 500
    over6 = np.abs(wrong["eps_1e-6"].astype(np.float32) - exp) / (2 * bud)
    assert (over6 > 1).all()

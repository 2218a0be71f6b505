"""The judge of rlhip_dqn_grad_batch_f32 (tests/dqn_batch_ref.py) judged itself, on the CPU:

  * without per-sample discounts and Double DQN it IS oracle.dqn_loss_grad, bit for bit;
  * with per-sample discounts, weights and Double DQN it agrees with Float64 torch autograd under the rounding bars of
    tests/test_oracle_vs_torch.py's Float64 section;
  * the input sets of the GPU tests pass the census: no Double DQN sample whose online top-two gap a re-ordered Float32 sum could
    close (zero samples left out), and the rows the issue asks for are present."""
import numpy as np
import pytest
import torch

import oracle
import dqn_batch_ref as ref
from test_oracle_vs_torch import _assert_within_rounding_bar, _mlp64, U


@pytest.mark.parametrize("ns,h,na,act", [(5, 4, 1, 0), (6, 128, 3, 0), (6, 64, 3, 1), (16, 256, 4, 1)])
def test_model_is_the_oracle_without_discount_vector_and_double(ns, h, na, act):
    for weights in (False, True):
        c = ref.make_case(ns, h, na, act, 130, seed=11 + ns + h, weights=weights)
        loss, grad, td = ref.case_loss_grad(c)
        lo, go = oracle.dqn_loss_grad(ns, h, na, act, c["p"], c["pt"], c["s"], c["a"], c["r"], c["term"], c["sn"], c["gamma"], c["delta"],
                                      weights=c["weights"])
        assert loss == lo and np.array_equal(grad, go)
        assert td[:3].max() == 0.0  # the d = 0 rows


def test_discounts_are_the_oracles_powers_clamped():
    d = ref.discounts(0.9, np.array([-3, 0, 1, 2, 32, 40]))
    assert d.dtype == np.float32
    assert list(d) == [np.float32(oracle.gamma_pow(0.9, n)) for n in (0, 0, 1, 2, 32, 32)]
    assert d[1] == 1.0 and d[2] == np.float32(0.9)


@pytest.mark.parametrize("act", [0, 1])
@pytest.mark.parametrize("ns,na", [(5, 3), (6, 3), (16, 4)])
def test_model_against_float64_autograd(ns, na, act):
    from torch.func import grad, vmap

    h, B = 24, 160
    c = ref.make_case(ns, h, na, act, B, seed=300 + ns + 7 * act, n_used=True, weights=True, double_dqn=True)
    loss, g, td = ref.case_loss_grad(c)
    gamma, delta = c["gamma"], c["delta"]
    P, PT = torch.tensor(c["p"], dtype=torch.float64), torch.tensor(c["pt"], dtype=torch.float64)
    S, SN = torch.tensor(c["s"].T, dtype=torch.float64), torch.tensor(c["sn"].T, dtype=torch.float64)
    A = torch.tensor(np.eye(na)[c["a"]])
    W = torch.tensor(c["weights"], dtype=torch.float64)
    disc = torch.tensor(np.float64(gamma) ** np.clip(c["n_used"], 0, 32).astype(np.float64))
    with torch.no_grad():
        qo = vmap(lambda x: _mlp64(P, ns, h, na, act, x))(SN)
        qt = vmap(lambda x: _mlp64(PT, ns, h, na, act, x))(SN)
        sel = qt.gather(1, qo.argmax(1, keepdim=True))[:, 0]
        G = torch.tensor(c["r"], dtype=torch.float64) + disc * (1 - torch.tensor(c["term"], dtype=torch.float64)) * sel
        q = (vmap(lambda x: _mlp64(P, ns, h, na, act, x))(S) * A).sum(1)
    assert np.array_equal(qo.argmax(1).numpy(), ref.target(ns, h, na, act, c["p"], c["pt"], c["r"], c["term"], c["sn"], gamma, c["n_used"],
                                                           True)[1])
    d = (q - G).numpy()
    quad = np.abs(d) < delta
    assert 0.1 <= quad.mean() <= 0.9, f"both Huber branches: {quad.mean():.2f} quadratic"

    def loss_b(pp, x, ab, gb, wb):
        e = (_mlp64(pp, ns, h, na, act, x) * ab).sum() - gb
        return wb * torch.where(e.abs() < delta, 0.5 * e * e, delta * (e.abs() - 0.5 * delta)) / B

    gb = vmap(grad(loss_b), in_dims=(None, 0, 0, 0, 0))(P, S, A, G, W).numpy()
    g64 = gb.sum(0)
    lb = vmap(loss_b, in_dims=(None, 0, 0, 0, 0))(P, S, A, G, W).numpy()
    # the Float32 powers gamma^n carry up to 31 roundings of their own, into G: they join the chain that feeds the cancelling difference
    amp = np.where(quad, 1.0 + (np.abs(q.numpy()) + np.abs(G.numpy())) / np.maximum(np.abs(d), 1e-30), 1.0)
    K = (ns + 1) + (h + 1) + 2 * (ns + 1) + 12 + 32
    _assert_within_rounding_bar(g, g64, np.abs(gb), amp, K, f"batch model ns={ns} na={na} act={act}")
    assert abs(loss - float(lb.sum())) <= K * U * float((amp * 2 * np.abs(lb)).sum()) + U * abs(float(lb.sum()))
    np.testing.assert_allclose(td, np.abs(d), rtol=1e-4, atol=1e-5)


def _every_gpu_case():
    for shape, batches in ref.grid():
        for b, k in batches:
            yield ref.make_case(*shape, b, seed=1000 + k, **ref.flags(k)), k
    yield ref.make_case(16, 256, 3, 0, ref.BIG_BATCH, seed=77, **ref.flags(7)), None


def test_gpu_input_sets_pass_the_census():
    seen, left_out, n_double, worst_cond = set(), 0, 0, 0.0
    rows = dict(term=0, quad=0, lin=0, zero=0, cut=0)
    for c, k in _every_gpu_case():
        if k is not None:
            seen.add(k % 16)
        # one rounding of 2^-24 in each of Q(s)[a] and y, amplified `conditioning` times, has to stay under F32_GRAD_TOL = 1e-6 = 16.8 x
        # 2^-24: conditioning <= 8
        worst_cond = max(worst_cond, ref.conditioning(c))
        if c["batch"] > 4096:  # (its rows are counted by the census only)
            left_out += ref.census(c)
            continue
        if c["double_dqn"]:
            n_double += c["batch"]
            left_out += ref.census(c)
        _, _, td = ref.case_loss_grad(c)
        rows["term"] += int(c["term"].sum())
        rows["quad"] += int(((td < c["delta"]) & (td > 0)).sum())
        rows["lin"] += int((td >= c["delta"]).sum())
        rows["zero"] += int((td == 0).sum())
        if c["n_used"] is not None:
            assert c["n_used"].min() >= 1 and c["n_used"].max() <= 32
            rows["cut"] += int(((c["term"] != 0) & (c["n_used"] < 32)).sum())
    assert left_out == 0, f"{left_out} Double DQN samples sit within twice the re-ordering bound of a tie (cap: 0)"
    assert seen == set(range(16)), "every combination of n_used / weights / double_dqn / td_out"
    assert worst_cond <= 8.0, f"an input set whose db2 cancels: conditioning {worst_cond:.1f}"
    assert n_double > 10000 and all(v > 0 for v in rows.values()), rows

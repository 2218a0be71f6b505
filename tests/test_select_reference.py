"""The oracle's action selection (oracle/rlo_select.c) against the independent model tests/select_ref.py on the case grids of
tests/select_cases.py, and its sampling laws against select_ref.law.  CPU only.

The GPU tests pin the kernels to the oracle bit for bit; the oracle is the kernels' twin, statement for statement, so a
misreading of the reference that both share is invisible there.  Here the oracle meets a model written from the reference's
text alone: decisions must agree wherever the model's margin exceeds the derived Float32 budget (select_ref's docstring), the
share of columns that rule leaves out is capped at 1e-3 per case, the grids whose arithmetic is exact take no allowance, and
every planted misreading (`fault=`) must be caught.  tests/test_gpu_select_edges.py runs the same grids and statistics on the
kernels.
"""
import numpy as np
import pytest

import oracle
import select_cases as SC
import select_ref as R

ALL_CASES = [c for e in SC.ENTRIES for c in SC.cases(e)]




@pytest.mark.parametrize("entry", SC.ENTRIES)
def test_census_and_coverage(entry):
    """no class of any grid is empty; every addressing, mask encoding, step, shape and the wrapping env id occur"""
    for c in SC.cases(entry):
        SC.census(c)
    SC.coverage(entry)


@pytest.mark.parametrize("case", ALL_CASES, ids=lambda c: c.id)
def test_oracle_agrees_with_model(case):
    j = SC.judge(case, SC.run_oracle(case))
    print(f"{case.id}: mismatch {j.mismatch} excluded {j.excluded:.2e} logp err {getattr(j, 'logp_err', 0):.3e} "
          f"budget {getattr(j, 'logp_budget', 0):.3e}")
    assert j.mismatch == 0
    assert j.excluded == 0 if SC.is_exact(case) else j.excluded <= SC.EXCLUDED_CAP


def test_pinf_logit_is_the_plain_formula():
    """NOT pinned to the reference (NNlib may special-case Inf): a +Inf logit poisons the column through Inf - Inf = NaN; the
    oracle returns action 0 with a NaN log-probability, as x - max - log(sum(exp(x - max))) does."""
    for case in SC.cases("categorical"):
        if case.mask is None and len(case.classes.get("pinf", ())):
            ix = case.classes["pinf"]
            got = SC.run_oracle(case)
            assert np.all(got["actions"][ix] == 0) and np.all(np.isnan(got["logp"][ix]))


FAULT_ENTRIES = dict(last_max=("eps_greedy",), nan_not_max=("eps_greedy",), nan_tie=("eps_greedy", "prob", "ucb"),
                     u_gt_eps=("eps_greedy",), rand_all_under_mask=("eps_greedy",), mask_after_softmax=("categorical",),
                     walk_le=("weighted",), masked_weight_kept=("weighted",), ignore_is_normalized=("weighted",),
                     index_mod=("eps_greedy", "ucb"), shared_uniform=("categorical",), gumbel_add=("categorical", "gumbel_softmax"),
                     ucb_log_step=("ucb",), ucb_no_increment=("ucb",))
assert set(FAULT_ENTRIES) == set(R.FAULTS)
_oracle_cache = {}


def _oracle_cached(case):
    if case.id not in _oracle_cache:
        _oracle_cache[case.id] = SC.run_oracle(case)
    return _oracle_cache[case.id]


@pytest.mark.parametrize("fault", R.FAULTS)
def test_every_fault_is_caught(fault):
    """the model with ONE misreading planted disagrees with the oracle on judged columns, in every entry point it touches"""
    for entry in FAULT_ENTRIES[fault]:
        caught = 0
        for case in SC.cases(entry):
            if case.n > 300:
                continue  # the small grids hold every class already
            caught += SC.judge(case, _oracle_cached(case), fault=fault).mismatch
            if caught:
                break
        print(f"{fault} on {entry}: caught on {case.id}")
        assert caught > 0, (fault, entry)


# ---------------------------------------------------------------------------------------------- laws and independence
@pytest.mark.parametrize("c", SC.law_cases(), ids=lambda c: c.id)
def test_oracle_law(c):
    """chi^2 of 2^17 draws from one column against the exact law of the model, bar = the 1 - 1e-6 quantile"""
    stat, dof, cnt = SC.chi2_counts(SC.law_oracle(c), c.p, c.na)
    bar = SC.chi2_bar(dof)
    print(f"{c.id}: chi2 {stat:.2f} dof {dof} bar {bar:.2f}")
    assert stat < bar  # (one legal action: dof 0, bar 0 -- chi2_counts is +inf unless every draw is that action, and then -1)
    if c.entry == "eps_greedy":  # the law of the draw IS what prob() returns: ties the two entry points to each other
        p = oracle.eps_greedy_prob(c.column.astype(np.float64), c.eps, c.mask_column, c.is_break_tie)
        assert np.array_equal(p, c.p)


@pytest.mark.parametrize("c", SC.INDEPENDENCE, ids=lambda c: c.id)
def test_oracle_independence(c):
    """3 x 3 contingency chi^2 of (a_i at step t, a_i at step t + 1) and of (a_i, a_{i+1}) at one step"""
    a0, a1 = SC.law_oracle(c), SC.law_oracle(c, step=c.step + 1)
    for name, (x, y) in dict(steps=(a0, a1), neighbours=(a0[:-1], a0[1:])).items():
        stat, dof, _ = SC.chi2_independence(x, y)
        bar = SC.chi2_bar(dof)
        print(f"{c.id} {name}: chi2 {stat:.2f} dof {dof} bar {bar:.2f}")
        assert stat < bar


LAW_FAULT_N = 1 << 15  # the model draws through one host call per Philox block; the planted laws are far off at this size


def _law_model(c, fault, n=LAW_FAULT_N):
    v = SC.tile(c.column, n)
    m = None if c.mask_column is None else SC.tile(c.mask_column, n)
    d = R.draws(c.entry, c.seed, c.env_id_base, n, c.step, c.na, fault=fault)
    if c.entry == "categorical":
        return R.categorical(v, d["u"], m, fault).decision
    return R.eps_greedy(v, c.eps, d["u"], d["rand_w"], d["tie_w"], m, c.is_break_tie, fault).decision


@pytest.mark.parametrize("fault", R.LAW_FAULTS)
def test_law_faults(fault):
    """A shared uniform and added Gumbel noise change the law of the draw: the statistic of the faulted model exceeds the bar.
    `w % n` does NOT: it maps a uniform 32-bit word to a uniform index just as (w * n) >> 32 does (both within n 2^-32), so
    no statistic of the action counts can see it -- it is caught on the grids (test_every_fault_is_caught), where the index
    itself is compared, and here the test asserts what is true of it: its counts stay under the bar."""
    by_id = {c.id: c for c in SC.law_cases()}
    c = by_id["eps_greedy-na5"] if fault == "index_mod" else by_id["categorical-na3"]
    clean = SC.chi2_counts(_law_model(c, None), c.p, c.na)
    stat, dof, _ = SC.chi2_counts(_law_model(c, fault), c.p, c.na)
    bar = SC.chi2_bar(dof)
    print(f"{fault}: chi2 {stat:.2f} (unfaulted model {clean[0]:.2f}) dof {dof} bar {bar:.2f}")
    assert clean[0] < bar
    assert stat < bar if fault == "index_mod" else stat > bar

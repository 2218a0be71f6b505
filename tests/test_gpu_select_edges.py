"""The selection kernels (csrc/select.hip, csrc/select_device.h) on the case grids of tests/select_cases.py, through the C ABI:
against the independent model tests/select_ref.py under its margin rule, against the oracle bit for bit, and the sampling
laws of 2^17 draws per case against select_ref.law.  tests/test_select_reference.py runs the same on the oracle.

Addressing: "soa" and "julia" go through rlhip.ops / the explorer classes with contiguous tensors (the explorers take a
transposed view for "julia"); "strided" hands a non-contiguous window of a larger NaN-filled buffer to the C ABI with its
strides.  Masks are torch.bool or uint8 holding 2 / 255.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import select_cases as SC

pytestmark = pytest.mark.gpu
POISON_I, POISON_F = -77, 12345.0
EXPLORER = dict(weighted="WeightedExplorer", weighted_softmax="WeightedSoftmaxExplorer", gumbel_softmax="GumbelSoftmaxExplorer")
ALL_CASES = [c for e in SC.ENTRIES for c in SC.cases(e)]


def _place(a, addressing, fill):
    """device tensor holding the (na, n) host array `a` under `addressing` -> (the (na, n) view, k_stride, i_stride, base)"""
    na, n = a.shape
    t = torch.as_tensor(np.ascontiguousarray(a))
    if addressing == "soa":
        d = t.cuda().contiguous()
        return d, n, 1, d
    if addressing == "julia":
        base = t.t().contiguous().cuda()  # (n, na): the storage of a Julia (na, n) matrix
        return base.t(), 1, na, base
    big = torch.full((na + 3, n + 7), fill, dtype=t.dtype).cuda()
    view = big[1:na + 1, 2:n + 2]
    view.copy_(t.cuda())
    return view, big.stride(0), 1, big


def _mask(case):
    if case.mask is None:
        return None
    if case.mask_kind == "bool":
        return case.mask
    return SC.mask_u8(case)


def _same_bits(a, b):
    """Float32 arrays equal bit for bit (signed zeros included); a NaN matches any NaN -- the sign and payload of the NaN that
    Inf + -Inf produces are the platform's, not the formula's"""
    nan = np.isnan(b)
    return np.array_equal(np.isnan(a), nan) and np.array_equal(a.view(np.uint32)[~nan], b.view(np.uint32)[~nan])


def _vp(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def run_kernel(case):
    import rlhip
    from rlhip import ops
    from rlhip._lib import call

    e, addr = case.entry, case.addressing
    v, ks, is_, vbase = _place(case.values, addr, float("nan"))
    m = _mask(case)
    mv = mbase = None
    if m is not None:
        mv, mks, mis, mbase = _place(m, addr, 1 if m.dtype == np.uint8 else True)
        assert (mks, mis) == (ks, is_)
    na, n = case.na, case.n
    direct = addr == "strided"
    arg = (lambda t: t) if addr == "soa" else (lambda t: None if t is None else t.t())  # ops take the storage, shape (n, na)
    m8 = None if mv is None else (mv.view(torch.uint8) if mv.dtype == torch.bool else mv)
    if e == "eps_greedy":
        if direct:
            out = torch.full((n,), POISON_I, dtype=torch.int32, device="cuda")
            call("rlhip_eps_greedy_select_f32", _vp(v), na, n, ks, is_, _vp(m8), float(case.eps), int(case.is_break_tie), case.seed,
                 case.env_id_base, case.step, _vp(out), ops.stream_ptr())
        else:
            out = ops.eps_greedy_select(arg(v), case.eps, case.seed, case.step, case.env_id_base, arg(mv), case.is_break_tie, soa=addr == "soa")
        return dict(actions=out.cpu().numpy())
    if e == "prob":
        if direct:
            pbig = torch.full(tuple(vbase.shape), POISON_F, dtype=torch.float64, device="cuda")
            p = pbig[1:na + 1, 2:n + 2]
            call("rlhip_eps_greedy_prob_f32", _vp(v), na, n, ks, is_, _vp(m8), float(case.eps), int(case.is_break_tie), _vp(p), ops.stream_ptr())
            outside = pbig.clone()
            outside[1:na + 1, 2:n + 2] = POISON_F
            assert bool((outside == POISON_F).all())  # nothing written outside the window
        else:
            p = ops.eps_greedy_prob(arg(v), case.eps, arg(mv), case.is_break_tie, soa=addr == "soa")
            p = p if addr == "soa" else p.t()
        return dict(probs=p.cpu().numpy())
    if e == "categorical":
        if direct:
            a = torch.full((n,), POISON_I, dtype=torch.int32, device="cuda")
            lp = torch.full((n,), POISON_F, dtype=torch.float32, device="cuda")
            call("rlhip_categorical_sample_f32", _vp(v), na, n, ks, is_, _vp(m8), case.seed, case.env_id_base, case.step, _vp(a), _vp(lp),
                 ops.stream_ptr())
        else:
            a, lp = ops.categorical_sample(arg(v), case.seed, case.step, case.env_id_base, arg(mv), soa=addr == "soa")
        return dict(actions=a.cpu().numpy(), logp=lp.cpu().numpy())
    if e == "ucb":
        ex = rlhip.UCBExplorer(na, n_env=n, c=case.c, seed=case.seed)
        ex.step = case.step
        ex.actioncounts = torch.as_tensor(case.counts).cuda().contiguous()
        acts = [ex.plan_(v, env_id_base=case.env_id_base).cpu().numpy() - 1]
        for more in getattr(case, "more_values", []):
            acts.append(ex.plan_(_place(more, addr, float("nan"))[0], env_id_base=case.env_id_base).cpu().numpy() - 1)
        assert ex.step == case.step + case.steps
        return dict(actions=acts, counts=ex.actioncounts.cpu().numpy())
    ex = getattr(rlhip, EXPLORER[e])(seed=case.seed)
    ex.step, ex.is_normalized = case.step, case.is_normalized
    a = ex.plan_(v, env_id_base=case.env_id_base) if mv is None else ex.plan_(v, mv, env_id_base=case.env_id_base)
    return dict(actions=a.cpu().numpy() - 1)


@pytest.mark.parametrize("case", ALL_CASES, ids=lambda c: c.id)
def test_kernel_against_model_and_oracle(case):
    SC.census(case)
    got = run_kernel(case)
    j = SC.judge(case, got)
    print(f"{case.id}: mismatch {j.mismatch} excluded {j.excluded:.2e} logp err {getattr(j, 'logp_err', 0):.3e} "
          f"budget {getattr(j, 'logp_budget', 0):.3e}")
    assert j.mismatch == 0  # the model, wherever its margin exceeds the derived budget
    assert j.excluded == 0 if SC.is_exact(case) else j.excluded <= SC.EXCLUDED_CAP
    ref = SC.run_oracle(case)  # the oracle, bit for bit
    if case.entry == "prob":
        assert np.array_equal(got["probs"], ref["probs"], equal_nan=True)
    elif case.entry == "ucb":
        for s, (a, b) in enumerate(zip(got["actions"], ref["actions"])):
            assert np.array_equal(a, b), s
        assert np.array_equal(got["counts"], ref["counts"], equal_nan=True)
    else:
        assert np.array_equal(got["actions"], ref["actions"])
        if case.entry == "categorical":
            nan = np.isnan(ref["logp"])
            assert np.array_equal(np.isnan(got["logp"]), nan)
            assert np.array_equal(got["logp"].view(np.uint32)[~nan], ref["logp"].view(np.uint32)[~nan])


def test_pinf_logit_is_the_plain_formula():
    """NOT pinned to the reference (see select_ref): a +Inf logit gives action 0 and a NaN log-probability"""
    for case in SC.cases("categorical"):
        if case.mask is None and len(case.classes.get("pinf", ())):
            ix, got = case.classes["pinf"], run_kernel(case)
            assert np.all(got["actions"][ix] == 0) and np.all(np.isnan(got["logp"][ix]))


# ----------------------------------------------------------------------------------------------- CategoricalNetwork
def _net_inputs(na, n, seed):
    cl = dict(SC.LOGIT_CLASSES, **SC.MASK_CLASSES)
    return SC._grid(na, n, cl, True, np.random.default_rng(seed), 0)[:2]


@pytest.mark.parametrize("na,n", [(2, 257), (5, 65), (64, 300), (65, 63)])
@pytest.mark.parametrize("masked", [False, True])
def test_categorical_network(na, n, masked):
    """(net)(state[, mask]; is_sampling, is_return_log_prob): the masked logits are logits + ifelse(mask, 0, -Inf) bit for bit, the
    draw is rlhip_categorical_sample_f32's on the same counters, z its one-hot"""
    import rlhip
    from rlhip import ops

    l, mask = _net_inputs(na, n, 31 * na + n)
    ld = torch.as_tensor(l).cuda()
    md = torch.as_tensor(mask).cuda() if masked else None
    net = rlhip.CategoricalNetwork(lambda s: s, seed=19, env_id_base=WRAPPED)
    net.step = 2 ** 32 - 2
    z, logits = net(ld, md, is_sampling=True, is_return_log_prob=True)
    with np.errstate(all="ignore"):
        want = l + np.where(mask, np.float32(0), np.float32(-np.inf)) if masked else l
    assert _same_bits(logits.cpu().numpy(), want)
    a, _ = ops.categorical_sample(ld, 19, 2 ** 32 - 2, WRAPPED, md)
    assert torch.equal(net.actions, a)
    assert np.array_equal(z.cpu().numpy(), (np.arange(na)[:, None] == a.cpu().numpy()[None, :]).astype(np.float32))
    if masked:
        only = net(ld, md)  # no sampling: the masked logits alone
        assert _same_bits(only.cpu().numpy(), want)


WRAPPED = 2 ** 32 - 40  # the env id wraps inside the launch


@pytest.mark.parametrize("with_mask", [False, True])
def test_categorical_network_null_outputs(with_mask):
    """every legal combination of NULL outputs writes exactly the outputs it was given (poison elsewhere would show a skipped
    store); one-hot without actions, and no output at all, are refused and write nothing"""
    from rlhip import ops
    from rlhip._lib import RLHipArgumentError, call

    na, n = 5, 300
    l, mask = _net_inputs(na, n, 7)
    ld, md = torch.as_tensor(l).cuda(), (torch.as_tensor(mask.astype(np.uint8) * 255).cuda() if with_mask else None)
    with np.errstate(all="ignore"):
        want_m = l + np.where(mask, np.float32(0), np.float32(-np.inf)) if with_mask else l
    a_ref, _ = ops.categorical_sample(ld, 5, 1, 9, md)
    a_ref = a_ref.cpu().numpy()
    for use_m in (False, True):
        for use_a in (False, True):
            for use_z in (False, True):
                mo = torch.full((na, n), POISON_F, dtype=torch.float32, device="cuda")
                ao = torch.full((n,), POISON_I, dtype=torch.int32, device="cuda")
                zo = torch.full((na, n), POISON_F, dtype=torch.float32, device="cuda")
                args = ("rlhip_categorical_network_f32", _vp(ld), na, n, _vp(md), 5, 9, 1, _vp(mo) if use_m else None,
                        _vp(ao) if use_a else None, _vp(zo) if use_z else None, ops.stream_ptr())
                legal = (use_m or use_a) and (use_a or not use_z)
                if legal:
                    call(*args)
                else:
                    with pytest.raises(RLHipArgumentError):
                        call(*args)
                torch.cuda.synchronize()
                mo, ao, zo = mo.cpu().numpy(), ao.cpu().numpy(), zo.cpu().numpy()
                if legal and use_m:
                    assert _same_bits(mo, want_m)
                else:
                    assert np.all(mo == POISON_F)
                if legal and use_a:
                    assert np.array_equal(ao, a_ref)
                else:
                    assert np.all(ao == POISON_I)
                if legal and use_z:
                    assert np.array_equal(zo, (np.arange(na)[:, None] == a_ref[None, :]).astype(np.float32))
                else:
                    assert np.all(zo == POISON_F)


# ---------------------------------------------------------------------------------------------------------- refusals
def test_refusals_leave_outputs_untouched():
    from rlhip import ops
    from rlhip._lib import RLHipArgumentError, call

    n = 70
    v = torch.rand((65, n), device="cuda")
    cnt = torch.full((65, n), 1e-10, dtype=torch.float64, device="cuda")
    out = torch.full((n,), POISON_I, dtype=torch.int32, device="cuda")
    lp = torch.full((n,), POISON_F, dtype=torch.float32, device="cuda")
    pr = torch.full((65, n), POISON_F, dtype=torch.float64, device="cuda")
    s = ops.stream_ptr()
    refused = [("rlhip_explorer_select_f32", k, _vp(v), 65, n, n, 1, None, 0, 1, 0, 1, _vp(out), s) for k in (0, 1, 2)]  # na = 65
    refused += [("rlhip_explorer_select_f32", 3, _vp(v), 4, n, n, 1, None, 0, 1, 0, 1, _vp(out), s),  # kind = 3
                ("rlhip_explorer_select_f32", -1, _vp(v), 4, n, n, 1, None, 0, 1, 0, 1, _vp(out), s),
                ("rlhip_ucb_select_f32", _vp(v), 4, n, n, 1, 2.0, _vp(cnt), 0, 1, 0, _vp(out), s),  # step = 0
                ("rlhip_explorer_select_f32", 0, _vp(v), 0, n, n, 1, None, 0, 1, 0, 1, _vp(out), s),  # na = 0 everywhere
                ("rlhip_ucb_select_f32", _vp(v), 0, n, n, 1, 2.0, _vp(cnt), 1, 1, 0, _vp(out), s),
                ("rlhip_eps_greedy_select_f32", _vp(v), 0, n, n, 1, None, 0.1, 0, 1, 0, 1, _vp(out), s),
                ("rlhip_eps_greedy_prob_f32", _vp(v), 0, n, n, 1, None, 0.1, 0, _vp(pr), s),
                ("rlhip_categorical_sample_f32", _vp(v), 0, n, n, 1, None, 1, 0, 1, _vp(out), _vp(lp), s),
                ("rlhip_categorical_network_f32", _vp(v), 0, n, None, 1, 0, 1, None, _vp(out), None, s)]
    for args in refused:
        with pytest.raises(RLHipArgumentError):
            call(*args)
    torch.cuda.synchronize()
    assert bool((out == POISON_I).all()) and bool((lp == POISON_F).all()) and bool((pr == POISON_F).all())
    assert bool((cnt == 1e-10).all())
    import rlhip

    with pytest.raises(RLHipArgumentError):  # the class surfaces the refusal
        rlhip.GumbelSoftmaxExplorer(seed=1).plan_(v)


# ---------------------------------------------------------------------------------------------- laws and independence
def law_kernel(c, step=None):
    import rlhip
    from rlhip import ops

    n = SC.LAW_N
    v = torch.as_tensor(SC.tile(c.column, n)).cuda()
    mc = getattr(c, "mask_column", None)
    m = None if mc is None else torch.as_tensor(SC.tile(mc, n)).cuda()
    step = c.step if step is None else step
    if c.entry == "categorical":
        return ops.categorical_sample(v, c.seed, step, c.env_id_base, m)[0].cpu().numpy()
    if c.entry == "eps_greedy":
        return ops.eps_greedy_select(v, c.eps, c.seed, step, c.env_id_base, m, c.is_break_tie).cpu().numpy()
    ex = getattr(rlhip, EXPLORER[c.entry])(seed=c.seed)
    ex.step, ex.is_normalized = step, c.is_normalized
    a = ex.plan_(v, env_id_base=c.env_id_base) if m is None else ex.plan_(v, m, env_id_base=c.env_id_base)
    return a.cpu().numpy() - 1


@pytest.mark.parametrize("c", SC.law_cases(), ids=lambda c: c.id)
def test_kernel_law(c):
    """chi^2 of one launch of 2^17 identical columns against select_ref.law; the counts equal the oracle's exactly.  For
    eps-greedy the expected vector is ALSO the output of rlhip_eps_greedy_prob_f32: the draw and prob() agree."""
    from rlhip import ops

    a = law_kernel(c)
    p = c.p
    if c.entry == "eps_greedy":
        m = None if c.mask_column is None else torch.as_tensor(c.mask_column[:, None]).cuda()
        pk = ops.eps_greedy_prob(torch.as_tensor(c.column[:, None]).cuda(), c.eps, m, c.is_break_tie).cpu().numpy()[:, 0]
        assert np.array_equal(pk, c.p)
        p = pk
    stat, dof, cnt = SC.chi2_counts(a, p, c.na)
    bar = SC.chi2_bar(dof)
    print(f"{c.id}: chi2 {stat:.2f} dof {dof} bar {bar:.2f}")
    assert stat < bar
    assert np.array_equal(cnt, SC.chi2_counts(SC.law_oracle(c), c.p, c.na)[2])


@pytest.mark.parametrize("c", SC.INDEPENDENCE, ids=lambda c: c.id)
def test_kernel_independence(c):
    a0, a1 = law_kernel(c), law_kernel(c, step=c.step + 1)
    r0, r1 = SC.law_oracle(c), SC.law_oracle(c, step=c.step + 1)
    for name, (x, y), (rx, ry) in (("steps", (a0, a1), (r0, r1)), ("neighbours", (a0[:-1], a0[1:]), (r0[:-1], r0[1:]))):
        stat, dof, tab = SC.chi2_independence(x, y)
        bar = SC.chi2_bar(dof)
        print(f"{c.id} {name}: chi2 {stat:.2f} dof {dof} bar {bar:.2f}")
        assert stat < bar
        assert np.array_equal(tab, SC.chi2_independence(rx, ry)[2])

"""The tail of the two-layer PPO optimiser step -- reduce_apply_kernel (csrc/ppo_grad.hip): row loop, norm exchange, Adam, the
patch of the unit-record image through record_slot32 -- at the shapes that exercise its row loop and its slot arithmetic.

Every case runs three consecutive update calls (the epoch word and the beta powers advance) of one epoch x two micro-batches and
compares `update_` (reduce_apply_kernel<APPLY_GRID>: rows summed, clipped and applied in one launch, the image patched word by
word) with the manual `grad_` / `apply_` sequence (reduce_apply_kernel<APPLY_NONE>, then apply_pack_kernel, which re-packs the
whole image from the parameters), bit for bit on params, m, v, beta_pow, grad and the losses; and the unit-record image after
the call with that fresh pack of the same parameters, bit for bit.

micro-batch -> partial rows nb: 64 -> 1 | 185 -> 3 (ragged last tile, most groups empty) | 960 -> 15 | 1024 -> 16 (one row per
group) | 1088 -> 17 | 2112 -> 33 | 16384 -> 256 (one team per workgroup) | 16448 -> 129 (two teams, odd) | 32768 -> 256 (two
teams: the headline's tail).  Crossed with hidden 8 / 64 / 256, the three nets (ns / nout = 4 / 2, 3 / 2, 2 / 3) and the clip
active (tiny max_grad_norm) and inactive.  (np = h (2 ns + 3 + nout) + nout + 1 is 13 h + 3, 11 h + 3, 10 h + 4 for the three
nets: with h a multiple of 8 never a multiple of 64, so the last workgroup always has lanes without a parameter.)

One more case runs the last-arriver variant (RLHIP_GRID_BARRIER_CAP=0, APPLY_LAST) in a fresh child process, and one the
captured-graph path."""
import hashlib
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_GRAD_BLOCKS, REC = 512, 16
NETS = {"cartpole": False, "pendulum": True, "mountaincar": False}  # kind -> continuous head: ns / nout = 4 / 2, 3 / 2, 2 / 3
NB_OF = {64: 1, 185: 3, 960: 15, 1024: 16, 1088: 17, 2112: 33, 16384: 256, 16448: 129, 32768: 256}
ARRAYS = ("params", "m", "v", "beta_pow", "grad", "losses")


def _nb(bm):  # prepare_grad: 64-sample tiles, two tiles per workgroup above 256 tiles
    tiles = (bm + 63) // 64
    return min(MAX_GRAD_BLOCKS, (tiles + 1) // 2 if tiles > 256 else tiles)


def _image(pol):
    """the unit-record image in the learner's workspace (the carve of prepare_grad / workspace_packed)"""
    base = pol.workspace.data_ptr()
    q = base + MAX_GRAD_BLOCKS * pol.np * 4 + MAX_GRAD_BLOCKS * 4 * 4
    q = (q + 15) & ~15
    q += 4096 * 8 + 16 * 4 + MAX_GRAD_BLOCKS * 8 * 8
    q = (q + 63) & ~63
    off = q - base
    return pol.workspace[off:off + (REC * pol.cfg.hidden + 4) * 4].view(torch.int32).clone()


def _pair(kind, bm, hidden, clip, seed=5):
    import rlhip

    pols = []
    for _ in range(2):
        env = rlhip.HipVecEnv(kind, bm, seed=seed, continuous=NETS[kind])
        kw = {"max_grad_norm": 1e-3} if clip else {"max_grad_norm": 1e9}
        pols.append(rlhip.PPOPolicy(env, update_freq=2, hidden=hidden, n_epochs=1, n_microbatches=2, **kw))
    return pols


def _manual_update(pol):
    pol.gae_()
    for e in range(pol.cfg.n_epochs):
        for mb in range(pol.cfg.n_microbatches):
            pol.grad_(pol.update_ctr * pol.cfg.n_epochs + e, mb)
            pol.apply_(1.0)
    pol.update_ctr += 1


def _bits(t):
    return t.view(torch.int32)


def _run_case(kind, bm, hidden, clip, calls=3):
    """-> sha256 over the six arrays and the image after every call (the same on every variant of the tail)"""
    a, b = _pair(kind, bm, hidden, clip)
    assert _nb(bm) == NB_OF[bm]
    h = hashlib.sha256()
    for call in range(calls):
        a.rollout_()
        b.rollout_()
        a.update_()
        _manual_update(b)
        for name in ARRAYS:
            x, y = _bits(getattr(a, name)), _bits(getattr(b, name))
            assert torch.equal(x, y), f"{name} differs from the manual sequence in call {call}: {int((x != y).sum())} words"
            h.update(x.cpu().numpy().tobytes())
        ia, ib = _image(a), _image(b)
        assert torch.equal(ia, ib), f"unit-record image differs from a fresh pack in call {call}: words {(ia != ib).nonzero().flatten()[:8].tolist()}"
        h.update(ia.cpu().numpy().tobytes())
    assert not torch.equal(a.m, torch.zeros_like(a.m)) and torch.isfinite(a.params).all()
    return h.hexdigest()


@pytest.mark.parametrize("clip", [False, True], ids=["noclip", "clip"])
@pytest.mark.parametrize("kind", list(NETS))
@pytest.mark.parametrize("hidden", [8, 64, 256])
@pytest.mark.parametrize("bm", list(NB_OF))
def test_update_equals_manual_sequence_and_patches_the_record_image(bm, hidden, kind, clip):
    _run_case(kind, bm, hidden, clip)


def test_last_arriver_variant_equals_the_grid_variant_and_the_manual_sequence():
    """RLHIP_GRID_BARRIER_CAP=0 in a fresh child process: update_ launches reduce_apply_kernel<APPLY_LAST> (same row loop, one
    workgroup applies Adam and re-packs): the child runs the same case -- against its own manual sequence -- and its digest
    equals the one of the grid variant here"""
    case = ("mountaincar", 1088, 64, True)
    src = ("import sys\n"
           "sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
           "import tests.test_gpu_ppo_tail_chain as t\n"
           "print('DIGEST', t._run_case(*%r))\n") % (ROOT, os.path.join(ROOT, "reinforcementlearning.jl_amd"), case)
    r = subprocess.run([sys.executable, "-c", src], env=dict(os.environ, RLHIP_GRID_BARRIER_CAP="0"), capture_output=True,
                       text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    digest = [ln for ln in r.stdout.splitlines() if ln.startswith("DIGEST")][0].split()[1]
    assert digest == _run_case(*case)


def test_captured_graph_replay_equals_eager_on_every_array_and_the_image():
    """the device-counter update captured in a HIP graph: three replays against three eager rollout_ + update_ calls"""
    import rlhip

    kind, bm, hidden = "mountaincar", 1088, 64
    pols = []
    for _ in range(2):
        env = rlhip.HipVecEnv(kind, bm, seed=5, continuous=NETS[kind])
        pols.append(rlhip.PPOPolicy(env, update_freq=2, hidden=hidden, n_epochs=1, n_microbatches=2, max_grad_norm=1e-3))
    a, c = pols
    for p in pols:  # one eager iteration first, so that the counters are non-zero at capture time
        p.rollout_()
        p.update_()
    c.capture_graph_(warmup=0)
    for it in range(3):
        a.rollout_()
        a.update_()
        c.replay_()
        torch.cuda.synchronize()
        for name in ARRAYS:
            assert torch.equal(_bits(getattr(a, name)), _bits(getattr(c, name))), f"{name} differs at replay {it}"
        assert torch.equal(_image(a), _image(c)), f"unit-record image differs at replay {it}"

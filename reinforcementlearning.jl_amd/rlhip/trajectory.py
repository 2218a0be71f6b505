"""Trajectory / CircularArraySARTSTraces / BatchSampler / InsertSampleRatioController -- host mirror of
the un-vendored ReinforcementLearningTrajectories 0.4 surface the reference re-exports
(src/ReinforcementLearningCore/src/ReinforcementLearningCore.jl:10), with the storage in HBM.

Constructor forms follow the in-tree call sites: RLCore/test/policies/q_based_policy.jl:41-47,
docs/src/How_to_implement_a_new_algorithm.md:90-112.  Push protocol: RLCore/src/policies/agent/agent_base.jl:45-59.
The ring arithmetic itself is ring.hip behind the C ABI; head/length counters are host integers.
"""
import ctypes as C

import torch

from . import _lib
from ._lib import call
from .ops import ptr, stream_ptr


class CircularArraySARTSTraces:
    """CircularArraySARTSTraces(; capacity, state = T => (obs_dim, n_env), action = Int => (n_env,),
    reward = Float32 => (n_env,), terminal = Bool => (n_env,)).  One frame = one vec-step.

    action_dtype = torch.float32 is `action = Float32 => (n_env,)`, the traces of a continuous env with one action component (SACPolicy):
    the action word of every transition holds the bits of a Float32 -- the push stores whatever 4-byte words it is handed -- and
    `.action` / `gather` hand them back as Float32, reinterpreted from the same bytes."""

    def __init__(self, capacity, n_env=1, obs_dim=1, dtype=torch.float32, device="cuda", action_dtype=torch.int32):
        if dtype not in (torch.float32, torch.uint8):
            raise TypeError("state eltype must be Float32 or UInt8")
        if action_dtype not in (torch.int32, torch.float32):
            raise TypeError("action eltype must be Int32 or Float32")
        self.action_dtype = action_dtype
        dev = torch.device(device)
        self.capacity, self.n_env, self.obs_dim, self.dtype = capacity, n_env, obs_dim, dtype
        # Float32 observations with <= 4 components live in a RECORD ring (csrc/ring_device.h, include/rlhip.h RLHIP_RING_RECORDS):
        # one 64-byte record {s[4], action, reward, terminal, spare, s_next[4], pad[4]} per (state slot, env) -- the whole
        # transition that LEAVES that state -- so that a sampled transition is ONE cache line.  `records` is the storage (and
        # what a checkpoint holds); `state` / `action` / `reward` / `terminal` / `next_state` are strided VIEWS of it, indexed
        # by the record's slot (capacity + 1 slots; the newest slot holds a state only).  Other rings (UInt8 frames, wider
        # observations) keep one tensor per trace, every frame as pushed.
        self.records_layout = dtype == torch.float32 and obs_dim <= 4
        self.rb = _lib.Ring()
        if self.records_layout:
            self.records = torch.zeros((capacity + 1, n_env, 16), dtype=torch.float32, device=dev)
            assert self.records.numel() * 4 == int(_lib.lib.rlhip_ring_state_bytes(capacity, n_env, obs_dim, 4))
            call("rlhip_ring_init", C.byref(self.rb), capacity, n_env, obs_dim, 4, ptr(self.records), None, None, None)
        else:
            self.state = torch.zeros((capacity + 1, obs_dim, n_env), dtype=dtype, device=dev)
            self.action = torch.zeros((capacity, n_env), dtype=action_dtype, device=dev)
            self.reward = torch.zeros((capacity, n_env), dtype=torch.float32, device=dev)
            self.terminal = torch.zeros((capacity, n_env), dtype=torch.uint8, device=dev)
            call("rlhip_ring_init", C.byref(self.rb), capacity, n_env, obs_dim, 4 if dtype == torch.float32 else 1,
                 ptr(self.state), ptr(self.action), ptr(self.reward), ptr(self.terminal))
        assert int(_lib.lib.rlhip_ring_layout(C.byref(self.rb))) == (2 if self.records_layout else 0)
        self.frame_major = bool(_lib.lib.rlhip_ring_gather_is_frame_major(C.byref(self.rb)))

    def __getattr__(self, name):
        # record rings only (frame rings own real tensors of these names): strided views of `records`
        if name in ("state", "action", "reward", "terminal", "next_state") and self.__dict__.get("records_layout"):
            rec = self.__dict__["records"]
            if name == "state":
                return rec[:, :, :self.obs_dim]          # (capacity + 1, n_env, obs_dim)
            if name == "next_state":
                return rec[:, :, 8:8 + self.obs_dim]     # s' of the transition that leaves the slot's state
            if name == "action":
                # (capacity + 1, n_env), by the slot of the transition's s; the same word as Int32 or as Float32
                return rec[:, :, 4] if self.__dict__.get("action_dtype") == torch.float32 else rec.view(torch.int32)[:, :, 4]
            if name == "reward":
                return rec[:, :, 5]
            return rec.view(torch.uint8)[:, :, 24]       # low byte of the terminal word (byte 24 of the 64-byte record)
        raise AttributeError(name)

    def push_state_(self, obs):
        """push!(traces, (state = s,))"""
        call("rlhip_ring_push_state", C.byref(self.rb), ptr(obs), stream_ptr())

    def push_transition_(self, next_obs, action0, reward, terminal):
        """push!(traces, (state = s', action = a, reward = r, terminal = t)); action0 is 0-based int32 (Float32 with
        action_dtype = torch.float32)."""
        if terminal.dtype == torch.bool:
            terminal = terminal.view(torch.uint8)
        if self.action_dtype == torch.float32 and action0.dtype != torch.float32:
            raise TypeError(f"these traces store Float32 actions, the push hands over {action0.dtype}")
        call("rlhip_ring_push_transition", C.byref(self.rb), ptr(next_obs), ptr(action0), ptr(reward),
             ptr(terminal), stream_ptr())

    def __len__(self):
        return int(_lib.lib.rlhip_ring_length(C.byref(self.rb)))

    def n_transitions(self):
        return len(self) * self.n_env

    def sample_indices(self, batch, seed, draw_ctr):
        idx = torch.empty(batch, dtype=torch.int64, device=self.state.device)
        call("rlhip_ring_sample_indices", C.byref(self.rb), batch, seed, draw_ctr, ptr(idx), stream_ptr())
        return idx

    def check_indices(self, idx):
        """(number of flat logical indices outside [0, length * n_env), position of the first one or -1): the debugging aid behind the
        bounds-checked build (rlhip_ring_check_indices; one launch + a stream synchronisation)."""
        n_bad, first = C.c_int64(0), C.c_int64(-1)
        call("rlhip_ring_check_indices", C.byref(self.rb), ptr(idx), idx.numel(), C.byref(n_bad), C.byref(first), stream_ptr())
        return int(n_bad.value), int(first.value)

    def gather(self, idx):
        """traces[inds] -> (state, action0, reward, terminal, next_state)."""
        b = idx.numel()
        dev = self.state.device
        shape = (b, self.obs_dim) if self.frame_major else (self.obs_dim, b)
        s = torch.empty(shape, dtype=self.dtype, device=dev)
        sn = torch.empty(shape, dtype=self.dtype, device=dev)
        a = torch.empty(b, dtype=torch.int32, device=dev)
        r = torch.empty(b, dtype=torch.float32, device=dev)
        t = torch.empty(b, dtype=torch.uint8, device=dev)
        call("rlhip_ring_gather", C.byref(self.rb), ptr(idx), b, ptr(s), ptr(a), ptr(r), ptr(t), ptr(sn),
             stream_ptr())
        return s, a.view(self.action_dtype), r, t, sn


def _gather_stacked(self, idx, n_stack):
    """traces[inds] with StackFrames applied at sample time (single-env rings of single frames):
    -> (state (b, n_stack, obs_dim), action0, reward, terminal, next_state), stacks oldest-first."""
    b, dev = idx.numel(), self.state.device
    s = torch.empty((b, n_stack, self.obs_dim), dtype=self.dtype, device=dev)
    sn = torch.empty((b, n_stack, self.obs_dim), dtype=self.dtype, device=dev)
    a = torch.empty(b, dtype=torch.int32, device=dev)
    r = torch.empty(b, dtype=torch.float32, device=dev)
    t = torch.empty(b, dtype=torch.uint8, device=dev)
    call("rlhip_ring_gather_stacked", C.byref(self.rb), ptr(idx), b, n_stack, ptr(s), ptr(a), ptr(r), ptr(t), ptr(sn),
         stream_ptr())
    return s, a, r, t, sn


def _nstep_outputs(self, b, shape):
    dev = self.state.device
    return (torch.empty(shape, dtype=self.dtype, device=dev), torch.empty(b, dtype=torch.int32, device=dev),
            torch.empty(b, dtype=torch.float32, device=dev), torch.empty(b, dtype=torch.uint8, device=dev),
            torch.empty(shape, dtype=self.dtype, device=dev), torch.empty(b, dtype=torch.int32, device=dev))


def _gather_nstep(self, idx, n_step, gamma):
    """n-step transitions of a FRAME ring (rlhip_ring_gather_nstep, one launch): for every flat logical start index the window
    li .. li + ns - 1 (cut at its first terminal step and at the newest stored transition)
    -> (state li, action0 li, discount_rewards_reduced(rewards[window], gamma), terminal of the last step, state li + ns, ns),
    states laid out as `gather` lays them out.  Record rings fold their windows instead (NStepBatchSampler.fold)."""
    b = idx.numel()
    s, a, ret, t, sn, n_used = _nstep_outputs(self, b, (b, self.obs_dim) if self.frame_major else (self.obs_dim, b))
    call("rlhip_ring_gather_nstep", C.byref(self.rb), ptr(idx), b, n_step, gamma, ptr(s), ptr(a), ptr(ret), ptr(t), ptr(sn),
         ptr(n_used), stream_ptr())
    return s, a, ret, t, sn, n_used


def _gather_stacked_nstep(self, idx, n_stack, n_step, gamma):
    """`gather_nstep` with StackFrames applied at sample time (rlhip_ring_gather_stacked_nstep): state = the stack that ends at
    frame li, next_state = the stack that ends at frame li + ns, both (b, n_stack, obs_dim), oldest first"""
    b = idx.numel()
    s, a, ret, t, sn, n_used = _nstep_outputs(self, b, (b, n_stack, self.obs_dim))
    call("rlhip_ring_gather_stacked_nstep", C.byref(self.rb), ptr(idx), b, n_stack, n_step, gamma, ptr(s), ptr(a), ptr(ret), ptr(t),
         ptr(sn), ptr(n_used), stream_ptr())
    return s, a, ret, t, sn, n_used


def _push_state_maxpool_(self, screen1, screen2):
    """push!(traces, (state = max.(screen1, screen2),)) -- AtariEnv's 2-frame max-pool fused into the push"""
    call("rlhip_ring_push_state_maxpool", C.byref(self.rb), ptr(screen1), ptr(screen2), stream_ptr())


def _push_transition_maxpool_(self, screen1, screen2, action0, reward, terminal):
    if terminal.dtype == torch.bool:
        terminal = terminal.view(torch.uint8)
    call("rlhip_ring_push_transition_maxpool", C.byref(self.rb), ptr(screen1), ptr(screen2), ptr(action0),
         ptr(reward), ptr(terminal), stream_ptr())


CircularArraySARTSTraces.gather_stacked = _gather_stacked
CircularArraySARTSTraces.gather_nstep = _gather_nstep
CircularArraySARTSTraces.gather_stacked_nstep = _gather_stacked_nstep
CircularArraySARTSTraces.push_state_maxpool_ = _push_state_maxpool_
CircularArraySARTSTraces.push_transition_maxpool_ = _push_transition_maxpool_


class CircularPrioritizedTraces(CircularArraySARTSTraces):
    """CircularPrioritizedTraces(CircularArraySARTSTraces(...); default_priority): every pushed transition
    enters the device sum-tree with `default_priority`; `traces.set_priority_(keys, p)` is
    `trajectory[:priority, keys] = p` (un-vendored RLTrajectories 0.4; sumtree.hip).

    n_step > 1 (record rings): the traces serve an NStepBatchSampler(n_step, ...).  The validity mask of RLTrajectories'
    `sample(::NStepBatchSampler, ::CircularPrioritizedTraces)` is kept in the tree (rlhip_ring_push_priority_nstep, csrc/per_nstep.hip):
    the newest n_step - 1 frames stay at priority 0 and a frame receives `default_priority` once n_step transitions lie at or after
    it, so every draw is a window start with its n transitions ahead.  Write priorities back (`set_priority_`) under keys drawn since
    the last push.  n_step = 1, the default, is the plain push.  Frame rings with n_step > 1: CircularPrioritizedFrameTraces."""

    def __init__(self, capacity, n_env=1, obs_dim=1, dtype=torch.float32, default_priority=100.0, device="cuda", n_step=1):
        self._check_n_step(n_step, capacity, dtype == torch.float32 and obs_dim <= 4)  # before anything is allocated
        super().__init__(capacity, n_env, obs_dim, dtype, device)
        self.n_step = int(n_step)
        self.default_priority = float(default_priority)
        if not self.default_priority > 0.0:  # a tree without mass cannot be sampled (the draw would land on an empty slot)
            raise ValueError("default_priority must be > 0")
        self.n_leaves = capacity * n_env
        nodes = int(_lib.lib.rlhip_sumtree_nodes(self.n_leaves))
        self.priorities = torch.zeros(nodes, dtype=torch.float32, device=self.state.device)  # zero-init contract

    @staticmethod
    def _check_n_step(n_step, capacity, records_layout):
        if isinstance(n_step, bool) or int(n_step) != n_step or not 1 <= int(n_step) <= 32:
            raise ValueError("n_step must be an integer in 1..32")
        if int(n_step) > 1 and not records_layout:
            raise ValueError("n_step > 1 needs a record ring (Float32 observations, obs_dim <= 4)")
        if int(n_step) > capacity:
            raise ValueError("n_step exceeds the capacity: no window would ever be complete")

    def __setattr__(self, name, value):
        # every assignment of the mask width is checked against the ring -- rlhip/checkpoint.py restores fields with setattr, so a
        # checkpoint whose n_step these traces cannot serve is refused when it is loaded, not at the next push
        if name == "n_step":
            self._check_n_step(value, self.capacity, self.records_layout)
            value = int(value)
        super().__setattr__(name, value)

    def push_transition_(self, next_obs, action0, reward, terminal):
        super().push_transition_(next_obs, action0, reward, terminal)
        if self.n_step == 1:
            call("rlhip_ring_push_priority", C.byref(self.rb), ptr(self.priorities), self.default_priority, stream_ptr())
        else:  # the newest frame := 0, the frame with n_step transitions at or after it := default_priority
            call("rlhip_ring_push_priority_nstep", C.byref(self.rb), ptr(self.priorities), self.default_priority, self.n_step,
                 stream_ptr())

    def sample_prioritized(self, batch, seed, draw_ctr):
        """-> (logical flat indices for gather, physical keys, priorities)"""
        dev = self.state.device
        idx = torch.empty(batch, dtype=torch.int64, device=dev)
        key = torch.empty(batch, dtype=torch.int64, device=dev)
        prio = torch.empty(batch, dtype=torch.float32, device=dev)
        call("rlhip_ring_sample_prioritized", C.byref(self.rb), ptr(self.priorities), batch, seed, draw_ctr,
             ptr(idx), ptr(key), ptr(prio), stream_ptr())
        return idx, key, prio

    def sample_gather_prioritized(self, batch, seed, draw_ctr):
        """the prioritized draw and the gather of its batch in ONE launch (bit-identical to sample_prioritized + gather)
        -> (idx, key, priority), (state, action0, reward, terminal, next_state)"""
        dev = self.state.device
        idx = torch.empty(batch, dtype=torch.int64, device=dev)
        key = torch.empty(batch, dtype=torch.int64, device=dev)
        prio = torch.empty(batch, dtype=torch.float32, device=dev)
        shape = (batch, self.obs_dim) if self.frame_major else (self.obs_dim, batch)
        s = torch.empty(shape, dtype=self.dtype, device=dev)
        sn = torch.empty(shape, dtype=self.dtype, device=dev)
        a = torch.empty(batch, dtype=torch.int32, device=dev)
        r = torch.empty(batch, dtype=torch.float32, device=dev)
        t = torch.empty(batch, dtype=torch.uint8, device=dev)
        call("rlhip_ring_sample_gather_prioritized", C.byref(self.rb), ptr(self.priorities), batch, seed, draw_ctr, ptr(idx),
             ptr(key), ptr(prio), ptr(s), ptr(a), ptr(r), ptr(t), ptr(sn), stream_ptr())
        return (idx, key, prio), (s, a, r, t, sn)

    def update_sample_gather_prioritized(self, upd_keys, upd_prio, batch, seed, draw_ctr):
        """`trajectory[:priority, upd_keys] = upd_prio`, then the prioritized draw and the gather of its batch -- ONE launch for
        <= 64 keys on a frame-major ring (bit-identical to set_priority_ + sample_gather_prioritized, which is what runs otherwise)
        -> (idx, key, priority), (state, action0, reward, terminal, next_state)"""
        dev = self.state.device
        if not hasattr(self, "_sync"):
            self._sync = torch.zeros(2, dtype=torch.int32, device=dev)  # zero before the first call; every call re-arms it
        n_upd = 0 if upd_keys is None else upd_keys.numel()
        if n_upd and (upd_keys.dtype != torch.int64 or upd_prio.dtype != torch.float32 or upd_prio.numel() != n_upd):
            raise TypeError("keys must be int64 and priorities float32 of the same length")
        idx = torch.empty(batch, dtype=torch.int64, device=dev)
        key = torch.empty(batch, dtype=torch.int64, device=dev)
        prio = torch.empty(batch, dtype=torch.float32, device=dev)
        shape = (batch, self.obs_dim) if self.frame_major else (self.obs_dim, batch)
        s = torch.empty(shape, dtype=self.dtype, device=dev)
        sn = torch.empty(shape, dtype=self.dtype, device=dev)
        a = torch.empty(batch, dtype=torch.int32, device=dev)
        r = torch.empty(batch, dtype=torch.float32, device=dev)
        t = torch.empty(batch, dtype=torch.uint8, device=dev)
        call("rlhip_ring_update_sample_gather_prioritized", C.byref(self.rb), ptr(self.priorities), ptr(upd_keys) if n_upd else None,
             ptr(upd_prio) if n_upd else None, n_upd, batch, seed, draw_ctr, ptr(idx), ptr(key), ptr(prio), ptr(s), ptr(a), ptr(r), ptr(t),
             ptr(sn), ptr(self._sync), stream_ptr())
        return (idx, key, prio), (s, a, r, t, sn)

    def set_priority_(self, keys, prio):
        """trajectory[:priority, keys] = prio  (sequential semantics: the last duplicate key wins)"""
        if keys.dtype != torch.int64 or prio.dtype != torch.float32:
            raise TypeError("keys must be int64 and priorities float32")
        if keys.numel() != prio.numel():
            raise ValueError("keys and priorities differ in length")
        call("rlhip_sumtree_update", ptr(self.priorities), self.n_leaves, ptr(keys), ptr(prio), keys.numel(),
             stream_ptr())

    def total_priority(self):
        return float(self.priorities[1])


class CircularPrioritizedFrameTraces(CircularPrioritizedTraces):
    """CircularPrioritizedTraces over a FRAME ring (UInt8 images, Float32 observations with more than four components) that serve an
    NStepBatchSampler(n_step, ...), n_step in 1..32: the validity mask is kept in the tree by rlhip_ring_push_priority_nstep_frames
    (the rule of the record rings' push, csrc/per_nstep.hip), and `sample_gather_nstep_prioritized` is the prioritized draw and the
    n-step gather of its batch in ONE launch (csrc/per_frames_nstep.hip) -- with `n_stack` the stack-at-sample form, the sampler of a
    Rainbow-style Atari agent.  Record-layout observations (Float32, obs_dim <= 4) are refused: CircularPrioritizedTraces serves them."""

    @staticmethod
    def _check_n_step(n_step, capacity, records_layout):
        if isinstance(n_step, bool) or int(n_step) != n_step or not 1 <= int(n_step) <= 32:
            raise ValueError("n_step must be an integer in 1..32")
        if records_layout:
            raise ValueError("CircularPrioritizedFrameTraces needs a frame layout (UInt8, or Float32 with obs_dim > 4); a record ring "
                             "takes CircularPrioritizedTraces(..., n_step = n_step)")
        if int(n_step) > capacity:
            raise ValueError("n_step exceeds the capacity: no window would ever be complete")

    def push_transition_(self, next_obs, action0, reward, terminal):
        CircularArraySARTSTraces.push_transition_(self, next_obs, action0, reward, terminal)
        # the newest frame := 0, the frame with n_step transitions at or after it := default_priority (n_step = 1: the plain push's tree)
        call("rlhip_ring_push_priority_nstep_frames", C.byref(self.rb), ptr(self.priorities), self.default_priority, self.n_step,
             stream_ptr())

    def sample_gather_nstep_prioritized(self, batch, n, gamma, seed, draw_ctr, n_stack=None):
        """the prioritized draw and the n-step gather of its batch in ONE launch (bit-identical to sample_prioritized + gather_nstep,
        with `n_stack` + gather_stacked_nstep) -> (idx, key, priority), (state, action0, return, terminal, next_state, n_used).
        `n` is the window the gather folds; on a tree masked for n_step = n every window is complete"""
        dev = self.state.device
        idx = torch.empty(batch, dtype=torch.int64, device=dev)
        key = torch.empty(batch, dtype=torch.int64, device=dev)
        prio = torch.empty(batch, dtype=torch.float32, device=dev)
        if n_stack is None:
            s, a, ret, t, sn, n_used = _nstep_outputs(self, batch, (batch, self.obs_dim) if self.frame_major else (self.obs_dim, batch))
            call("rlhip_ring_sample_gather_nstep_prioritized", C.byref(self.rb), ptr(self.priorities), batch, n, gamma, seed, draw_ctr,
                 ptr(idx), ptr(key), ptr(prio), ptr(s), ptr(a), ptr(ret), ptr(t), ptr(sn), ptr(n_used), stream_ptr())
        else:
            s, a, ret, t, sn, n_used = _nstep_outputs(self, batch, (batch, n_stack, self.obs_dim))
            call("rlhip_ring_sample_gather_stacked_nstep_prioritized", C.byref(self.rb), ptr(self.priorities), batch, n_stack, n, gamma,
                 seed, draw_ctr, ptr(idx), ptr(key), ptr(prio), ptr(s), ptr(a), ptr(ret), ptr(t), ptr(sn), ptr(n_used), stream_ptr())
        return (idx, key, prio), (s, a, ret, t, sn, n_used)


class BatchSampler:
    """BatchSampler(batchsize; rng): uniform indices with replacement (Philox SAMPLER stream); over
    CircularPrioritizedTraces: `inds, priorities = rand(rng, sumtree, batchsize)` and the batch also carries
    `key` (for the priority write-back) and `priority`."""

    def __init__(self, batchsize, seed=0):
        self.batchsize, self.seed, self.draw_ctr = batchsize, seed, 0

    def sample(self, traces):
        extra = {}
        if isinstance(traces, CircularPrioritizedTraces):
            (idx, key, prio), (s, a, r, t, sn) = traces.sample_gather_prioritized(self.batchsize, self.seed, self.draw_ctr)
            self.draw_ctr += 1
            return dict(state=s, action=a + 1, reward=r, terminal=t.view(torch.bool), next_state=sn, key=key, priority=prio)
        else:
            idx = traces.sample_indices(self.batchsize, self.seed, self.draw_ctr)
            extra = dict(key=idx)
        self.draw_ctr += 1
        s, a, r, t, sn = traces.gather(idx)
        return dict(state=s, action=a + 1, reward=r, terminal=t.view(torch.bool), next_state=sn, **extra)


def folded_scratch(owner, traces, b):
    """-> (`owner._folded`, `owner._iota`): the record ring of capacity 1 x `b` envs that holds a folded batch of `traces` and its
    index vector, made anew when the batch size or the observation width changes"""
    if owner._folded is None or owner._folded.n_env != b or owner._folded.obs_dim != traces.obs_dim:
        device = traces.state.device  # (a view of the records: only looked up when something is allocated)
        owner._folded = CircularArraySARTSTraces(capacity=1, n_env=b, obs_dim=traces.obs_dim, device=device)
        owner._iota = torch.empty(b, dtype=torch.int64, device=device)
    return owner._folded, owner._iota


class NStepBatchSampler:
    """NStepBatchSampler(n, gamma, batchsize; rng) of RLTrajectories 0.4 (un-vendored; oracle/rlo_buffer.c restates it): start
    indices with n transitions ahead of them, each window folded on the device into ONE transition
    (s_i, a_i, R = discount_rewards_reduced(r_i .. r_{i+ns-1}, gamma), any(terminal), s_{i+ns}) -- ns = n unless a terminal flag
    ends the window earlier.  `sample` returns the batch dictionary of BatchSampler; `fold` returns the folded record ring +
    indices the DQN gradient entry points take unchanged (with gamma^n = `gamma_n` as their discount): record rings.
    On a FRAME ring (UInt8 images, wider Float32 observations) `sample` gathers the n-step transitions in one launch
    (`traces.gather_nstep`; with `n_stack = k` the stack-at-sample form `traces.gather_stacked_nstep`) and the batch also carries
    `n_steps`, the transitions each window used: the discount of sample b's target is gamma ** n_steps[b].
    Over CircularPrioritizedTraces(n_step = n) the starts are drawn in proportion to the masked priorities and the batch also carries
    `key` and `priority`, as BatchSampler's does; traces built for another n_step are a ValueError.  Over
    CircularPrioritizedFrameTraces(n_step = n) -- prioritized frame rings -- `sample` is the draw and the (stacked) n-step gather in
    one launch, the same dictionary bit for bit as `sample_indices` followed by `gather_nstep` / `gather_stacked_nstep`."""

    def __init__(self, n, gamma, batchsize, seed=0, n_stack=None):
        if not 1 <= int(n) <= 32:
            raise ValueError("n must be in 1..32")
        if n_stack is not None and not 1 <= int(n_stack) <= 8:
            raise ValueError("n_stack must be in 1..8")
        self.n_stack = None if n_stack is None else int(n_stack)
        self.n, self.gamma, self.batchsize, self.seed, self.draw_ctr = int(n), float(gamma), int(batchsize), seed, 0
        self.gamma_n = float(_lib.lib.rlhip_gamma_pow(self.gamma, self.n))
        self._folded = None
        self.key = self.priority = self._draw = None  # prioritized traces: keys / priorities of the last draw (+ the fused call's buffers)

    def _prioritized(self, traces):
        if not isinstance(traces, CircularPrioritizedTraces):
            return False
        if traces.n_step != self.n:
            raise ValueError(f"the traces mask windows of n_step = {traces.n_step}, the sampler folds n = {self.n}: "
                             "construct CircularPrioritizedTraces(..., n_step = n)")
        return True

    def sample_indices(self, traces, draw_ctr=None):
        """window starts: uniform over 1:(length - n + 1) per env; over CircularPrioritizedTraces(n_step = n) in proportion to the
        masked priorities (the shipped prioritized draw), with `.key` / `.priority` of the draw kept on the sampler"""
        ctr = self.draw_ctr if draw_ctr is None else draw_ctr
        if self._prioritized(traces):
            if len(traces) < self.n:
                raise _lib.RLHipArgumentError("the trajectory holds fewer than n transitions: the masked tree has no mass")
            idx, self.key, self.priority = traces.sample_prioritized(self.batchsize, self.seed, ctr)
            return idx
        idx = torch.empty(self.batchsize, dtype=torch.int64, device=traces.state.device)
        call("rlhip_ring_sample_indices_nstep", C.byref(traces.rb), self.batchsize, self.n, self.seed, ctr, ptr(idx), stream_ptr())
        return idx

    def sample_fold_prioritized(self, traces, draw_ctr=None):
        """the prioritized draw and the window fold in ONE launch (rlhip_per_sample_fold_nstep_f32; byte for byte sample_indices + fold)
        -> (folded traces, iota, idx, key, priority)"""
        if not self._prioritized(traces):
            raise TypeError("sample_fold_prioritized takes CircularPrioritizedTraces(n_step = n)")
        ctr = self.draw_ctr if draw_ctr is None else draw_ctr
        b, dev = self.batchsize, traces.state.device
        folded, iota = folded_scratch(self, traces, b)
        if self._draw is None or self._draw[0].numel() != b or self._draw[0].device != dev:
            self._draw = (torch.empty(b, dtype=torch.int64, device=dev), torch.empty(b, dtype=torch.int64, device=dev),
                          torch.empty(b, dtype=torch.float32, device=dev))
        idx, self.key, self.priority = self._draw
        call("rlhip_per_sample_fold_nstep_f32", C.byref(traces.rb), ptr(traces.priorities), b, self.n, self.gamma, self.seed, ctr,
             ptr(idx), ptr(self.key), ptr(self.priority), C.byref(folded.rb), ptr(iota), stream_ptr())
        return folded, iota, idx, self.key, self.priority

    def fold(self, traces, idx=None):
        """-> (folded traces: a CircularArraySARTSTraces of capacity 1 x batchsize envs holding the n-step transitions, iota)"""
        if idx is None:
            if self._prioritized(traces):
                folded, iota = self.sample_fold_prioritized(traces)[:2]
                self.draw_ctr += 1
                return folded, iota
            idx = self.sample_indices(traces)
            self.draw_ctr += 1
        b = idx.numel()
        folded, iota = folded_scratch(self, traces, b)
        call("rlhip_ring_fold_nstep", C.byref(traces.rb), ptr(idx), b, self.n, self.gamma, C.byref(folded.rb), ptr(iota), stream_ptr())
        return folded, iota

    def _sample_frames(self, traces):
        if isinstance(traces, CircularPrioritizedFrameTraces) and self._prioritized(traces):  # draw + gather: one launch
            if len(traces) < self.n:
                raise _lib.RLHipArgumentError("the trajectory holds fewer than n transitions: the masked tree has no mass")
            (idx, self.key, self.priority), (s, a, ret, t, sn, n_used) = traces.sample_gather_nstep_prioritized(
                self.batchsize, self.n, self.gamma, self.seed, self.draw_ctr, self.n_stack)
            self.draw_ctr += 1
            return dict(state=s, action=a + 1, reward=ret, terminal=t.view(torch.bool), next_state=sn, n_steps=n_used, key=self.key,
                        priority=self.priority)
        idx = self.sample_indices(traces)
        self.draw_ctr += 1
        if self.n_stack is None:
            s, a, ret, t, sn, n_used = traces.gather_nstep(idx, self.n, self.gamma)
        else:
            s, a, ret, t, sn, n_used = traces.gather_stacked_nstep(idx, self.n_stack, self.n, self.gamma)
        extra = dict(key=self.key, priority=self.priority) if self._prioritized(traces) else dict(key=idx)
        return dict(state=s, action=a + 1, reward=ret, terminal=t.view(torch.bool), next_state=sn, n_steps=n_used, **extra)

    def sample(self, traces):
        if not traces.records_layout:
            return self._sample_frames(traces)
        if self.n_stack is not None:
            raise ValueError("n_stack selects the stack-at-sample gather of a frame ring; these traces are a record ring")
        folded, iota = self.fold(traces)
        s, a, r, t, sn = folded.gather(iota)
        extra = dict(key=self.key, priority=self.priority) if self._prioritized(traces) else {}
        return dict(state=s, action=a + 1, reward=r, terminal=t.view(torch.bool), next_state=sn, **extra)


class DoubleTargetFold:
    """Double DQN targets as a device fold (rlhip_dqn_fold_double_f32 / rlhip_dqn3_fold_double_f32, include/rlhip.h): every sampled
    record {s, a, r, t, s'} becomes {s, a, y = r + gamma_eff (1 - t) Qt(s')[findmax(Q(s'))], terminal = 1, s'} in a batch-sized
    record ring, on which every DQN gradient entry point computes the Double DQN update unchanged (its target line gives y + 0).
    Owns the folded ring, the iota and the workspace, as NStepBatchSampler owns its own.  `fold(ring, None, ..., in_place=True)`
    rewrites an already folded ring (the n-step form, gamma_eff = gamma^n) record by record: it takes no indices, because any
    order but 0, 1, .., n_env - 1 would have workgroups read records that others are rewriting."""

    checkpoint_scratch = True  # rlhip/checkpoint.py: the folded ring is rewritten by every fold, a checkpoint does not hold it

    def __init__(self):
        self._folded = self._iota = self._own_iota = self._ws = None
        self._ws_key = None

    def own_iota(self, b, device):
        """0, 1, .., b - 1: the index vector of the in-place fold"""
        if self._own_iota is None or self._own_iota.numel() != b or self._own_iota.device != device:
            self._own_iota = torch.arange(b, dtype=torch.int64, device=device)
        return self._own_iota

    def workspace(self, network, b, device):
        """the fold kernels' workspace for `network` at batch `b` (None where they need none), sized when either changes"""
        key = (network.n_in, network.hidden, network.n_out, b, network.layers)
        if self._ws_key != key:
            nbytes = int(_lib.lib.rlhip_dqn_double_workspace_bytes(*key))
            if nbytes < 0:
                raise ValueError("rlhip_dqn_double_workspace_bytes: bad network / batch description")
            self._ws, self._ws_key = (torch.empty(nbytes, dtype=torch.uint8, device=device) if nbytes else None), key
        return self._ws

    def fold(self, traces, idx, network, target, target_packed, gamma_eff, in_place=False):
        """-> (folded traces, iota); `network` is a HipApproximator (2 or 3 layers), `target` / `target_packed` its target copy"""
        if in_place:
            if idx is not None:
                raise ValueError("the in-place fold walks the ring's own records 0 .. n_env - 1: pass idx = None")
            b, dev = traces.n_env, traces.state.device
            folded = traces
            idx = iota = self.own_iota(b, dev)
        else:
            b, dev = idx.numel(), idx.device
            folded, iota = folded_scratch(self, traces, b)  # allocated on the traces' device: the one `idx` was drawn on
        ws = ptr(self.workspace(network, b, dev))
        if network.layers == 3:
            call("rlhip_dqn3_fold_double_f32", C.byref(traces.rb), network.hidden, network.n_out, network.act, ptr(network.params),
                 ptr(network.packed), ptr(target), ptr(target_packed), ptr(idx), b, gamma_eff, C.byref(folded.rb), ptr(iota), ws,
                 stream_ptr())
        else:
            call("rlhip_dqn_fold_double_f32", C.byref(traces.rb), network.hidden, network.n_out, network.act, ptr(network.params),
                 ptr(target), ptr(idx), b, gamma_eff, C.byref(folded.rb), ptr(iota), ws, stream_ptr())
        return folded, iota


class InsertSampleRatioController:
    """InsertSampleRatioController(ratio, threshold; n_inserted = 0, n_sampled = 0): sampling is allowed
    once n_inserted >= threshold and while n_sampled <= (n_inserted - threshold) * ratio
    (docs/src/How_to_implement_a_new_algorithm.md:108)."""

    def __init__(self, ratio=1.0, threshold=1, n_inserted=0, n_sampled=0):
        self.ratio, self.threshold, self.n_inserted, self.n_sampled = ratio, threshold, n_inserted, n_sampled

    def on_insert_(self, n=1):
        self.n_inserted += n

    def on_sample_(self):
        if self.n_inserted >= self.threshold and self.n_sampled <= (self.n_inserted - self.threshold) * self.ratio:
            self.n_sampled += 1
            return True
        return False


class Trajectory:
    """Trajectory(container, sampler, controller): `push_` inserts, iteration yields sampled batches while
    the controller allows (the `for batch in trajectory` protocol, RLCore/src/policies/learners/td_learner.jl:85-92)."""

    def __init__(self, container, sampler=None, controller=None):
        self.container = container
        self.sampler = sampler or BatchSampler(32)
        self.controller = controller or InsertSampleRatioController()

    def push_state_(self, obs):
        self.container.push_state_(obs)

    def push_transition_(self, next_obs, action0, reward, terminal):
        self.container.push_transition_(next_obs, action0, reward, terminal)
        self.controller.on_insert_(1)

    def __len__(self):
        return len(self.container)

    def __iter__(self):
        while len(self.container) > 0 and self.controller.on_sample_():
            yield self.sampler.sample(self.container)

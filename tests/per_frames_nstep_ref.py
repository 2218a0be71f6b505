"""Prioritized n-step replay on FRAME rings stated on the list model of tests/ring_nstep_ref.py, plus the leaves of the masked sum-tree
stated on the same lists (no head / length / modulo arithmetic of the ring: a key is `(k mod capacity) * n_env + e` for the k-th pushed
transition, and a drawn key finds its transition by looking through the stored ones):

  * the k-th pushed transition (k from 0) of env e owns key (k mod capacity) * n_env + e;
  * after push k that key is 0 when n > 1 (no complete window starts at the newest transition; after a wrap the slot still carried the
    overwritten transition's priority);
  * after push k the key of push k - n + 1, if that push exists, is `priority` (n transitions lie at or after it from now on).

The gather's judge is RingNStepRef, the draw's judge oracle.SumTree (fill_range / update / sample) on those leaves.
Shared by tests/test_per_frames_nstep_reference.py (CPU) and tests/test_gpu_per_frames_nstep.py, which walk the SAME plan of trees and
draws (`trees`, `draws`), so that what the census says about a case on the CPU is what the device test draws."""
import numpy as np

import oracle
import ring_nstep_ref as R

# (dtype, obs_dim, n_env, capacity, frame_major): the routes of rlhip_ring_sample_gather_nstep_prioritized
PLAIN_CASES = [
    ("f32", 6, 5, 7, False),      # small route
    ("f32", 5, 300, 3, False),    # batch 301 crosses the 256-sample tile
    ("u8", 1030, 1, 4, False),    # small route, not a multiple of 16 bytes
    ("u8", 1024, 1, 6, True),     # frame-major
    ("u8", 7056, 1, 6, True),     # frame-major, 441 chunks: a partial trip
]
STACKED_CASES = [("u8", 48, 12), ("u8", 7056, 12)]  # (dtype, obs_dim, capacity), n_env = 1
STACKS = (1, 4, 8)
PRIORITY = 2.5
CTR_MAX = 2 ** 32 - 1
SEED = 11  # the sampler seed of every draw


def masked_nsteps(cap):
    return sorted({1, 2, 3, cap})


def unmasked_nsteps(cap):
    return sorted({2, 3, cap, 32})


def draws(n_env):
    """(batch, gamma, draw_ctr) of every draw made on one tree: batch 1, 64 and one beyond a 256-sample tile, both ends of the counter,
    both discounts"""
    return ((1, 0.99, 0), (64, 0.99, CTR_MAX), (301 if n_env == 300 else 257, 0.99, 0), (64, 0.0, 1))


class PrioritizedFramesRef(R.RingNStepRef):
    """the list model of the ring with the leaves of a tree masked for windows of n transitions"""

    def __init__(self, capacity, n_env, obs_dim, dtype, n, priority=PRIORITY):
        super().__init__(capacity, n_env, obs_dim, dtype)
        self.n, self.priority = int(n), float(priority)
        self.st = oracle.SumTree(self.capacity * self.n_env)

    def key(self, k, e=0):
        return (k % self.capacity) * self.n_env + e

    def push_transition(self, next_obs, a, r, t):
        super().push_transition(next_obs, a, r, t)
        k = self.pushed_transitions - 1
        if self.n > 1:
            self.st.fill_range(self.key(k), self.n_env, 0.0)
        if k - self.n + 1 >= 0:
            self.st.fill_range(self.key(k - self.n + 1), self.n_env, self.priority)

    def stored(self):
        """pushed transition numbers still in the ring, oldest first: logical index li is position li of this list"""
        return list(range(self.pushed_transitions - len(self), self.pushed_transitions))

    def start_of_key(self, key):
        """-> (li, e) of the stored transition that owns the key"""
        slot, e = divmod(int(key), self.n_env)
        hits = [li for li, k in enumerate(self.stored()) if k % self.capacity == slot]
        assert len(hits) == 1, f"key {key} belongs to no stored transition"
        return hits[0], e

    def complete_starts(self):
        """keys of the stored starts that have n transitions at or after them"""
        ks = self.stored()
        return {self.key(k, e) for li, k in enumerate(ks) if li + self.n <= len(ks) for e in range(self.n_env)}

    def has_mass(self):
        return bool(self.st.tree[1] > 0)

    def draw(self, batch, seed, draw_ctr):
        """-> (flat logical indices, keys, priorities): oracle.SumTree.sample, each key mapped through the lists"""
        key, prio = self.st.sample(batch, seed, draw_ctr)
        idx = np.array([li * self.n_env + e for li, e in map(self.start_of_key, key.tolist())], np.int64)
        return idx, key, prio


# last word of the content seed per case ((obs_dim, n_env, capacity) / (obs_dim, capacity)), the smallest under which the census of
# tests/test_per_frames_nstep_reference.py holds for the draws of `draws` (a single-env ring of capacity 4 holds few windows); others 0
PLAIN_SALT = {(1030, 1, 4): 2}
STACKED_SALT = {(48, 12): 9}


def plain_ref(case, pushes, n, sink=None):
    dtype, od, n_env, cap, _ = case
    rng = np.random.default_rng([od, n_env, cap, pushes, PLAIN_SALT.get((od, n_env, cap), 0)])
    ref = PrioritizedFramesRef(cap, n_env, od, np.uint8 if dtype == "u8" else np.float32, n)
    return R.fill(ref, rng, dtype, pushes, 0.25, sink)


def stacked_ref(case, pushes, n, sink=None):
    dtype, od, cap = case
    rng = np.random.default_rng([od, cap, pushes, STACKED_SALT.get((od, cap), 0)])
    ref = PrioritizedFramesRef(cap, 1, od, np.uint8 if dtype == "u8" else np.float32, n)
    return R.fill(ref, rng, dtype, pushes, 0.2, sink)


def write_back(ref, salt):
    """random priorities under the first 8 keys of a draw, the first of them 0 when another drawn key keeps the tree's mass; applied to
    the model's tree -> (keys, priorities) for the device to apply"""
    _, key, _ = ref.draw(64, SEED, 7)
    k = np.ascontiguousarray(key[:8])
    p = (0.5 + 3.5 * np.random.default_rng([salt, ref.n]).random(k.size)).astype(np.float32)
    if (k[1:] != k[0]).any():
        p[0] = 0.0  # (sequential semantics: a later duplicate of k[0] overrules it; either way a key with mass remains)
    ref.st.update(k, p)
    return k, p


def trees(make_ref, cap, sink_for=None):
    """Every tree of one (case, fill state): yields (name, model, n-steps to gather with, device owner, pending write-back).
      'masked n'    written by the lagged push after every transition; windows of n are drawn AND gathered
      'empty n'     the same while the ring holds fewer than n transitions: no mass, nothing for the model to say
      'written n'   'masked n' (n > 1) after a write-back of random priorities under drawn keys -- already applied to the model, handed
                    to the caller as (keys, priorities) for the device
      'unmasked'    the plain push (n = 1): any stored transition is a start, so windows cut at the ring's end occur
    `make_ref(n, sink)` builds and fills the model; `sink_for(n)` -> (sink, owner) lets the device test fill its traces in step."""
    for n in masked_nsteps(cap):
        sink, owner = sink_for(n) if sink_for else (None, None)
        ref = make_ref(n, sink)
        if not ref.has_mass():
            assert len(ref) < n
            yield f"empty {n}", ref, (), owner, None
            continue
        yield f"masked {n}", ref, (n,), owner, None
        if n > 1:
            yield f"written {n}", ref, (n,), owner, write_back(ref, cap)
    sink, owner = sink_for(1) if sink_for else (None, None)
    yield "unmasked", make_ref(1, sink), tuple(unmasked_nsteps(cap)), owner, None


def census(make_ref, cap, n_stack=None):
    """what the draws of one (case, fill state) hold, from the model alone: the counts of ring_nstep_ref.census summed per kind of tree"""
    out = {}
    for name, ref, gather_ns, _, _ in trees(make_ref, cap):
        kind = name.split(" ")[0]
        for n in gather_ns:
            for batch, _, ctr in draws(ref.n_env):
                c = R.census(ref, ref.draw(batch, SEED, ctr)[0], n, n_stack)
                c["full_multi_step"] = c["full"] if n > 1 else 0  # (every 1-step window without a terminal is "full")
                mine = out.setdefault(kind, {})
                for k, v in c.items():
                    mine[k] = mine.get(k, 0) + int(v)
    return out

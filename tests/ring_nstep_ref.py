"""n-step transitions of a frame ring stated on the list model of tests/ring_ref.py (plain numpy; no oracle, no GPU): positions in
Python lists, no head / length / modulo arithmetic, so this statement cannot share an indexing error with csrc/ring_nstep.hip.

The window of start (li, e) is transitions li .. li + ns - 1 of env e, ns = the smallest of n, k + 1 for the first k >= 0 with
terminal[li + k] != 0, and len - li.  The sample is (s = frame li, a[li], ret, terminal[li + ns - 1], s' = frame li + ns, ns) with
ret = discount_rewards_reduced over the window, folded step by step in np.float32 from the window's end:
gain = 0; for k = ns - 1 .. 0: gain = r[li + k] + gamma * gain (each product and each sum rounded to Float32: no fused multiply-add).

stack(f, n_stack) = frames f - n_stack + 1 .. f of a single-env ring, oldest first; a member is all zeros when its frame index is
negative or a terminal transition lies among the transitions from that frame up to f - 1.

Shared by tests/test_ring_nstep_reference.py (CPU) and tests/test_gpu_ring_nstep.py."""
import numpy as np

from ring_ref import RingRef, random_frame

# (dtype, obs_dim, n_env, capacity, frame_major): the routes of rlhip_ring_gather_nstep
PLAIN_CASES = [
    ("f32", 6, 5, 7, False),      # small f32 route
    ("f32", 5, 300, 3, False),    # a batch beyond one 256-sample tile
    ("u8", 7, 3, 5, False),       # odd frame size
    ("u8", 1008, 1, 4, False),    # small route, n_env = 1, below 1024 bytes
    ("u8", 1030, 1, 4, False),    # small route, not a multiple of 16 bytes
    ("u8", 1024, 1, 6, True),     # frame-major
    ("f32", 256, 1, 6, True),     # frame-major
    ("u8", 7056, 1, 6, True),     # frame-major, 441 chunks: a partial trip
]
PLAIN_NSTEPS = lambda cap: sorted({1, 2, 3, cap, 32})  # noqa: E731
GAMMAS = (0.99, 0.0, 1.0)
# (dtype, obs_dim, capacity), n_env = 1: rlhip_ring_gather_stacked_nstep
STACKED_CASES = [("u8", 48, 12), ("u8", 7056, 12), ("f32", 8, 12)]
STACKS = (1, 2, 4, 8)
STACKED_NSTEPS = (1, 2, 5, 32)
STACKED_PUSHES = (5, 27)


def plain_pushes(cap):
    return (2, 2 * cap + 3)  # ring not full; wrapped


class RingNStepRef(RingRef):
    def _first(self):
        return self.pushed_transitions - len(self)

    def window(self, li, e, n):
        """-> ns of the window that starts at logical transition li of env e"""
        assert 0 <= li < len(self) and 0 <= e < self.n_env and n >= 1, (li, e, n)
        k0 = self._first() + li
        ns = 0
        for t in self.t[k0:k0 + n]:  # (a list slice ends at the newest stored transition by itself)
            ns += 1
            if t[e] != 0:
                break
        return ns

    def nstep_transition(self, li, e, n, gamma):
        """-> (s, a, ret, term, s', ns)"""
        ns = self.window(li, e, n)
        k0 = self._first() + li
        g = np.float32(gamma)
        gain = np.float32(0.0)
        for r in reversed(self.r[k0:k0 + ns]):
            gain = np.float32(r[e] + np.float32(g * gain))
        return (self.frames[k0][:, e], self.a[k0][e], gain, np.uint8(self.t[k0 + ns - 1][e] != 0), self.frames[k0 + ns][:, e],
                np.int32(ns))

    def stack(self, f, n_stack):
        """the stack that ends at logical state frame f (0 <= f <= len) of a single-env ring -> (n_stack, obs_dim), oldest first"""
        assert self.n_env == 1 and 0 <= f <= len(self)
        first = self._first()
        out = np.zeros((n_stack, self.obs_dim), self.dtype)
        for back in range(n_stack):  # member n_stack - 1 - back is frame f - back
            g = f - back
            if g < 0 or any(t[0] != 0 for t in self.t[first + g:first + f]):
                break  # ... and every older member stays zero with it
            out[n_stack - 1 - back] = self.frames[first + g][:, 0]
        return out

    def member_is_zero_filled(self, f, n_stack):
        """per member of stack(f): was it zero-FILLED (as opposed to copied from a frame)"""
        first = self._first()
        return [f - back < 0 or any(t[0] != 0 for t in self.t[first + f - back:first + f]) for back in range(n_stack - 1, -1, -1)]

    def gather_nstep(self, flat_idx, n, gamma):
        """-> (s (obs_dim, batch), a, ret, term, s' (obs_dim, batch), ns)"""
        flat_idx = np.asarray(flat_idx, np.int64).reshape(-1)
        b = flat_idx.size
        s, sn = np.empty((self.obs_dim, b), self.dtype), np.empty((self.obs_dim, b), self.dtype)
        a, ret, t, ns = np.empty(b, np.int32), np.empty(b, np.float32), np.empty(b, np.uint8), np.empty(b, np.int32)
        for i, j in enumerate(flat_idx.tolist()):
            li, e = divmod(j, self.n_env)
            s[:, i], a[i], ret[i], t[i], sn[:, i], ns[i] = self.nstep_transition(li, e, n, gamma)
        return s, a, ret, t, sn, ns

    def gather_stacked_nstep(self, idx, n_stack, n, gamma):
        """-> (s (batch, n_stack, obs_dim), a, ret, term, s', ns)"""
        idx = np.asarray(idx, np.int64).reshape(-1)
        b = idx.size
        s, sn = np.empty((b, n_stack, self.obs_dim), self.dtype), np.empty((b, n_stack, self.obs_dim), self.dtype)
        a, ret, t, ns = np.empty(b, np.int32), np.empty(b, np.float32), np.empty(b, np.uint8), np.empty(b, np.int32)
        for i, li in enumerate(idx.tolist()):
            _, a[i], ret[i], t[i], _, ns[i] = self.nstep_transition(li, 0, n, gamma)
            s[i], sn[i] = self.stack(li, n_stack), self.stack(li + int(ns[i]), n_stack)
        return s, a, ret, t, sn, ns


def frame_major6(batch):
    s, a, ret, t, sn, ns = batch
    return np.ascontiguousarray(s.T), a, ret, t, np.ascontiguousarray(sn.T), ns


def nstep_traces(rng, n_env, p_term, n_actions=6):
    """random actions, rewards that include -0.0 and exact zeros, terminals with probability p_term"""
    r = rng.standard_normal(n_env).astype(np.float32)
    r[rng.random(n_env) < 0.1] = np.float32(-0.0)
    return rng.integers(0, n_actions, n_env).astype(np.int32), r, (rng.random(n_env) < p_term).astype(np.uint8)


def fill(ref, rng, dtype, pushes, p_term, sink=None):
    """one state and `pushes` transitions into the model (and into `sink(frame, a, r, t)`, a = None for the state: the device ring)"""
    f = random_frame(rng, dtype, ref.obs_dim, ref.n_env)
    ref.push_state(f)
    if sink:
        sink(f, None, None, None)
    for _ in range(pushes):
        f, (a, r, t) = random_frame(rng, dtype, ref.obs_dim, ref.n_env), nstep_traces(rng, ref.n_env, p_term)
        ref.push_transition(f, a, r, t)
        if sink:
            sink(f, a, r, t)
    return ref


# seeds under which the census of tests/test_ring_nstep_reference.py holds (single-env rings of capacity 4 or 6 hold few windows)
PLAIN_SALT = {(1008, 1, 4): 27, (1030, 1, 4): 2, (256, 1, 6): 5}  # (obs_dim, n_env, capacity) -> last word of the seed; others 0
STACKED_SALT = {(48, 12): 9}                                      # (obs_dim, capacity)


def plain_model(case, pushes, sink=None):
    """the filled model of one plain case (the same content in `sink`)"""
    dtype, od, n_env, cap, _ = case
    rng = np.random.default_rng([od, n_env, cap, pushes, PLAIN_SALT.get((od, n_env, cap), 0)])
    ref = RingNStepRef(cap, n_env, od, np.uint8 if dtype == "u8" else np.float32)
    return fill(ref, rng, dtype, pushes, 0.25, sink)


def stacked_model(case, pushes, sink=None):
    dtype, od, cap = case
    rng = np.random.default_rng([od, cap, pushes, STACKED_SALT.get((od, cap), 0)])
    ref = RingNStepRef(cap, 1, od, np.uint8 if dtype == "u8" else np.float32)
    return fill(ref, rng, dtype, pushes, 0.2, sink)


def exhaustive_batch(ref, seed):
    """every valid flat index, shuffled, with duplicates added"""
    rng = np.random.default_rng(seed)
    total = len(ref) * ref.n_env
    idx = np.concatenate([np.arange(total), rng.integers(0, total, max(3, total // 4))]).astype(np.int64)
    rng.shuffle(idx)
    return idx


def census(ref, idx, n, n_stack=None):
    """which kinds of window the batch holds, from the model alone"""
    c = dict(full=0, terminal_cut=0, terminal_at_n=0, ring_end_cut=0, zero_s=0, zero_sn=0, ns_lt_stack=0, ns_ge_stack=0)
    for j in np.asarray(idx).tolist():
        li, e = divmod(j, ref.n_env)
        ns = ref.window(li, e, n)
        term = ref.t[ref._first() + li + ns - 1][e] != 0
        c["full"] += ns == n and not term
        c["terminal_cut"] += bool(term) and ns < n
        c["terminal_at_n"] += bool(term) and ns == n
        c["ring_end_cut"] += (not term) and ns < n
        if n_stack is not None:
            c["zero_s"] += any(ref.member_is_zero_filled(li, n_stack))
            c["zero_sn"] += any(ref.member_is_zero_filled(li + ns, n_stack))
            c["ns_lt_stack"] += ns < n_stack
            c["ns_ge_stack"] += ns >= n_stack
    return c

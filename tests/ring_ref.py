"""CircularArraySARTSTraces stated as a list model (plain numpy; no oracle, no GPU): every push appends to Python lists and a
transition is read back by its position in those lists.  There is no head / length / modulo arithmetic here, so this statement
cannot share an indexing error with csrc/ring.hip or oracle/rlo_buffer.c.

Semantics (RLTrajectories 0.4 `CircularArraySARTSTraces`, push protocol RLCore/src/policies/agent/agent_base.jl:45-59): the traces
hold the newest `capacity` transitions; `next_state[i] = state[i + 1]` (one multiplexed state trace), so with
`first = pushed_transitions - len` logical transition li of env e is
    (frames[first + li][:, e], a[first + li][e], r[first + li][e], t[first + li][e], frames[first + li + 1][:, e]).
Shared by tests/test_ring_reference.py (CPU, against oracle.Ring) and tests/test_gpu_ring_layouts.py."""
import numpy as np


class RingRef:
    def __init__(self, capacity, n_env, obs_dim, dtype=np.float32):
        self.capacity, self.n_env, self.obs_dim, self.dtype = int(capacity), int(n_env), int(obs_dim), np.dtype(dtype)
        self.frames, self.a, self.r, self.t = [], [], [], []  # frames[k + 1] is s' of pushed transition k

    def _frame(self, obs):
        f = np.array(obs, dtype=self.dtype, copy=True)
        assert f.shape == (self.obs_dim, self.n_env), (f.shape, (self.obs_dim, self.n_env))
        return f

    def push_state(self, obs):
        """push!(traces, (state = s,)): opens the traces; a second open state is rejected by the ring"""
        assert not self.frames, "a state is already open"
        self.frames.append(self._frame(obs))

    def push_transition(self, next_obs, a, r, t):
        """push!(traces, (state = s', action = a, reward = r, terminal = t))"""
        assert self.frames, "push the first state before the first transition"
        for x in (a, r, t):
            assert np.shape(x) == (self.n_env,)
        self.frames.append(self._frame(next_obs))
        self.a.append(np.array(a, np.int32))
        self.r.append(np.array(r, np.float32))
        self.t.append((np.asarray(t) != 0).astype(np.uint8))

    def push_state_maxpool(self, screen1, screen2):
        """frame = max.(screen1, screen2)  (AtariEnv.act!, RLEnvs/src/environments/3rd_party/atari.jl:104-107)"""
        self.push_state(np.maximum(screen1, screen2))

    def push_transition_maxpool(self, screen1, screen2, a, r, t):
        self.push_transition(np.maximum(screen1, screen2), a, r, t)

    @property
    def pushed_transitions(self):
        return len(self.a)

    def __len__(self):
        return min(self.pushed_transitions, self.capacity)

    def transition(self, li, e):
        """logical transition li (0 = oldest kept) of env e -> (s, a, r, t, s')"""
        assert 0 <= li < len(self) and 0 <= e < self.n_env, (li, e)
        k = self.pushed_transitions - len(self) + li
        return self.frames[k][:, e], self.a[k][e], self.r[k][e], self.t[k][e], self.frames[k + 1][:, e]

    def gather(self, flat_idx):
        """traces[inds], inds flat over (transition, env): li, e = divmod(j, n_env)
        -> (s (obs_dim, batch), a, r, t, s' (obs_dim, batch))"""
        flat_idx = np.asarray(flat_idx, np.int64).reshape(-1)
        b = flat_idx.size
        s, sn = np.empty((self.obs_dim, b), self.dtype), np.empty((self.obs_dim, b), self.dtype)
        a, r, t = np.empty(b, np.int32), np.empty(b, np.float32), np.empty(b, np.uint8)
        for i, j in enumerate(flat_idx.tolist()):
            li, e = divmod(j, self.n_env)
            s[:, i], a[i], r[i], t[i], sn[:, i] = self.transition(li, e)
        return s, a, r, t, sn


def frame_major(batch):
    """(s (obs_dim, batch), a, r, t, s') -> the frame-major form (s (batch, obs_dim), ..): what the large-frame gather of a
    single-env ring returns, a frame staying contiguous"""
    s, a, r, t, sn = batch
    return np.ascontiguousarray(s.T), a, r, t, np.ascontiguousarray(sn.T)


# (dtype, obs_dim, n_env, capacity, frame_major): every frame-ring and record-ring route of csrc/ring.hip that only these tests
# fill through a push and compare on content -- the route each case takes is named in tests/test_gpu_ring_layouts.py
CASES = [
    ("f32", 6, 5, 7, False),
    ("f32", 6, 8, 5, False),
    ("f32", 5, 300, 3, False),
    ("f32", 8, 1, 9, False),
    ("u8", 4, 8, 6, False),
    ("u8", 32, 3, 5, False),
    ("u8", 7, 3, 5, False),
    ("u8", 1008, 1, 4, False),
    ("u8", 1030, 1, 4, False),
    ("u8", 1024, 1, 4, True),
    ("f32", 1, 37, 6, False),
    ("f32", 3, 37, 6, False),
]


def case_id(c):
    return f"{c[0]}-{c[1]}x{c[2]}-cap{c[3]}"


def random_frame(rng, dtype, obs_dim, n_env):
    """UInt8: the full 0..255 range, 0 and 255 planted in every frame that has room; Float32: non-constant normals"""
    if dtype == "u8":
        f = rng.integers(0, 256, (obs_dim, n_env), dtype=np.uint8)
        flat = f.reshape(-1)
        if flat.size >= 2:
            i, j = rng.choice(flat.size, 2, replace=False)
            flat[i], flat[j] = 0, 255
        return f
    return rng.standard_normal((obs_dim, n_env)).astype(np.float32)


def random_traces(rng, n_env, n_actions=6):
    """random actions, non-constant rewards, terminals with p = 0.2"""
    return (rng.integers(0, n_actions, n_env).astype(np.int32), rng.standard_normal(n_env).astype(np.float32),
            (rng.random(n_env) < 0.2).astype(np.uint8))

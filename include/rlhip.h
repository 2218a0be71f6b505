/*
 * rlhip.h -- C ABI of librlhip.so: the MI355X-native rollout + learner hot path for
 * ReinforcementLearning.jl (vectorised classic-control env step -> replay ring push/gather ->
 * GAE / TD target / Huber / Adam -> gradient hand-off to the all-reduce).
 *
 * The reference has NO foreign-function boundary (it is 100 % Julia, zero `ccall`; SURVEY.md
 * section 0), so each entry point below names the Julia function(s) it replaces; the `ccall`
 * stubs a maintainer would add are in INTEGRATION.md and reinforcementlearning.jl_amd/julia/RLHip.jl.
 * Reference paths are relative to /root/reference/src/ :
 *   RLEnvs = ReinforcementLearningEnvironments/src/environments/examples
 *   RLCore = ReinforcementLearningCore/src
 *
 * Conventions
 *   - plain C: pointers, sizes, POD structs.  No torch / HIP types in any signature
 *     (a stream is an opaque `void*` holding a hipStream_t; NULL = the default stream).
 *   - every function returns int32: 0 = RLHIP_OK, < 0 = error; message via rlhip_last_error().
 *   - all data pointers are DEVICE pointers unless the name ends in `_host`.  Calls enqueue on the
 *     given stream and return immediately (no implicit sync) unless documented otherwise.
 *   - indices are 0-based (Julia glue adds/subtracts 1: actions 1..na <-> 0..na-1).
 *   - layouts are SoA: a per-env quantity q with D components is stored as q[d * n + i]
 *     (component-major, env index i contiguous) so that one wavefront lane per env reads coalesced.
 *     Time-major trajectories: x[(t * D + d) * n + i].
 *   - random draws follow the Philox4x32-10 specification in DESIGN.md (ctr = {idx, blk, t, tag},
 *     key = seed); `env_id_base` offsets idx so shards on different GPUs own disjoint streams and
 *     results do not depend on the number of GPUs.
 */
#ifndef RLHIP_H
#define RLHIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RLHIP_OK 0
#define RLHIP_EINVAL (-1) /* bad argument (the reference would throw AssertionError / ArgumentError / MethodError) */
#define RLHIP_EHIP (-2)   /* a HIP runtime call failed */
#define RLHIP_ENODEV (-3) /* no gfx950 device visible */
#define RLHIP_ETIMEOUT (-4) /* a peer never arrived at a gradient exchange; the result was overwritten with NaN */
#define RLHIP_ECOMM (-5)    /* RCCL is missing or one of its calls failed / no transport for this exchange */

/* 2 (round 5): rlhip_ring rings of Float32 observations with <= 4 components store 64-byte transition records (s, a, r, t, s'
 *    per (slot, env)); `rlhip_ring.layout` names the layout, rlhip_ring_init takes NULL action / reward / terminal for
 *    them; rlhip_ppo_workspace_init + the capacity check of rlhip_ppo_update_f32; rlhip_eps_greedy_prob_f32.  ABI 1 stored those
 *    states transition-major with three separate traces (and round 3 component-major): a host built against an older header
 *    fails rlhip_abi_version() == RLHIP_ABI_VERSION and, if it skips that check, rlhip_ring_init (RLHIP_EINVAL). */
#define RLHIP_ABI_VERSION 2

typedef void* rlhip_stream_t; /* hipStream_t */
typedef void* rlhip_event_t;  /* hipEvent_t  */

/* ------------------------------------------------------------------------------ runtime -- */
int32_t rlhip_abi_version(void);
const char* rlhip_last_error(void);
int32_t rlhip_device_count(int32_t* n_out);
int32_t rlhip_set_device(int32_t device);
/* device arch name, e.g. "gfx950:sramecc+:xnack-" (host buffer) */
int32_t rlhip_device_name(int32_t device, char* name_host, int32_t cap);

/* Device memory / streams / events for hosts that own no GPU allocator (the Julia glue).  A host
 * that already has one (PyTorch-ROCm here) passes its own pointers and stream instead. */
int32_t rlhip_malloc(void** ptr_out, size_t bytes);
int32_t rlhip_free(void* ptr);
int32_t rlhip_memset(void* ptr, int32_t value, size_t bytes, rlhip_stream_t stream);
int32_t rlhip_memcpy_h2d(void* dst, const void* src_host, size_t bytes, rlhip_stream_t stream); /* syncs stream */
int32_t rlhip_memcpy_d2h(void* dst_host, const void* src, size_t bytes, rlhip_stream_t stream); /* syncs stream */
int32_t rlhip_memcpy_d2d(void* dst, const void* src, size_t bytes, rlhip_stream_t stream);
int32_t rlhip_stream_create(rlhip_stream_t* stream_out);
int32_t rlhip_stream_destroy(rlhip_stream_t stream);
int32_t rlhip_stream_sync(rlhip_stream_t stream);
int32_t rlhip_event_create(rlhip_event_t* event_out);
int32_t rlhip_event_destroy(rlhip_event_t event);
int32_t rlhip_event_record(rlhip_event_t event, rlhip_stream_t stream);
/* syncs on `stop`, returns milliseconds between the two recorded events */
int32_t rlhip_event_elapsed_ms(rlhip_event_t start, rlhip_event_t stop, float* ms_out);

/* Philox uniforms U[0,1) (24-bit, Float32) -- synthetic data / weight init helper.
 * out[i] = u01(word (i % 4) of Philox(seed, idx = i / 4, blk = 0, t, tag)). */
int32_t rlhip_fill_uniform_f32(float* out, int64_t n, uint64_t seed, uint32_t t, uint32_t tag,
                               rlhip_stream_t stream);
/* keyed permutation of [0, n) (the `shuffle(rng, 1:n)` stand-in): out[i] = perm_epoch(i) */
int32_t rlhip_permutation(uint32_t* out, uint32_t n, uint64_t seed, uint32_t epoch,
                          rlhip_stream_t stream);

/* --------------------------------------------------------------------------------- envs -- */
#define RLHIP_ENV_CARTPOLE 0    /* RLEnvs/CartPoleEnv.jl */
#define RLHIP_ENV_PENDULUM 1    /* RLEnvs/PendulumEnv.jl */
#define RLHIP_ENV_MOUNTAINCAR 2 /* RLEnvs/MountainCarEnv.jl */
#define RLHIP_ENV_ACROBOT 3     /* RLEnvs/src/environments/3rd_party/AcrobotEnv.jl (stand-alone env kernels only) */

/* CartPoleEnv(; kwargs...)  RLEnvs/CartPoleEnv.jl:22-32,74-79 -- Float64 as typed by the caller */
typedef struct {
    double gravity, masscart, masspole, halflength, forcemag, dt, thetathreshold_deg, xthreshold;
    int64_t max_steps;
    int32_t continuous; /* 0: action int32 in {0,1} (Julia 1,2); 1: action of type T in [-1,1] */
} rlhip_cartpole_cfg;

/* PendulumEnv(; kwargs...)  RLEnvs/PendulumEnv.jl:41-53 */
typedef struct {
    double max_speed, max_torque, g, m, l, dt;
    int64_t max_steps;
    int32_t continuous; /* 1: torque of type T; 0: int32 index in 0..n_actions-1 */
    int32_t n_actions;
} rlhip_pendulum_cfg;

/* MountainCarEnv(; kwargs...)  RLEnvs/MountainCarEnv.jl:19-40,67-81 */
typedef struct {
    double min_pos, max_pos, max_speed, goal_pos, goal_velocity, power, gravity;
    int64_t max_steps;
    int32_t continuous;
} rlhip_mountaincar_cfg;

/* AcrobotEnv(; kwargs...)  3rd_party/AcrobotEnv.jl:22-40.  PARITY UNPINNED: the reference integrates one act! with
 * OrdinaryDiffEq.solve(ode, RK4()) (:128-129), an un-vendored adaptive driver whose step-size controller decides the
 * arithmetic; this library takes ONE classic RK4 step of length dt over the reference's dsdt (:147-199) in Float64
 * (the "python gym" scheme the file cites), wraps / bounds (:135-138) and stores the state as T.  Discrete actions
 * 0..2 (torque -1, 0, +1); max_torque_noise > 0 draws one uniform per act! from the Philox stream ENVNOISE.
 * reward(env) is -1 after reset! (:99). */
typedef struct {
    double link_length_a, link_length_b, link_mass_a, link_mass_b, link_com_pos_a, link_com_pos_b, link_moi,
        max_torque_noise, max_vel_a, max_vel_b, g, dt;
    int64_t max_steps;
    int32_t nips; /* book_or_nips: 0 "book" (default), 1 "nips" */
} rlhip_acrobot_cfg;

int32_t rlhip_cartpole_default(rlhip_cartpole_cfg* cfg_host);
int32_t rlhip_acrobot_default(rlhip_acrobot_cfg* cfg_host);
int32_t rlhip_pendulum_default(rlhip_pendulum_cfg* cfg_host);
int32_t rlhip_mountaincar_default(rlhip_mountaincar_cfg* cfg_host, int32_t continuous);

/* SoA state of n env instances (device arrays, caller-owned).
 *   s[k]    T[n]   state component k (cartpole: x, xdot, theta, thetadot; pendulum: theta, thetadot;
 *                  mountaincar: x, v; acrobot: theta1, theta2, dtheta1, dtheta2)
 *   t       i32[n] step counter of the running episode
 *   done    u8[n]  is_terminated(env) after the LAST act!
 *   reward  T[n]   reward(env) after the last act!
 *   episode u32[n] number of resets so far (Philox time counter of the next reset)
 * PACKED MODE (episode == NULL; rlhip_env_reset / rlhip_env_step / rlhip_env_obs only): the reset counter lives in
 * the bits of t[i] that max_steps leaves free -- t[i] = step | episode << tbits, tbits = the smallest b >= 1 with
 * 2^b > max_steps + 1 (CartPole default 200: 8 bits of step, 24 bits = 16.7 M episodes; the counter SATURATES there --
 * rlhip_env_packed_episode_capacity -- so a host that may step an instance that often must keep episode[]).
 * Same states, rewards, flags and reset draws as the separate array; an auto-reset then touches no memory that the
 * step kernel does not stream anyway (with episode[] every reset is a scattered 4-byte read-modify-write: +9 % HBM
 * traffic at 2^24 CartPole envs under a random policy).  max_steps < 2^20 - 1.                  */
typedef struct {
    void* s[4];
    int32_t* t;
    uint8_t* done;
    void* reward;
    uint32_t* episode;
} rlhip_env_state;

int64_t rlhip_env_packed_episode_capacity(int64_t max_steps); /* 2^(32 - tbits) - 1, or -1 (max_steps out of range) */
int32_t rlhip_env_obs_dim(int32_t kind);   /* cartpole 4, pendulum 3 (sin, cos, thetadot), mountaincar 2, acrobot 6 */
int32_t rlhip_env_state_dim(int32_t kind); /* cartpole 4, pendulum 2, mountaincar 2, acrobot 4 */

/* reset!(env)   CartPoleEnv.jl:98-104, PendulumEnv.jl:84-92, MountainCarEnv.jl:99-105.
 * mask == NULL: reset every env (reset!(env; is_force = true) of the vector env); otherwise only
 * where mask[i] != 0 (reset!(env) of the vector env = "reset the terminated ones", pass st->done). */
int32_t rlhip_env_reset(int32_t kind, int32_t is_f64, const void* cfg_host,
                        const rlhip_env_state* st_host, int64_t n, uint64_t seed,
                        uint32_t env_id_base, const uint8_t* mask, rlhip_stream_t stream);

/* act!(env, a) = _step! + reward + is_terminated for every env in one launch
 *   CartPoleEnv.jl:106-140,:84-85; PendulumEnv.jl:94-122; MountainCarEnv.jl:107-135,:95.
 * actions: i32[n] (discrete, 0-based) or T[n] (continuous).
 * auto_reset != 0: the MultiThreadEnv protocol -- reward/done of the finished step stay visible and a
 *   terminated env immediately starts a fresh episode inside the same kernel.
 * last_obs (nullable): T[obs_dim * n] receives the observation BEFORE the auto-reset.
 * obs_out  (nullable): T[obs_dim * n] receives state(env) AFTER the step (and auto-reset).       */
int32_t rlhip_env_step(int32_t kind, int32_t is_f64, const void* cfg_host,
                       const rlhip_env_state* st_host, int64_t n, const void* actions,
                       int32_t auto_reset, uint64_t seed, uint32_t env_id_base, void* last_obs,
                       void* obs_out, rlhip_stream_t stream);

/* state(env)  CartPoleEnv.jl:86, PendulumEnv.jl:70,82, MountainCarEnv.jl:97 -> T[obs_dim * n] */
int32_t rlhip_env_obs(int32_t kind, int32_t is_f64, const rlhip_env_state* st_host, int64_t n,
                      void* obs_out, rlhip_stream_t stream);

/* -------------------------------------------------------------------------------- scans -- */
/* discount_rewards / discount_rewards_reduced / generalized_advantage_estimation
 *   RLCore/utils/basic.jl:138-235, :237-319, :334-417.
 * Matrices are column-major n1 x n2 like Julia.  dims = 0: vector (n2 must be 1);
 * dims = 1 / 2: the Julia `dims` keyword = the axis the scan runs along.  A matrix with dims = 0 is
 * RLHIP_EINVAL (the reference throws MethodError).  terminal / init may be NULL (`nothing`).
 * values has one more entry than rewards along the scan axis.
 * dims = 2 is the coalesced PPO layout (rewards (n_env, T)): one lane per env, T serial.        */
int32_t rlhip_discount_rewards_f32(float* out, const float* rewards, int64_t n1, int64_t n2,
                                   float gamma, const uint8_t* terminal, const float* init,
                                   int32_t dims, rlhip_stream_t stream);
int32_t rlhip_discount_rewards_f64(double* out, const double* rewards, int64_t n1, int64_t n2,
                                   double gamma, const uint8_t* terminal, const double* init,
                                   int32_t dims, rlhip_stream_t stream);
int32_t rlhip_discount_rewards_reduced_f32(float* out, const float* rewards, int64_t n1, int64_t n2,
                                           float gamma, const uint8_t* terminal, const float* init,
                                           int32_t dims, rlhip_stream_t stream);
int32_t rlhip_discount_rewards_reduced_f64(double* out, const double* rewards, int64_t n1,
                                           int64_t n2, double gamma, const uint8_t* terminal,
                                           const double* init, int32_t dims, rlhip_stream_t stream);
int32_t rlhip_gae_f32(float* advantages, const float* rewards, const float* values, int64_t n1,
                      int64_t n2, float gamma, float lambda, const uint8_t* terminal, int32_t dims,
                      rlhip_stream_t stream);
int32_t rlhip_gae_f64(double* advantages, const double* rewards, const double* values, int64_t n1,
                      int64_t n2, double gamma, double lambda, const uint8_t* terminal, int32_t dims,
                      rlhip_stream_t stream);
/* PPO fusion: advantages AND returns = advantages + values[:, 1:T] in one pass over (n_env, T)
 * time-major arrays (dims = 2 semantics). returns may be NULL. */
int32_t rlhip_gae_returns_f32(float* advantages, float* returns, const float* rewards,
                              const float* values, const uint8_t* terminal, int64_t n_env, int64_t T,
                              float gamma, float lambda, rlhip_stream_t stream);

/* ---------------------------------------------------------------------------- selection -- */
/* element (k, i) of a (na x n) value array = values[k * k_stride + i * i_stride]:
 *   Julia (na, N) column-major: k_stride = 1, i_stride = na;  SoA: k_stride = n, i_stride = 1.  */

/* plan!(::EpsilonGreedyExplorer, values[, mask]) for n envs
 *   RLCore/policies/explorers/epsilon_greedy_explorer.jl:102-131 (+ findmax / find_all_max
 *   RLCore/utils/basic.jl:91-120); eps from rlhip_get_eps; GreedyExplorer (:200-205) = eps 0.
 * mask (nullable) u8, same strides as values, any non-zero byte = true.  actions: i32[n], 0-based.
 * draws: Philox(seed, idx = env_id_base + i (mod 2^32), blk 0, t = step, EXPLORE): (w0,w1) -> u, w2 -> random index,
 * w3 -> tie-break index.  Everywhere below: uniform Float64 = ((hi << 32 | lo) >> 11) 2^-53 of a word pair (hi first),
 * uniform Float32 = (w >> 8) 2^-24, index in [0, c) = (w c) >> 32.
 * Where the reference throws, index 0 is returned: rand(rng, Int[]) after find_all_max met a NaN maximum (no entry == NaN;
 * is_break_tie only) and findall / maximum over an all-false mask. */
int32_t rlhip_eps_greedy_select_f32(const float* values, int64_t na, int64_t n, int64_t k_stride,
                                    int64_t i_stride, const uint8_t* mask, double eps,
                                    int32_t is_break_tie, uint64_t seed, uint32_t env_id_base,
                                    uint32_t step, int32_t* actions, rlhip_stream_t stream);
/* prob(::EpsilonGreedyExplorer, values[, mask]) for n envs  epsilon_greedy_explorer.jl:141-194 (the vector the reference wraps
 * in Categorical(probs; check_args = false); pinned by RLCore/test/policies/explorers/epsilon_greedy_explorer.jl:45-73):
 *   probs[k] = eps / n_legal on legal actions, 0 on masked ones; + (1 - eps) on findmax(values[, mask]) (is_break_tie = 0),
 *   or + (1 - eps) / c on each of the c entries of find_all_max(values[, mask]) (is_break_tie = 1).
 * probs: f64, same (k_stride, i_stride) addressing as values.  Float64 like the reference (eps is a Float64).
 * is_break_tie with a NaN maximum: the tie set is empty, the column holds eps / n_legal only (as the reference's loop over no
 * index); with an all-false mask (the reference throws): zeros, and 1 - eps at index 0 when is_break_tie = 0 (findmax of all
 * typemin). */
int32_t rlhip_eps_greedy_prob_f32(const float* values, int64_t na, int64_t n, int64_t k_stride, int64_t i_stride,
                                  const uint8_t* mask, double eps, int32_t is_break_tie, double* probs,
                                  rlhip_stream_t stream);
/* get_eps  epsilon_greedy_explorer.jl:69-88 (host-side scalar; kind 0 = linear, 1 = exp) */
double rlhip_get_eps(int32_t kind, double eps_stable, double eps_init, int64_t warmup_steps,
                     int64_t decay_steps, int64_t step);
/* sample_categorical (Gumbel-max)  RLCore/utils/networks.jl:425-432 on logits .+ ifelse.(mask, 0f0, typemin) (:468).
 * logp_out (nullable) f32[n] = logsoftmax(logits)[action].
 * draws: Philox(seed, idx = env_id_base + i (mod 2^32), blk = k / 2, t = step, GUMBEL) for action k (0-based): even k takes the
 * Float64 uniform of (w0, w1), odd k that of (w2, w3) -- one block per two actions, no word read twice; Gumbel noise
 * -log(-log(u)) in Float64, added to the Float32 log-probability; the first maximal index wins.
 * The mask is an ADDITION as in the reference: a masked NaN or +Inf logit becomes NaN (NaN + -Inf, Inf + -Inf), every other
 * masked logit -Inf.  logsoftmax is the plain x - max - log(sum(exp(x - max))) with max skipping NaN: a NaN logit, a +Inf logit
 * (Inf - Inf) and a column of -Inf only (all masked) make every log-probability NaN; action 0 is returned with a NaN logp_out.
 * For +Inf the reference delegates to NNlib.logsoftmax, which is not vendored and may special-case it: that case is pinned
 * here as stated, not to the reference. */
int32_t rlhip_categorical_sample_f32(const float* logits, int64_t na, int64_t n, int64_t k_stride,
                                     int64_t i_stride, const uint8_t* mask, uint64_t seed,
                                     uint32_t env_id_base, uint32_t step, int32_t* actions,
                                     float* logp_out, rlhip_stream_t stream);

/* (net::CategoricalNetwork)(state[, mask]; is_sampling, is_return_log_prob)  RLCore/utils/networks.jl:405-432, masked
 * methods :459-472, on (na, n) component-major logits in one launch: masked_logits_out (nullable) = logits +
 * ifelse(mask, 0, typemin) (:461; mask NULL = all true); actions (nullable) = the Gumbel-max draw from them (0-based, same
 * draws as rlhip_categorical_sample_f32); onehot_out (nullable, needs actions) = Flux.onehotbatch(draw, 1:na). */
int32_t rlhip_categorical_network_f32(const float* logits, int64_t na, int64_t n, const uint8_t* mask, uint64_t seed,
                                      uint32_t env_id_base, uint32_t step, float* masked_logits_out, int32_t* actions,
                                      float* onehot_out, rlhip_stream_t stream);

/* The remaining explorers as batched kernels (BatchExplorer semantics: the inner explorer applied to each column,
 * RLCore/src/policies/explorers/batch_explorer.jl:14-21).  values / mask addressing as rlhip_eps_greedy_select.
 *   kind 0  WeightedExplorer{is_normalized}   weighted_explorer.jl:19-33  (mask: weight 0)
 *   kind 1  WeightedSoftmaxExplorer           weighted_softmax_explorer.jl:21-27  (mask: typemin)
 *   kind 2  GumbelSoftmaxExplorer             gumbel_softmax_explorer.jl:11-24  (Float32 Gumbel noise)
 * draws, idx = env_id_base + i (mod 2^32), t = step:
 *   kind 0, 1  blk 0, EXPLORE: the Float64 uniform of (w0, w1) -> t = u * sum(weights) (kind 0 with is_normalized, kind 1: t = u);
 *              the walk `cw < t` over the Float32 running sum, w2 / w3 unused
 *   kind 2     blk 0x8000 + k / 4, GUMBEL, for action k: the Float32 uniform of word k % 4 -- one block per four actions; the
 *              blocks 0x8000.. keep clear of rlhip_categorical_sample_f32's (blk < 2^15 for na <= 2^16) under the same tag
 * na <= 64 (RLHIP_EINVAL above, nothing written); kind outside 0..2 is RLHIP_EINVAL.  kind 1 / 2 use the plain softmax /
 * logsoftmax formulas (see rlhip_categorical_sample_f32): a NaN or +Inf value or an all-false mask gives action 0; kind 0 walks
 * whatever IEEE gives (all-zero weights: action 0; the walk stops at the first NaN or +Inf partial sum). */
int32_t rlhip_explorer_select_f32(int32_t kind, const float* values, int64_t na, int64_t n, int64_t k_stride,
                                  int64_t i_stride, const uint8_t* mask, int32_t is_normalized, uint64_t seed,
                                  uint32_t env_id_base, uint32_t step, int32_t* actions, rlhip_stream_t stream);
/* UCBExplorer  UCB_explorer.jl:24-30: argmax of values + c sqrt(log(step + 1) / counts) with a uniform pick among
 * ties; action_counts: f64 (na, n) device, counts[k * n + i], initialised to eps (1e-10), incremented here.
 * step >= 1 (Int64, the reference's p.step; 0 is RLHIP_EINVAL, nothing written).
 * draws: Philox(seed, idx = env_id_base + i (mod 2^32), blk 0, t = step mod 2^32, EXPLORE): w0 -> tie-break index among the
 * entries equal to the maximum, in ascending action order; w1..w3 unused.
 * A NaN score makes the maximum NaN and the tie set empty (the reference throws at rand(rng, inds)): action 0 is returned and
 * counts[0] incremented. */
int32_t rlhip_ucb_select_f32(const float* values, int64_t na, int64_t n, int64_t k_stride, int64_t i_stride,
                             double c, double* action_counts, int64_t step, uint64_t seed, uint32_t env_id_base,
                             int32_t* actions, rlhip_stream_t stream);

/* ---------------------------------------------------------------------- parameter updates -- */
/* TargetNetwork sync: dest = rho * dest + (1 - rho) * src   target_network.jl:76-85 (rho = 0: hard copy) */
int32_t rlhip_polyak_f32(float* dst, const float* src, int64_t n, float rho, rlhip_stream_t stream);
/* clip_by_global_norm!(gs, ps, clip_norm)  RLCore/utils/basic.jl:19-29 over one flat gradient.
 * gn_out: f32[1] device (the returned norm). */
int32_t rlhip_clip_by_global_norm_f32(float* grad, int64_t n, float clip_norm, float* gn_out,
                                      rlhip_stream_t stream);
/* Flux.Optimise.update!(opt_state, model, grad)  flux_approximator.jl:46 with Optimisers.Adam.
 * beta_pow: f32[2] device = running (beta1^t, beta2^t), initialised to (beta1, beta2); updated here. */
int32_t rlhip_adam_f32(float* params, const float* grad, float* m, float* v, float* beta_pow,
                       int64_t n, float lr, float beta1, float beta2, float eps,
                       rlhip_stream_t stream);
/* fused: [global norm -> clip] -> Adam in ONE single-workgroup launch (n <= ~1M).  clip_norm <= 0
 * disables clipping.  grad_scale multiplies the gradient first (1/world_size after a sum all-reduce). */
int32_t rlhip_clip_adam_f32(float* params, float* grad, float* m, float* v, float* beta_pow,
                            int64_t n, float grad_scale, float clip_norm, float lr, float beta1,
                            float beta2, float eps, float* gn_out, rlhip_stream_t stream);
/* normlogpdf / diagnormlogpdf  RLCore/utils/distributions.jl:18-21, :31-34 (eps = 1f-8).
 * diag: arrays (d x n) column-major, out f32[n]. */
int32_t rlhip_normlogpdf_f32(const float* mu, const float* sigma, const float* x, float* out,
                             int64_t n, rlhip_stream_t stream);
int32_t rlhip_diagnormlogpdf_f32(const float* mu, const float* sigma, const float* x, int64_t d,
                                 int64_t n, float* out, rlhip_stream_t stream);
/* Stochastic Gaussian policy heads  RLCore/src/utils/networks.jl: GaussianNetwork :64-116 (logpdfcorrection /
 * inversesquash :39-42), SoftGaussianNetwork :147-198.  mu, raw_sigma: outputs of the mu / sigma sub-networks,
 * f32 (d x n) column-major; sigma = clamp(raw_sigma, min_sigma, max_sigma).  K samples per state
 * (K = 1: the `is_sampling = true` call; K > 1: the `(state, action_samples::Int)` call): z = mu + sigma * noise with
 * noise from the Philox NORMAL stream (draw k + d*j of (seed, env_id_base + i, step)).
 *   squash 0 identity / 1 tanh (GaussianNetwork.squash); soft 1 = SoftGaussianNetwork (tanh, its own logp form)
 *   action_out f32 (d x K x n) = squash(z); logp_out f32 (K x n), nullable (`is_return_log_prob = false`)
 * rlhip_gaussian_head_logp_f32 is the `(model)(state, action)` call: log-probability of given (squashed) actions. */
int32_t rlhip_gaussian_head_sample_f32(const float* mu, const float* raw_sigma, int64_t d, int64_t n, int64_t K,
                                       float min_sigma, float max_sigma, int32_t squash, int32_t soft,
                                       uint64_t seed, uint32_t env_id_base, uint32_t step, float* action_out,
                                       float* logp_out, rlhip_stream_t stream);
int32_t rlhip_gaussian_head_logp_f32(const float* mu, const float* raw_sigma, const float* action, int64_t d,
                                     int64_t n, int64_t K, float min_sigma, float max_sigma, int32_t squash,
                                     int32_t soft, float* logp_out, rlhip_stream_t stream);
/* CovGaussianNetwork  RLCore/src/utils/networks.jl:221-381 and the rest of RLCore/src/utils/distributions.jl (csrc/cov_heads.hip).
 * All arrays f32, column-major: mu (da x n), chol_vec (nv x n) with nv = da (da + 1) / 2 (the output of the Sigma sub-network),
 * L (da x da x n), actions (da x K x n) -- element (k, j, i) at (i K + j) da + k --, log-probabilities (K x n).  da in 1 ... 16,
 * K >= 1, n = 0 is a no-op; anything else returns RLHIP_EINVAL.  Noise: draw k + da*j of (seed, env_id_base + i, step) of the Philox
 * NORMAL stream, as for the heads above.  Order of operations (all f32, no contraction):
 *   softplusbeta(x) = logf(expf(x / 10.0f) + 1.0f) * 10.0f;  L[i,i] = softplusbeta(v) + 1.0e-5f;  L[i,j] = v (i > j);  0 above;
 *       1-based vector index of (i, j) = ((2 da - j)(j - 1)) / 2 + i
 *   sample:  acc = L[i,1] eps[1];  acc = acc + L[i,j] eps[j] (j = 2 ... i);  z[i] = mu[i] + acc
 *   solve:   t = x[i] - mu[i];  t = t - L[i,j] y[j] (j = 1 ... i - 1 ascending);  y[i] = t / L[i,i]
 *   logpdf:  ld = 0 + sum_i logf(L[i,i]) ascending;  logdet = 2 ld;  ss = 0 + sum_i y[i] y[i] ascending;
 *            out = -(((float)da * log2pi + logdet) + ss) / 2       (log2pi = log(2f0 pi), logdetLorU's device method :76)
 * Only the lower triangle of a dense L is read. */
/* vec_to_tril(cholesky_vec, da)  networks.jl:359-381 */
int32_t rlhip_vec_to_tril_f32(const float* chol_vec, int64_t da, int64_t n, float* L_out, rlhip_stream_t stream);
/* mvnormlogpdf(mu, L, x), the batch form  distributions.jl:46-50, :62-66 (logdetLorU :75-77): out f32 (K x n) */
int32_t rlhip_mvnormlogpdf_f32(const float* mu, const float* L, const float* x, int64_t da, int64_t K, int64_t n, float* out,
                               rlhip_stream_t stream);
/* (model::CovGaussianNetwork)(rng, state; is_sampling = true[, is_return_log_prob = true]) networks.jl:247-272 (K = 1) and
 * (model)(rng, state, action_samples::Int) :300-312 (K > 1) on the outputs of the mu / Sigma sub-networks, ONE launch: vec_to_tril,
 * the draws and z = mu + L eps, then mvnormlogpdf(mu, L, z) -- byte for byte what rlhip_vec_to_tril_f32, the product with the same
 * draws and rlhip_mvnormlogpdf_f32 give.  logp_out (K x n) and L_out (da x da x n) are nullable. */
int32_t rlhip_cov_gaussian_head_sample_f32(const float* mu, const float* chol_vec, int64_t da, int64_t n, int64_t K,
                                           uint64_t seed, uint32_t env_id_base, uint32_t step, float* action_out,
                                           float* logp_out, float* L_out, rlhip_stream_t stream);
/* (model::CovGaussianNetwork)(state, action)  networks.jl:327-343: vec_to_tril and mvnormlogpdf(mu, L, action) in one launch;
 * L_out nullable */
int32_t rlhip_cov_gaussian_head_logp_f32(const float* mu, const float* chol_vec, const float* action, int64_t da, int64_t n,
                                         int64_t K, float* logp_out, float* L_out, rlhip_stream_t stream);
/* normkldivergence(mu1, s1, mu2, s2)  distributions.jl:137-139, elementwise over n:
 *   ((logf(s2) - logf(s1)) + (s1 s1 + (mu1 - mu2)(mu1 - mu2)) / (2 (s2 s2))) - 0.5f */
int32_t rlhip_normkldivergence_f32(const float* mu1, const float* s1, const float* mu2, const float* s2, int64_t n, float* out,
                                   rlhip_stream_t stream);
/* diagnormkldivergence(mu1, s1, mu2, s2)  distributions.jl:117-124: arrays (d x n) column-major, out f32[n] (any d >= 1, as in
 * diagnormlogpdf).  v = s s;  logdet = sum logf(v2) - sum logf(v1);  trace = sum v1 / v2;  sq = sum ((mu2 - mu1)(mu2 - mu1)) / v2
 * (every sum from 0, ascending);  out = (((logdet - (float)d) + trace) + sq) / 2 */
int32_t rlhip_diagnormkldivergence_f32(const float* mu1, const float* s1, const float* mu2, const float* s2, int64_t d,
                                       int64_t n, float* out, rlhip_stream_t stream);
/* mvnormkldivergence(mu1, L1, mu2, L2)  distributions.jl:88-109, out f32[n].  The reference's dense inverses and products are
 * replaced by the equal closed form on triangular solves:  logdet = 2 ld(L2) - 2 ld(L1);  trace = 0 + sum_c sum_{i >= c} w[i,c]^2
 * with w[:,c] = L2 \ L1[:,c] (columns ascending, rows ascending inside a column, the solve of column c starting at row c);
 * sq = sum_i (L2 \ (mu2 - mu1))[i]^2;  out = (((logdet - (float)da) + trace) + sq) / 2 */
int32_t rlhip_mvnormkldivergence_f32(const float* mu1, const float* L1, const float* mu2, const float* L2, int64_t da, int64_t n,
                                     float* out, rlhip_stream_t stream);
/* The pullbacks of the functions above (csrc/cov_heads_grad.hip): the reference introduces them as "GPU automatic differentiable"
 * versions and its users (MPO) differentiate through every one.  A cotangent has the shape of the forward output, a gradient the
 * shape of the forward input; every output pointer is nullable and its work is skipped; inputs must not be NULL; da in 1 ... 16 for
 * every entry, K >= 1, n = 0 is a no-op; anything else returns RLHIP_EINVAL.  All f32, no contraction, no atomics; the sums over the
 * K samples of a state run in ascending k, sequentially, in one lane, so a result does not depend on the launch geometry.
 *
 * Pullback of mvnormlogpdf(mu, L, x)  distributions.jl:46-66; dlogp (K x n).  Per state, k = 1 ... K ascending:
 *   y = L \ (x_k - mu)     the forward solve above
 *   u = L^T \ y            columns c = da ... 1: u[c] = t[c] / L[c,c]; then t[r] = t[r] - L[c,r] u[c] for r < c
 *   gu[r] = g_k u[r];  dx_k[r] = -gu[r];  dmu[r] = 0 + sum_k gu_k[r];  S[r,c] = 0 + sum_k gu_k[r] y_k[c] (r >= c);  gs = 0 + sum_k g_k
 *   dL[r,c] = S[r,c] (r > c);  dL[c,c] = S[c,c] - gs / L[c,c];  dL_out is dense (da x da x n) with +0 above the diagonal */
int32_t rlhip_mvnormlogpdf_bwd_f32(const float* mu, const float* L, const float* x, const float* dlogp, int64_t da, int64_t K,
                                   int64_t n, float* dmu_out, float* dL_out, float* dx_out, rlhip_stream_t stream);
/* Pullback of vec_to_tril(cholesky_vec, da)  networks.jl:359-381: dvec = dL[r,c] below the diagonal and
 * dL[c,c] * (1.0f / (1.0f + expf(-(v / 10.0f)))) on it (the derivative of softplusbeta in the form that stays finite where
 * expf(v / 10) overflows).  Only the lower triangle of dL is read. */
int32_t rlhip_vec_to_tril_bwd_f32(const float* chol_vec, const float* dL, int64_t da, int64_t n, float* dvec_out,
                                  rlhip_stream_t stream);
/* Pullback of (model::CovGaussianNetwork)(state, action)  networks.jl:327-343 onto the outputs of the mu / Sigma sub-networks, ONE
 * launch: byte for byte what rlhip_vec_to_tril_f32 -> rlhip_mvnormlogpdf_bwd_f32 -> rlhip_vec_to_tril_bwd_f32 give, without a dense L
 * or dL in memory.  The sampling calls need no pullback of their own: the reference draws z under ignore_derivatives
 * (networks.jl:255, :306), so the gradient of their log-probability is this call with action = the sampled z. */
int32_t rlhip_cov_gaussian_head_logp_bwd_f32(const float* mu, const float* chol_vec, const float* action, const float* dlogp,
                                             int64_t da, int64_t n, int64_t K, float* dmu_out, float* dvec_out,
                                             rlhip_stream_t stream);
/* Pullback of mvnormkldivergence(mu1, L1, mu2, L2)  distributions.jl:88-109; dout f32[n] = g.  Per state:
 *   m = L2 \ (mu2 - mu1);  q = L2^T \ m;  dmu2[r] = g q[r];  dmu1[r] = -(g q[r]);  W[r,j] = q[r] m[j] (r >= j)
 *   for c = 1 ... da:  a = L2 \ L1[:,c] from row c (the rows above are +0);  p = L2^T \ a (all rows);
 *       dL1[r,c] = g p[r] (r > c);  dL1[c,c] = g (p[c] - 1.0f / L1[c,c]);  W[r,j] = W[r,j] + p[r] a[j] for c <= j <= r
 *   dL2[r,j] = g (-W[r,j]) (r > j);  dL2[j,j] = g (1.0f / L2[j,j] - W[j,j]);  dL1, dL2 dense with +0 above the diagonal */
int32_t rlhip_mvnormkldivergence_bwd_f32(const float* mu1, const float* L1, const float* mu2, const float* L2, const float* dout,
                                         int64_t da, int64_t n, float* dmu1_out, float* dL1_out, float* dmu2_out, float* dL2_out,
                                         rlhip_stream_t stream);
/* Pullback of diagnormkldivergence(mu1, s1, mu2, s2)  distributions.jl:117-124; dout f32[n], g the column's.  Per component, with
 * a = s1, b = s2, dm = mu2 - mu1, v1 = a a, v2 = b b, w = dm / v2:
 *   dmu2 = g w;  dmu1 = -(g w);  ds1 = g (a / v2 - 1.0f / a);  ds2 = g (1.0f / b - (v1 + dm dm) / (v2 b)) */
int32_t rlhip_diagnormkldivergence_bwd_f32(const float* mu1, const float* s1, const float* mu2, const float* s2, const float* dout,
                                           int64_t d, int64_t n, float* dmu1_out, float* ds1_out, float* dmu2_out, float* ds2_out,
                                           rlhip_stream_t stream);
/* Pullback of normkldivergence(mu1, s1, mu2, s2)  distributions.jl:137-139, elementwise; dout f32[n].  dm = mu1 - mu2, v2 = b b,
 * w = dm / v2:  dmu1 = g w;  dmu2 = -(g w);  ds1 = g (a / v2 - 1.0f / a);  ds2 = g (1.0f / b - (a a + dm dm) / (v2 b)) */
int32_t rlhip_normkldivergence_bwd_f32(const float* mu1, const float* s1, const float* mu2, const float* s2, const float* dout,
                                       int64_t n, float* dmu1_out, float* ds1_out, float* dmu2_out, float* ds2_out,
                                       rlhip_stream_t stream);
/* The pullbacks of normlogpdf / diagnormlogpdf and of the diagonal Gaussian heads (csrc/heads_grad.hip): the reference introduces both
 * densities as "GPU automatic differentiable" (distributions.jl:14, :26), differentiates GaussianNetwork through its log-probabilities
 * and SoftGaussianNetwork through its actions and its log-probabilities (the reparameterisation trick, networks.jl:127-128).  Layouts as
 * in the forward entries: mu, raw_sigma (d x n) column-major, actions (d x K x n) with element (k, j, i) at (i K + j) d + k, dlogp (K x n).
 * d in 1 ... 64, K >= 1, n = 0 is a no-op; anything else returns RLHIP_EINVAL before any device work.  Inputs must not be NULL; every
 * gradient output is nullable and its work is skipped.  All f32, no contraction, no atomics; every sum over the K samples of a state runs
 * in ascending j, sequentially, in one lane, so a result does not depend on the launch geometry.  g is the upstream cotangent.
 *   sg = clamp(raw, lo, hi);  pass = !(raw > hi) && !(raw < lo) (inclusive bounds, a NaN passes: the reference's clamp rule);
 *   s = sg + 1.0e-8f;  draw_sigma = pass ? dsg : +0.0f -- a select, never a product: a non-finite dsg at a clamped component gives 0,
 *   as Julia's `delta * false` does.
 *
 * Pullback of normlogpdf(mu, sigma, x)  distributions.jl:18-21, elementwise over n; dout f32[n].  s = sigma + 1.0e-8f:
 *   z = (x - mu) / s;  w = z / s;  dmu = g w;  dx = -(g w);  dsigma = g ((z z - 1.0f) / s) */
int32_t rlhip_normlogpdf_bwd_f32(const float* mu, const float* sigma, const float* x, const float* dout, int64_t n, float* dmu_out,
                                 float* dsigma_out, float* dx_out, rlhip_stream_t stream);
/* Pullback of diagnormlogpdf(mu, sigma, x)  distributions.jl:31-34; arrays (d x n), dout f32[n], g the column's.  s = sigma + 1.0e-8f:
 *   v = s s;  e = x - mu;  w = e / v;  dmu = g w;  dx = -(g w);  dsigma = g (((e e) / v - 1.0f) / s)
 * The derivative of log(prod(v)) is taken in its closed form 2 / s.  Where prod(v) overflows or underflows the forward value is already
 * +-Inf; the closed form stays finite there, while the reference's automatic derivative (through 1 / prod(v)) would not. */
int32_t rlhip_diagnormlogpdf_bwd_f32(const float* mu, const float* sigma, const float* x, const float* dout, int64_t d, int64_t n,
                                     float* dmu_out, float* dsigma_out, float* dx_out, rlhip_stream_t stream);
/* Pullback of (model)(state, action)  networks.jl:110-116, :195-201 onto the outputs of the mu / sigma sub-networks.
 *   z = (soft || squash) ? atanhf(a) : a.  The given actions are data: they get no gradient and the tanh correction is constant.
 *   soft = 0 (the diagnormlogpdf form):  e = z - mu;  v = s s;
 *       dmu[k] = 0 + sum_j g_j (e / v);  dsg[k] = 0 + sum_j g_j (((e e) / v - 1.0f) / s)
 *   soft = 1 (the normlogpdf form):  zz = (z - mu) / s;  w = zz / s;
 *       dmu[k] = 0 + sum_j g_j w;  dsg[k] = 0 + sum_j g_j ((zz zz - 1.0f) / s) */
int32_t rlhip_gaussian_head_logp_bwd_f32(const float* mu, const float* raw_sigma, const float* action, const float* dlogp, int64_t d,
                                         int64_t n, int64_t K, float min_sigma, float max_sigma, int32_t squash, int32_t soft,
                                         float* dmu_out, float* draw_sigma_out, rlhip_stream_t stream);
/* Pullback of the sampling calls  networks.jl:64-100, :153-185.  The launch REGENERATES the draws: eps = draw k + d j of
 * (seed, env_id_base + i, step) and z = mu + sg eps, bit for bit the forward's, so a caller keeps only mu and raw_sigma between forward
 * and backward -- and for a tanh-squashed head this is the only exact route: tanhf saturates to +-1 at |z| of about 9, where atanhf of
 * the saved action is +-Inf.
 *   soft = 0 (GaussianNetwork): z is a constant (ignore_derivatives :69, :94); the soft = 0 sums above at the regenerated z.  dact must
 *       be NULL (the actions carry no gradient; a non-NULL dact is RLHIP_EINVAL), dlogp is required.
 *   soft = 1 (SoftGaussianNetwork, reparameterised): dact (d x K x n) and dlogp are nullable, at least one is required.
 *       t = tanhf(z);  zz = (z - mu) / s;  w = zz / s;
 *       dz = 0;  if dlogp: dz = g (2.0f t - w);  if dact: dz = dz + da (1.0f - t t)
 *       dmu[k] = 0 + sum_j ((dlogp ? g w : 0) + dz);  dsg[k] = 0 + sum_j ((dlogp ? g ((zz zz - 1.0f) / s) : 0) + dz eps)
 *       (2 t is the exact derivative of the reference's correction -2 (log 2 - z - softplus(-2 z))) */
int32_t rlhip_gaussian_head_sample_bwd_f32(const float* mu, const float* raw_sigma, int64_t d, int64_t n, int64_t K, float min_sigma,
                                           float max_sigma, int32_t squash, int32_t soft, uint64_t seed, uint32_t env_id_base,
                                           uint32_t step, const float* dact, const float* dlogp, float* dmu_out,
                                           float* draw_sigma_out, rlhip_stream_t stream);
/* Flux.Losses.huber_loss(q, target; delta) mean-aggregated -> loss_out f32[1]; dq (nullable) = dL/dq */
int32_t rlhip_huber_f32(const float* q, const float* target, int64_t n, float delta, float* loss_out,
                        float* dq, rlhip_stream_t stream);
/* DQN target G = r + gamma * (1 - terminal) * max_a' Qt(s', a')  (qt_next strides as in selection) */
int32_t rlhip_td_target_f32(const float* qt_next, int64_t na, int64_t n, int64_t k_stride,
                            int64_t i_stride, const float* reward, const uint8_t* terminal,
                            float gamma, float* target, rlhip_stream_t stream);

/* n-step form (R = r + gamma^n (1 - t) max_a' Qt(s_{i+n}, a')): reward = the n-step returns, terminal = any terminal
 * inside the window (both from rlhip_ring_fold_nstep), gamma^n = rlhip_gamma_pow(gamma, n_step) */
int32_t rlhip_td_target_n_f32(const float* qt_next, int64_t na, int64_t n, int64_t k_stride,
                              int64_t i_stride, const float* reward, const uint8_t* terminal,
                              float gamma, int32_t n_step, float* target, rlhip_stream_t stream);
/* gamma^n as the n-step learners use it: evaluated in Float64 and rounded once (Julia's `gamma^n` for a Float32 gamma) */
float rlhip_gamma_pow(float gamma, int32_t n);

/* -------------------------------------------------------------------------- replay ring -- */
/* CircularArraySARTSTraces(; capacity, state = Float32 => (obs_dim, n_env), action = Int32 => (n_env,),
 * reward = Float32 => (n_env,), terminal = Bool => (n_env,)) resident in HBM
 *   (un-vendored ReinforcementLearningTrajectories 0.4; call sites RLCore/policies/agent/agent_base.jl:45-59,
 *    RLCore/test/policies/q_based_policy.jl:41-47).
 * One frame = one vec-step.  state has capacity+1 frames (next_state[i] = state[i+1]), the other traces
 * capacity frames.  Head/length counters are HOST fields updated by the push calls (they are pure
 * functions of the push count, so no device sync is ever needed to know them).
 * elem_bytes: 4 (Float32 observations) or 1 (UInt8 frames, e.g. 84x84x4 Atari stacks).
 *
 * Two storage layouts (`layout`, set by rlhip_ring_init; rlhip_ring_layout() returns it):
 *   RLHIP_RING_FRAMES   every trace as pushed: state[(slot * obs_dim + k) * n_env + e] (capacity + 1 slots), action / reward /
 *                       terminal[slot * n_env + e] (capacity slots) -- UInt8 frames and Float32 observations with > 4 components.
 *   RLHIP_RING_RECORDS  Float32 observations with <= 4 components (the classic-control envs; what the fused DQN learners take):
 *                       `state` holds (capacity + 1) * n_env RECORDS of 64 bytes (one cache line = one fabric request),
 *                           record[slot * n_env + e] = { float s[4]; int32 action; float reward; uint32 terminal; uint32 spare;
 *                                                        float s_next[4]; uint32 pad[4] },
 *                       the whole transition (s, a, r, t, s') that LEAVES the state of that slot: a sampled transition is one
 *                       line (round 4: five; measured in csrc/ring_device.h).  push!(trajectory, (state = s', action, reward,
 *                       terminal)) completes the previous slot's record and opens the next (s = s': a state is stored twice).
 *                       Logical transition i lives in slot (head_sa + i) mod (capacity + 1); the newest slot holds a state only.
 *                       `action`, `reward`, `terminal` are NULL (a strided view for a host: words 4 / 5 / 6 of each 16-word
 *                       record, s_next at words 8..11).  s[k >= obs_dim] = s_next[k >= obs_dim] = 0.
 * rlhip_ring_state_bytes() is the size of the `state` allocation for either layout (64-byte aligned for records). */
#define RLHIP_RING_FRAMES 0
#define RLHIP_RING_RECORDS 2 /* (1 was ABI 1's transition-major state trace) */
typedef struct {
    int64_t capacity, n_env, obs_dim;
    int64_t head_sa, len_sa, head_rt, len_rt; /* host-side ring counters (head_rt / len_rt count the LOGICAL action / reward /
                                               * terminal traces in both layouts: lengths, sampler range, sum-tree keys) */
    int32_t elem_bytes;
    int32_t layout;    /* RLHIP_RING_FRAMES | RLHIP_RING_RECORDS */
    void* state;       /* FRAMES: (capacity + 1) * obs_dim * n_env elements; RECORDS: (capacity + 1) * n_env * 64 bytes */
    int32_t* action;   /* FRAMES: capacity * n_env; RECORDS: NULL */
    float* reward;     /* FRAMES: capacity * n_env; RECORDS: NULL */
    uint8_t* terminal; /* FRAMES: capacity * n_env; RECORDS: NULL */
} rlhip_ring;

int64_t rlhip_ring_state_bytes(int64_t capacity, int64_t n_env, int64_t obs_dim, int32_t elem_bytes);
int32_t rlhip_ring_layout(const rlhip_ring* rb_host);
/* action / reward / terminal: device arrays for RLHIP_RING_FRAMES, NULL for RLHIP_RING_RECORDS (= elem_bytes 4 and obs_dim <= 4;
 * anything else is RLHIP_EINVAL: a host written for ABI 1 fails here instead of reading transposed data) */
int32_t rlhip_ring_init(rlhip_ring* rb_host, int64_t capacity, int64_t n_env, int64_t obs_dim,
                        int32_t elem_bytes, void* state, int32_t* action, float* reward,
                        uint8_t* terminal);
/* push!(trajectory, (state = s,))   Agent PreEpisodeStage  agent_base.jl:45-47.
 * Protocol (checked before any counter of rb_host moves: a rejected call leaves the ring unchanged): the FIRST push is a state, every
 * later push a transition -- rlhip_ring_push_transition[_maxpool] without an open state and rlhip_ring_push_state[_maxpool] while
 * one is open (len_sa == len_rt + 1) return RLHIP_EINVAL.  The reference's EpisodesBuffer accepts a second PreEpisodeStage push by
 * padding the (a, r, t) slot between the two episodes and excluding it from sampling; this ring has no such mask.  Vector envs
 * auto-reset (one PreEpisode push per run); a single-instance host pushes the post-reset observation as s' of the terminal
 * transition (which `terminal = 1` cuts from the TD target and from stacked histories). */
int32_t rlhip_ring_push_state(rlhip_ring* rb_host, const void* obs, rlhip_stream_t stream);
/* push!(trajectory, (state = s', action = a, reward = r, terminal = t))   PostActStage  :56-59 */
int32_t rlhip_ring_push_transition(rlhip_ring* rb_host, const void* next_obs, const int32_t* action,
                                   const float* reward, const uint8_t* terminal,
                                   rlhip_stream_t stream);
/* length(trajectory.container) */
int64_t rlhip_ring_length(const rlhip_ring* rb_host);
/* BatchSampler(batch): flat indices j = frame_logical * n_env + env, uniform with replacement.
 * idx_out: i64[batch] device.  Philox(seed, idx = b, blk 0, t = draw_ctr, SAMPLER): ((w0:w1) * total) >> 64 */
int32_t rlhip_ring_sample_indices(const rlhip_ring* rb_host, int64_t batch, uint64_t seed,
                                  uint32_t draw_ctr, int64_t* idx_out, rlhip_stream_t stream);
/* `for batch in trajectory`: gather (s, a, r, t, s') for flat indices.  Outputs SoA: s, s_next
 * (obs_dim x batch) elements; a i32[batch]; r f32[batch]; term u8[batch].  LDS-staged index tile. */
/* Output layout of s / s_next: component-major SoA (obs_dim x batch) in general; FRAME-major
 * (batch x obs_dim, every frame contiguous) when rlhip_ring_gather_is_frame_major() != 0, i.e. for
 * n_env == 1 rings whose frame is >= 1024 bytes and a multiple of 16 bytes (image observations). */
int32_t rlhip_ring_gather_is_frame_major(const rlhip_ring* rb_host);
int32_t rlhip_ring_gather(const rlhip_ring* rb_host, const int64_t* idx, int64_t batch, void* s,
                          int32_t* a, float* r, uint8_t* term, void* s_next,
                          rlhip_stream_t stream);

/* n-step transitions -- NStepBatchSampler(n, gamma, batchsize) of RLTrajectories 0.4 (un-vendored: PARITY UNPINNED; the published
 * algorithm is restated in oracle/rlo_buffer.c).  The fold serves record rings (Float32 observations with <= 4 components); frame rings
 * have rlhip_ring_gather_nstep / rlhip_ring_gather_stacked_nstep below, and the index draw serves both.
 *   rlhip_ring_sample_indices_nstep   inds = rand(rng, 1:(length - n + 1), batchsize) per env: flat logical START indices
 *                                     (li * n_env + e with li <= length - n_step), same Philox draw as rlhip_ring_sample_indices.
 *   rlhip_ring_fold_nstep             for every start index the window li .. li + ns - 1 (ns = n_step, or up to and including the
 *                                     first terminal step) folded into ONE transition {s_li, a_li, R, any(terminal), s_{li + ns}},
 *                                     R = discount_rewards_reduced(rewards[window], gamma) (RLCore/src/utils/basic.jl:237-319:
 *                                     r_0 + gamma (r_1 + gamma (...)), Float32), written as the `batch` records of slot 0 of `folded`
 *                                     -- a record ring from rlhip_ring_init(capacity >= 1, n_env = batch, obs_dim) whose host
 *                                     counters are set to "one stored vec-step".  Every DQN gradient entry point then runs unchanged:
 *                                         rlhip_dqn_grad_idx_f32(folded, ..., idx = iota_out, gamma = rlhip_gamma_pow(gamma, n_step), ...)
 *                                     (likewise _idx_w_, rlhip_dqn3_grad[_w]_f32 with idx).  iota_out (nullable): 0 .. batch - 1.
 *                                     n_step in 1..32; n_step = 1 reproduces the stored transitions bit for bit. */
int32_t rlhip_ring_sample_indices_nstep(const rlhip_ring* rb_host, int64_t batch, int32_t n_step, uint64_t seed,
                                        uint32_t draw_ctr, int64_t* idx_out, rlhip_stream_t stream);
int32_t rlhip_ring_fold_nstep(const rlhip_ring* rb_host, const int64_t* idx, int64_t batch, int32_t n_step, float gamma,
                              rlhip_ring* folded_host, int64_t* iota_out, rlhip_stream_t stream);

/* Double DQN targets (`is_enable_double_DQN` of the removed DQNLearner) as a batch fold of the same shape.  For
 * every flat logical index the record {s, a, r, t, s'} is read, a* = findmax(Q_online(s')) (first maximum wins,
 * RLCore/src/utils/basic.jl:91-120), y = r + gamma_eff * (1 - t) * Qt(s')[a*], and {s, a, y, terminal = 1, s'} is written as record b
 * of slot 0 of `folded` (the convention of rlhip_ring_fold_nstep: one stored vec-step of `batch` envs; iota_out, nullable, receives
 * 0 .. batch - 1).  Every DQN gradient entry point then runs UNCHANGED on (folded, idx = iota_out) and computes the Double DQN update.
 * Why that is exact: the target line of every gradient kernel (and of oracle/rlo_learn.c) is G = r + gamma * cont * mx with
 * cont = 1 - terminal, built with -ffp-contract=off; with the reward field = y and terminal = 1 it gives G = y + 0 = y bit for bit,
 * for any finite Qt(s') and whatever gamma the gradient call is given.
 *   rlhip_dqn_fold_double_f32    two-layer nets (hidden a multiple of 4, <= 256; na <= 4; obs_dim 2..4: what rlhip_dqn_grad_*_f32
 *                                takes).  One launch; `workspace` is unused (may be NULL).
 *   rlhip_dqn3_fold_double_f32   three-layer bf16 MFMA nets (hidden 128 / 256, the (obs_dim, na) pairs of rlhip_dqn3_plan_f32): s'
 *                                gathered into `workspace`, rlhip_dqn3_plan_f32 once per net, one select-and-write launch.
 *   rlhip_dqn_double_workspace_bytes   bytes of `workspace` (layers = 2: 0; layers = 3: s' | Q(s') | Qt(s')); -1 on bad arguments.
 * Record rings only.  `folded` may be the source ring itself when the source is an already folded ring and idx its iota -- the n-step
 * form: rlhip_ring_fold_nstep first, then this fold in place with gamma_eff = rlhip_gamma_pow(gamma, n_step); every record is read and
 * written by the same workgroup (two-layer) or lane (three-layer).  A -DRLHIP_BOUNDS_CHECK build validates idx first. */
int64_t rlhip_dqn_double_workspace_bytes(int64_t ns, int64_t h, int64_t na, int64_t batch, int32_t layers);
int32_t rlhip_dqn_fold_double_f32(const rlhip_ring* rb_host, int64_t h, int64_t na, int32_t act, const float* params,
                                  const float* target_params, const int64_t* idx, int64_t batch, float gamma_eff,
                                  rlhip_ring* folded_host, int64_t* iota_out, void* workspace, rlhip_stream_t stream);
int32_t rlhip_dqn3_fold_double_f32(const rlhip_ring* rb_host, int64_t h, int64_t na, int32_t act, const float* params,
                                   const uint16_t* packed, const float* target_params, const uint16_t* target_packed,
                                   const int64_t* idx, int64_t batch, float gamma_eff, rlhip_ring* folded_host, int64_t* iota_out,
                                   void* workspace, rlhip_stream_t stream);

/* DuelingNetwork(base, val, adv) Q-networks (RLCore/src/utils/networks.jl:510-522: Q = val .+ adv .- mean(adv, dims = 1), `val` and
 * `adv` single Dense layers) as a PARAMETER fold.  The combine is linear in the head: with
 *     W2e[a, :] = Wval + Wadv[a, :] - mean_a'(Wadv[a', :]),   b2e[a] = bval + badv[a] - mean_a'(badv[a'])
 * a plain Dense(h, na) head computes the dueling Q, so every plan / act / gradient / Double DQN fold entry point serves a dueling net
 * UNCHANGED on the effective plain vector.  Why the gradient is exact: dL/dh = sum_a W2e[a, :] dQ_a is the same expression in both
 * forms, so dW1, db1 and the hidden-layer gradients of the plain kernels are the dueling net's as they stand, and the head maps back by
 * the chain rule, dWval = sum_a dW2e[a, :], dWadv[a, :] = dW2e[a, :] - mean_a'(dW2e[a', :]), the biases by the same two rules.  The fold
 * perturbs Q at rounding level only (measured <= 4.3e-7 of max|Q|); Huber's gradient and the max target are continuous in Q.
 * Flat dueling vector: [ plain layout (rlhip_mlp2_nparams / rlhip_mlp3_nparams) with (Wadv, badv) as its last Dense | Wval (h) |
 * bval (1) ]; the last Dense is W (na x h, column-major) followed by b (na).  Arithmetic (Float32, no contraction, bit-exact against
 * tests/dueling_ref.py): per hidden unit j the left-folded sum s = ((x0 + x1) + x2) + x3 over the na rows, mean = s / float(na) (a
 * true division), W2e[a, j] = (Wval[j] + Wadv[a, j]) - mean; unfold: dWval[j] = s over the dW2e rows, dWadv[a, j] = dW2e[a, j] - s / na.
 *   rlhip_dueling_nparams          plain nparams + h + 1 (-1 on bad arguments); layers = 2 or 3.
 *   rlhip_dueling_fold_f32         one launch: copies everything in front of the head, writes the effective head.  (duel2, eff2):
 *                                  an optional second net (the target), both NULL or both given.  eff != duel.
 *   rlhip_dueling_unfold_grad_f32  one launch: copies the base gradients, writes dWadv, dbadv, dWval, dbval.
 * 1 <= na <= 4, h >= 1; 16-byte copies when both pointers of a net are 16-byte aligned.  Optimiser state lives on the dueling vector:
 * unfold -> clip + Adam on the dueling vector -> fold (-> rlhip_mlp3_pack_bf16; the hidden W2 is the same in both vectors). */
int64_t rlhip_dueling_nparams(int64_t ns, int64_t h, int64_t na, int32_t layers);
int32_t rlhip_dueling_fold_f32(const float* duel, float* eff, const float* duel2, float* eff2, int64_t ns, int64_t h, int64_t na,
                               int32_t layers, rlhip_stream_t stream);
int32_t rlhip_dueling_unfold_grad_f32(const float* grad_eff, float* grad_duel, int64_t ns, int64_t h, int64_t na, int32_t layers,
                                      rlhip_stream_t stream);

/* Debugging aid ("a debug build that bounds-checks gather indices"; the reference's `traces[inds]` throws a
 * BoundsError): how many of the flat logical indices idx[0 .. batch) lie outside [0, length(trajectory) * n_env), and the position
 * of the first one (-1 if none).  One launch and a stream synchronisation: n_bad / first_bad are HOST pointers (first_bad may be
 * NULL).  A library built with -DRLHIP_BOUNDS_CHECK (RLHIP_EXTRA_FLAGS=-DRLHIP_BOUNDS_CHECK python .../build.py --force;
 * rlhip_ring_bounds_checked_build() = 1) runs this check inside every entry point that takes caller-supplied indices
 * (rlhip_ring_gather, rlhip_ring_gather_stacked, rlhip_ring_gather[_stacked]_nstep, rlhip_dqn_grad_idx[_w]_f32, rlhip_dqn3_grad[_w]_f32 with idx) and returns
 * RLHIP_EINVAL instead of reading outside the ring; the default build does not pay the synchronisation. */
int32_t rlhip_ring_check_indices(const rlhip_ring* rb_host, const int64_t* idx, int64_t batch, int64_t* n_bad,
                                 int64_t* first_bad, rlhip_stream_t stream);
int32_t rlhip_ring_bounds_checked_build(void);

/* ------------------------------------------------------- device-side episode hooks -- */
/* TotalRewardPerEpisode / BatchStepsPerEpisode / StepsPerEpisode (RLCore/src/core/hooks.jl:64-101, 146-196,
 * 202-231) without a per-step host read: one launch per vec-step (PostActStage) updates the per-instance
 * (steps, return) accumulators and appends one record per finished episode to a device log.
 * log_count keeps counting past log_capacity (records beyond it are dropped; the host can detect that). */
typedef struct {
    uint32_t vec_step; /* the vec-step in which the episode ended */
    uint32_t env;      /* instance index */
    int32_t steps;     /* episode length */
    int32_t pad;
    double total_reward;
} rlhip_episode_record;
int32_t rlhip_hook_episode_stats(const float* reward, const uint8_t* done, int64_t n, uint32_t vec_step,
                                 int32_t* steps_acc, double* return_acc, rlhip_episode_record* log,
                                 uint32_t log_capacity, uint32_t* log_count, rlhip_stream_t stream);

/* --------------------------------------- frame stacking at sample time, max-pool push -- */
/* StackFrames (RLCore/src/utils/stack_frames.jl:11-44) moved from the way in to the way out: the ring stores
 * single frames (n_env == 1), the gather assembles the n_stack-deep observations
 *   state stack of transition i = frames i-n+1 .. i,   next stack = i-n+2 .. i+1   (oldest first, newest last),
 * with all-zero frames before the episode start / before the oldest stored frame (what StackFrames holds after
 * reset!).  Outputs (batch, n_stack, frame) contiguous; a, r, term as rlhip_ring_gather.  n_stack <= 8. */
int32_t rlhip_ring_gather_stacked(const rlhip_ring* rb_host, const int64_t* idx, int64_t batch, int32_t n_stack,
                                  void* s, int32_t* a, float* r, uint8_t* term, void* s_next,
                                  rlhip_stream_t stream);
/* n-step transitions from FRAME rings (RLHIP_RING_FRAMES: UInt8 frames, Float32 observations with > 4 components) -- what
 * rlhip_ring_fold_nstep is for record rings, as a gather: one launch, the same two frames read per sample as the 1-step gather.
 * idx[b] = li * n_env + e with 0 <= li < length (the convention of rlhip_ring_gather): ANY stored transition is a legal start, so the
 * indices of rlhip_ring_sample_indices_nstep and of a 1-step prioritized draw (rlhip_ring_sample_prioritized) both feed the call.
 * The window is li .. li + ns - 1 of env e, ns = the smallest of n_step, k + 1 for the first k >= 0 with terminal[li + k] != 0, and
 * length - li: it stops at, and includes, the first terminal step and never reads past the newest stored transition.  Outputs:
 *     s = state frame li,  a = action[li],  term = (terminal[li + ns - 1] != 0),  s_next = state frame li + ns,
 *     ret = discount_rewards_reduced over the window (RLCore/src/utils/basic.jl:237-319) in Float32 from the window's end,
 *           gain = 0; for k = ns - 1 .. 0: gain = reward[li + k] + gamma * gain   (no contraction, this order, one lane),
 *     n_used (int32[batch], nullable) = ns: the discount of the caller's target is gamma^ns (rlhip_gamma_pow(gamma, ns)).
 *   rlhip_ring_gather_nstep          s / s_next laid out as rlhip_ring_gather lays them out for the same ring (component-major SoA;
 *                                    frame-major when rlhip_ring_gather_is_frame_major(), then with its 16-byte alignment condition).
 *   rlhip_ring_gather_stacked_nstep  s = stack(li), s_next = stack(li + ns), where stack(f) = frames f - n_stack + 1 .. f, oldest
 *                                    first, a member all zeros when its frame index is negative or a terminal transition lies among the
 *                                    transitions from that frame up to f - 1 (the rule of rlhip_ring_gather_stacked, whose
 *                                    preconditions and (batch, n_stack, frame) layout hold here).  Every source frame of the union of
 *                                    the two stacks is read once per sample.
 * n_step = 1 reproduces rlhip_ring_gather / rlhip_ring_gather_stacked byte for byte in s, a, term (for stored flags 0 / 1) and s_next;
 * ret == r then, but not byte for byte: a stored -0.0f comes back as +0.0f (r + gamma * 0), as it does from rlhip_ring_fold_nstep.
 * RLHIP_EINVAL before any launch: n_step outside 1..32, a record ring (use rlhip_ring_fold_nstep), an empty ring, NULL s / a / ret /
 * term / s_next / idx, the alignment conditions of the 1-step twins.  batch == 0 is RLHIP_OK.  A -DRLHIP_BOUNDS_CHECK build validates
 * idx first. */
int32_t rlhip_ring_gather_nstep(const rlhip_ring* rb_host, const int64_t* idx, int64_t batch, int32_t n_step, float gamma, void* s,
                                int32_t* a, float* ret, uint8_t* term, void* s_next, int32_t* n_used, rlhip_stream_t stream);
int32_t rlhip_ring_gather_stacked_nstep(const rlhip_ring* rb_host, const int64_t* idx, int64_t batch, int32_t n_stack, int32_t n_step,
                                        float gamma, void* s, int32_t* a, float* ret, uint8_t* term, void* s_next, int32_t* n_used,
                                        rlhip_stream_t stream);
/* AtariEnv.act! 2-frame max-pool `screens[1] .= max.(screens[1], screens[2])`
 * (RLEnvs/src/environments/3rd_party/atari.jl:104-107) fused into the push of a UInt8 frame. */
int32_t rlhip_ring_push_state_maxpool(rlhip_ring* rb_host, const void* screen1, const void* screen2,
                                      rlhip_stream_t stream);
int32_t rlhip_ring_push_transition_maxpool(rlhip_ring* rb_host, const void* screen1, const void* screen2,
                                           const int32_t* action, const float* reward,
                                           const uint8_t* terminal, rlhip_stream_t stream);

/* plan! + act! + push! of one DQN vec-step in ONE launch for the 2-layer Q-network (dqn_act.hip): bit-identical
 * to rlhip_dqn_plan_f32 -> rlhip_env_step (auto-reset) -> rlhip_ring_push_transition, whose ring counters it
 * advances the same way.  rlhip_dqn_act_supported: hidden in {64, 128, 256}, n <= 2^18, Float32 discrete env. */
int32_t rlhip_dqn_act_supported(int32_t kind, int64_t n, int64_t h);
int32_t rlhip_dqn_act_f32(int32_t kind, const void* env_cfg, const rlhip_env_state* st, int64_t n,
                          const float* params, int64_t h, int64_t na, int32_t act, double eps,
                          uint64_t explorer_seed, uint32_t explorer_step, uint64_t env_seed, uint32_t env_id_base,
                          rlhip_ring* rb_host, int32_t* actions, float* q_out, float* obs_out, float* last_obs,
                          rlhip_stream_t stream);
/* act! + push! in one launch for a policy whose plan! ran separately (the MFMA Q-network): actions i32[n] 0-based.
 * Bit-identical to rlhip_env_step(auto_reset = 1, last_obs, obs_out) followed by rlhip_ring_push_transition; the ring
 * counters advance as in that call.  Discrete Float32 CartPole / Pendulum / MountainCar. */
int32_t rlhip_env_act_push_f32(int32_t kind, const void* env_cfg, const rlhip_env_state* st, int64_t n,
                               const int32_t* actions, uint64_t env_seed, uint32_t env_id_base, rlhip_ring* rb,
                               float* obs_out, float* last_obs, rlhip_stream_t stream);

/* ------------------------------------- one-shot peer-to-peer all-reduce (multi-GPU learner) -- */
/* The exchange step of the sharded learner: SUM of the small flat gradient over the ranks, inside ONE
 * kernel on the caller's stream.  Each rank owns a comm buffer (uncached device memory, rlhip_p2p_comm_bytes(cap)
 * bytes, zero-initialised) which every peer maps through HIP IPC; rlhip_p2p_allreduce_f32 publishes the local vector,
 * waits for every rank's sequence flag and sums the buffers in rank order (bit-identical results on all ranks).
 * seq = 1, 2, 3, ... must advance by one per call on every rank.  A wait that exceeds timeout_polls sets
 * status_dev[0] = 1 (device or host-pinned memory) and overwrites `data` with NaN: an unreduced gradient must not
 * reach the optimiser silently.  These are the building blocks; hosts use rlhip_comm_* / rlhip_allreduce_grads below,
 * which own the buffers, validate the path on every rank and fall back to RCCL otherwise. */
int32_t rlhip_p2p_alloc(int64_t bytes, void** out);
int32_t rlhip_p2p_free(void* p);
int32_t rlhip_p2p_export(void* p, uint8_t handle_out[64]);
int32_t rlhip_p2p_import(const uint8_t handle[64], void** out);
int32_t rlhip_p2p_close(void* p);
int32_t rlhip_p2p_can_access(int32_t peer_device);                                  /* hipDeviceCanAccessPeer */
int32_t rlhip_p2p_probe(const void* p, int64_t byte_offset, uint32_t* value_out);   /* 4-byte D2H copy from a peer */
int64_t rlhip_p2p_comm_bytes(int64_t cap);
int32_t rlhip_p2p_allreduce_f32(float* data, int64_t n, int64_t cap, int32_t rank, int32_t world,
                                void* const* comm_bufs_host, uint32_t seq, int64_t timeout_polls,
                                int32_t* status_dev, rlhip_stream_t stream);

/* ------------------------------------ the sharded learner's collective behind the ABI -- */
/* SURVEY.md 8b/8e.  Replaces nothing in the reference (it has no Distributed / MPI / NCCL code); it is the exchange a
 * data-parallel `optimise!(::FluxApproximator, grad)` (RLCore/src/policies/learners/flux_approximator.jl:46) needs:
 * the SUM of the flat gradient over the ranks BEFORE clip_by_global_norm! (RLCore/src/utils/basic.jl:19-29).
 * The host moves two small blobs between its ranks with whatever byte transport it has (csrc/comm.hip header):
 *   rank 0: rlhip_comm_unique_id -> broadcast 128 B;  all: rlhip_comm_init;  all: rlhip_comm_export -> all-gather
 *   (64 B handle, device id);  all: rlhip_p2p_setup;  then rlhip_allreduce_grads per optimiser step.
 * rlhip_comm_init is a collective when unique_id_host != NULL (ncclCommInitRank on the CURRENT device; RCCL is
 * dlopen'ed here, not at library load).  unique_id_host = NULL creates a communicator without RCCL (the peer-to-peer
 * path only; e.g. several ranks sharing one GPU, which RCCL refuses).  cap = floats of the largest vector that takes
 * the peer-to-peer path.  rlhip_p2p_setup is a collective as well: it maps every peer's buffer, runs an exact
 * self-test and agrees on the verdict across ranks -- *active_out is the same on every rank; when it is 0
 * rlhip_comm_info().why says why and rlhip_allreduce_grads uses ncclAllReduce on the caller's stream.
 * rlhip_allreduce_grads: in-place SUM, enqueued on `stream`, bit-identical on every rank on the peer-to-peer path
 * (rank-order summation).  A peer that does not arrive within the timeout makes the call's result NaN and
 * rlhip_comm_check return RLHIP_ETIMEOUT (it reads a host-pinned word: no synchronisation).
 * Tear-down, two phases with a host-side barrier before each: barrier -> rlhip_comm_unmap (closes this rank's mappings of
 * the peers' buffers and its RCCL communicator) -> barrier -> rlhip_comm_destroy (frees the own, IPC-exported buffer: no
 * peer may still have it mapped).  rlhip_comm_destroy alone does both (world = 1, error paths). */
typedef void* rlhip_comm_t;
typedef struct rlhip_comm_desc {
    int32_t rank, world, device, p2p_active, rccl_active;
    uint32_t seq;          /* last peer-to-peer sequence number used */
    int64_t cap, timeout_polls;
    int32_t* status;       /* host-pinned, device-visible: [0] != 0 after a timeout */
    void* bufs[16];        /* every rank's exchange buffer as mapped in this process (rlhip_p2p_allreduce_f32 layout) */
    char why[256];         /* why the peer-to-peer path is not active ("ok" when it is) */
    char rccl_path[256];   /* the RCCL the process bound to ("" before the first use) */
} rlhip_comm_desc;
int32_t rlhip_comm_unique_id(uint8_t id_out_host[128]);
int32_t rlhip_comm_init(int32_t rank, int32_t world, const uint8_t* unique_id_host, int64_t cap,
                        rlhip_comm_t* comm_out);
int32_t rlhip_comm_export(rlhip_comm_t comm, uint8_t handle_out_host[64], int32_t* device_out);
int32_t rlhip_p2p_setup(rlhip_comm_t comm, const uint8_t* handles_host /* world x 64 B */,
                        const int32_t* devices_host /* world */, int32_t* active_out);
/* Switch the peer-to-peer path of this rank off (`why_host` is recorded for rlhip_comm_info): for a host that learns over its own
 * transport that another rank's set-up FAILED WITH AN ERROR (rlhip_comm_export / rlhip_p2p_setup returned non-zero there, so that
 * rank took no part in the agreement) -- every rank must then use the same transport.  Not needed after a clean
 * rlhip_p2p_setup: its verdict is already agreed across the ranks. */
int32_t rlhip_comm_disable_p2p(rlhip_comm_t comm, const char* why_host);
int32_t rlhip_allreduce_grads(rlhip_comm_t comm, float* grad, int64_t n, rlhip_stream_t stream);
int32_t rlhip_comm_check(rlhip_comm_t comm);
int32_t rlhip_comm_info(rlhip_comm_t comm, rlhip_comm_desc* out_host);
int32_t rlhip_comm_set_timeout(rlhip_comm_t comm, int64_t timeout_polls);
int32_t rlhip_comm_advance_seq(rlhip_comm_t comm, uint32_t n_steps);
int32_t rlhip_comm_unmap(rlhip_comm_t comm);
int32_t rlhip_comm_destroy(rlhip_comm_t comm);

/* ------------------------------------------------- one DQN vec-step as a single call -- */
/* One trip round the body of `_run` (RLCore/src/core/run.jl:52-70) for Agent{QBasedPolicy{DQN}} on the vector
 * env: plan! (q_based_policy.jl:30-32) -> act! -> push!(agent, PostActStage) (agent_base.jl:56-59) ->
 * optimise! (q_based_policy.jl:49; flux_approximator.jl:46; target_network.jl:70-88).  Enqueues exactly the
 * kernels of the per-step entry points, in the same order, so results are bit-identical to them.
 * The counters (explorer_step, draw_ctr, do_update, do_sync) are the host's: pure functions of the step count. */
typedef struct {
    int32_t kind;              /* 0 CartPole, 1 Pendulum (discrete), 2 MountainCar; Float32 state */
    const void* env_cfg;       /* rlhip_*_cfg (host) */
    const rlhip_env_state* st; /* device state arrays */
    int64_t n;                 /* env instances */
    uint64_t env_seed;
    uint32_t env_id_base;
    float* obs;                /* (obs_dim, n): current observation in, next observation out */
    float* last_obs;           /* (obs_dim, n) pre-reset observation of the step, may be NULL */
    rlhip_ring* ring;          /* host struct; its counters advance */
    int32_t layers;            /* 2: ns -> h -> na (dqn.hip); 3: ns -> h -> h -> na, h = 128 or 256 (dqn3.hip / ppo3w.hip, MFMA) */
    int64_t h, na;
    int32_t act;               /* 0 relu, 1 tanh */
    float* params;
    uint16_t* packed;          /* layers == 3 */
    float* target;
    uint16_t* target_packed;   /* layers == 3 */
    float *m, *v, *beta_pow;   /* Adam state */
    float lr, beta1, beta2, adam_eps, max_grad_norm, grad_scale;
    double eps;                /* get_eps(explorer, explorer_step) */
    uint64_t explorer_seed;
    uint32_t explorer_step;
    int64_t batch;
    float gamma, huber_delta;
    uint64_t sampler_seed;
    uint32_t draw_ctr;
    int32_t do_update;         /* run optimise! this step */
    int32_t do_sync;           /* target sync after this update */
    float rho;
    void* workspace;
    float *grad, *loss, *gn;   /* loss / gn: f32[1] device */
    int32_t* actions;          /* i32[n] out (0-based) */
    float* q;                  /* (na, n) out, may be NULL */
} rlhip_dqn_step_args;
int32_t rlhip_dqn_vec_step_f32(rlhip_dqn_step_args* args, rlhip_stream_t stream);

/* ------------------------- the same vec-step for folded learners (n-step, Double DQN, DuelingNetwork) -- */
/* The folded batch of a two-layer learner in ONE launch: what the per-stage learner issues as
 *     rlhip_ring_sample_indices[_nstep] -> rlhip_ring_fold_nstep (n_step > 1) -> rlhip_dqn_fold_double_f32 (double_dqn != 0)
 * (`NStepBatchSampler` of RLTrajectories 0.4 and `is_enable_double_DQN` of the removed DQNLearner; see those entries above), byte for
 * byte.  The lane that owns sample b draws its own flat logical start index (the Philox draw of rlhip_ring_sample_indices: same seed,
 * draw_ctr and sample slot; written to idx_out when given), walks the window up to and including the first terminal step
 * (R = discount_rewards_reduced, RLCore/src/utils/basic.jl:237-319, Float32, right to left; terminal = any(terminal); s' of the
 * window's last record; n_step = 1 reproduces the stored record) and, with double_dqn, replaces the reward by
 * y = R + gamma_eff * (1 - t) * Qt(s')[findmax(Q(s'))], gamma_eff = rlhip_gamma_pow(gamma, n_step), terminal = 1.  Record b of slot 0
 * of `folded` (a record ring of n_env = batch, not the source) is written as one 64-byte line, iota_out[b] = b, and the counters of
 * `folded` are set to "one stored vec-step".  With double_dqn == 0 the nets are not read: params / target_params may be NULL.
 * Record rings, obs_dim 2..4, h a multiple of 4 and <= 256, na <= 4, n_step 1..32, batch >= 1, at least n_step stored steps;
 * anything else is RLHIP_EINVAL before the launch.  The cost is a latency chain: n_step dependent record reads per sample, then the
 * two forwards out of LDS on one CU per 64-sample tile. */
int32_t rlhip_dqn_sample_fold_f32(const rlhip_ring* rb_host, int64_t batch, int32_t n_step, int32_t double_dqn, float gamma,
                                  uint64_t seed, uint32_t draw_ctr, int64_t h, int64_t na, int32_t act, const float* params,
                                  const float* target_params, rlhip_ring* folded_host, int64_t* idx_out, int64_t* iota_out,
                                  rlhip_stream_t stream);

/* One trip round the body of `_run` (RLCore/src/core/run.jl:52-70), as rlhip_dqn_vec_step_f32, for a learner whose batches are
 * folded: n-step targets, Double DQN targets, a DuelingNetwork (RLCore/src/utils/networks.jl:510-522) or any combination.  plan! +
 * act! + push! are those of rlhip_dqn_vec_step_f32.  optimise! (q_based_policy.jl:49) enqueues exactly what the per-stage learner
 * computes: the folded batch (two layers: rlhip_dqn_sample_fold_f32; three: rlhip_ring_sample_indices[_nstep],
 * rlhip_ring_fold_nstep, rlhip_dqn3_fold_double_f32, the latter in place on `folded` when n_step > 1), the unchanged gradient entry
 * point on (folded, iota) with gamma^n, then flux_approximator.jl:46 and target_network.jl:70-88: clip + Adam [+ pack] and on
 * do_sync Polyak [+ pack] -- for a dueling net unfold the gradient, clip + Adam on the dueling vector, fold it into base.params
 * [+ pack], and on do_sync Polyak on target_dueling, fold into base.target [+ pack].  Results are bit-identical to the per-stage
 * protocol.  With n_step == 1, double_dqn == 0 and a plain net the call IS rlhip_dqn_vec_step_f32(&base).  Every argument is
 * checked before the first launch: a refused call moves no counter. */
struct rlhip_dqn_fold_step_args_s { /* (a tagged struct with its typedef below: the first member is a struct, not a scalar) */
    rlhip_dqn_step_args base;      /* every field as documented there */
    int32_t n_step;                /* 1..32 */
    int32_t double_dqn;            /* 0 / 1 */
    rlhip_ring* folded;            /* record ring, capacity >= 1, n_env = base.batch; its counters are set to "one stored vec-step" */
    int64_t* idx;                  /* i64[batch] scratch */
    int64_t* iota;                 /* i64[batch] */
    float* td;                     /* f32[batch], may be NULL */
    void* fold_workspace;          /* rlhip_dqn_double_workspace_bytes(...) for layers == 3 && double_dqn; else may be NULL */
    /* dueling (all NULL for a plain net): base.params / base.target are then the EFFECTIVE vectors, base.m / base.v /
       base.beta_pow the Adam state of the DUELING vector */
    float* dueling_params;
    float* target_dueling;
    float* grad_dueling;           /* f32[rlhip_dueling_nparams] */
};
typedef struct rlhip_dqn_fold_step_args_s rlhip_dqn_fold_step_args;
int32_t rlhip_dqn_vec_step_fold_f32(rlhip_dqn_fold_step_args* args, rlhip_stream_t stream);

/* ------------------------------ the same vec-step for a learner over prioritized replay -- */
/* One trip round the body of `_run` (RLCore/src/core/run.jl:52-70), as rlhip_dqn_vec_step_fold_f32, for a learner whose trajectory is
 * `CircularPrioritizedTraces` of RLTrajectories 0.4 sampled by the prioritized `BatchSampler` (n_step == 1) or by `NStepBatchSampler`
 * over the masked tree (n_step > 1) -- the removed Zoo's PrioritizedDQN, with any of Double DQN targets, a DuelingNetwork and
 * importance-sampling weights (un-vendored: PARITY UNPINNED like the entries it composes).  It enqueues what the per-stage learner
 * enqueues, in the same order with the same arguments:
 *     plan! + act! + push!                as rlhip_dqn_vec_step_f32
 *     rlhip_ring_push_priority (n_step == 1) / rlhip_ring_push_priority_nstep            -- return here when !do_update
 *     rlhip_ring_sample_prioritized(ring, tree, batch, sampler_seed, draw_ctr, idx, key, prio) (n_step == 1) /
 *         rlhip_per_sample_fold_nstep_f32(..., idx, key, prio, folded, iota)
 *     rlhip_per_is_weights_f32(prio, batch, per_beta, is_weights)                         when per_beta > 0
 *     rlhip_dqn_fold_double_f32 / rlhip_dqn3_fold_double_f32                              when double_dqn: from the trajectory with idx
 *         into (folded, iota), or in place on (folded, iota) when n_step > 1
 *     the gradient entry point: on (folded, iota) with rlhip_gamma_pow(gamma, n_step) when n_step > 1 or double_dqn, on (ring, idx)
 *         with gamma otherwise; rlhip_dqn_grad_idx_w_f32 / rlhip_dqn3_grad_w_f32 with the weights, rlhip_dqn_grad_idx_f32 /
 *         rlhip_dqn3_grad_f32 without; td into fold.td
 *     rlhip_per_writeback_f32(tree, capacity * n_env, key, fold.td, batch, per_eps, per_alpha, priority_out)
 *     the tail of rlhip_dqn_vec_step_fold_f32 (clip + Adam [+ pack], on do_sync Polyak [+ pack]; the dueling vectors for a dueling net)
 * so results -- parameters, optimiser state, trajectory, tree -- are bit-identical to the per-stage protocol.  Every argument is
 * checked before the first launch (everything rlhip_dqn_vec_step_fold_f32 checks; a record ring; the network shapes of the gradient
 * entry points; tree non-NULL; default_priority > 0; per_eps, per_alpha, per_beta >= 0; n_step <= capacity; with do_update idx, key,
 * prio, fold.td and priority_out present, is_weights when per_beta > 0, priority_out not overlapping fold.td): a refused call moves
 * no counter.  (Entry points added, no layout or signature changed: RLHIP_ABI_VERSION stays 2.) */
struct rlhip_dqn_per_step_args_s {
    rlhip_dqn_fold_step_args fold; /* every field as documented there; fold.td = TD errors out, f32[batch], required when do_update */
    float* tree;                   /* the traces' sum-tree (rlhip_sumtree_nodes(capacity * n_env) floats) */
    float default_priority;        /* > 0 */
    float per_eps, per_alpha;      /* write-back value (|td| + eps)^alpha */
    float per_beta;                /* this update's beta (the host evaluates a schedule); 0: no importance-sampling weights */
    int64_t* key;                  /* i64[batch]: the drawn physical keys */
    float* prio;                   /* f32[batch]: their priorities */
    float* is_weights;             /* f32[batch]; required when per_beta > 0 */
    float* priority_out;           /* f32[batch]: the written-back priorities; must not overlap fold.td */
};
typedef struct rlhip_dqn_per_step_args_s rlhip_dqn_per_step_args;
int32_t rlhip_dqn_vec_step_per_f32(rlhip_dqn_per_step_args* args, rlhip_stream_t stream);

/* ------------------------------------------------------ 3-layer Q-network on the MFMA -- */
/* Chain(Dense(ns, 128, act), Dense(128, 128, act), Dense(128, na)) -- the blog's DQN model
 * (docs/homepage/blog/a_practical_introduction_to_RL.jl/index.html:15126-15128), forward(learner, x) =
 * model(x) (RLCore/src/policies/learners/flux_approximator.jl:43).  Flat f32 master parameters in
 * Flux.destructure order W1 (h x ns) | b1 | W2 (h x h) | b2 | W3 (na x h) | b3.  The hidden x hidden layer runs
 * on v_mfma_f32_32x32x16_bf16 (bf16 operands, f32 accumulate) from a packed bf16 copy of W2 in both operand
 * orders: uint16[rlhip_mlp3_packed_elems(h)], 16-byte aligned, refreshed by rlhip_mlp3_pack_bf16 after every
 * parameter update.  hidden must be 128 (dqn3.hip) or 256 (the streaming kernels of ppo3w.hip). */
int64_t rlhip_mlp3_nparams(int64_t ns, int64_t h, int64_t na);
int64_t rlhip_mlp3_packed_elems(int64_t h);
int32_t rlhip_mlp3_init_f32(float* params, int64_t ns, int64_t h, int64_t na, uint64_t seed, uint32_t net_id,
                            rlhip_stream_t stream);
int32_t rlhip_mlp3_pack_bf16(const float* params, int64_t ns, int64_t h, int64_t na, uint16_t* packed,
                             rlhip_stream_t stream);
/* plan!(QBasedPolicy, env) = forward + EpsilonGreedyExplorer (no tie-break), as rlhip_dqn_plan_f32.
 * actions may be NULL (pure forward: q_out (na x n)), q_out may be NULL. */
int32_t rlhip_dqn3_plan_f32(const float* params, const uint16_t* packed, int64_t ns, int64_t h, int64_t na,
                            int32_t act, const float* obs, int64_t n, double eps, uint64_t seed,
                            uint32_t env_id_base, uint32_t step, int32_t* actions, float* q_out,
                            rlhip_stream_t stream);
/* plan! + act! + push! of one DQN vec-step of the 3-layer Q-network (hidden 128) in ONE launch: rlhip_dqn3_plan_f32 followed by
 * rlhip_env_act_push_f32, bit for bit (the lane that selects env e's action goes on with its env step, auto-reset and ring push);
 * the 3-layer counterpart of rlhip_dqn_act_f32, used by rlhip_dqn_vec_step_f32.  obs: (ns, n) device -- this step's observation on
 * entry, the next one's on return.  Supported: the three classic-control envs with their discrete action sets, n <= 32768. */
int32_t rlhip_dqn3_act_supported(int32_t kind, int64_t n, int64_t h, int64_t na);
int32_t rlhip_dqn3_act_f32(int32_t kind, const void* env_cfg, const rlhip_env_state* st, int64_t n, const float* params,
                           const uint16_t* packed, int64_t h, int64_t na, int32_t act, double eps, uint64_t explorer_seed,
                           uint32_t explorer_step, uint64_t env_seed, uint32_t env_id_base, rlhip_ring* rb, int32_t* actions,
                           float* q_out, float* obs, float* last_obs, rlhip_stream_t stream);
int64_t rlhip_dqn3_workspace_bytes(int64_t ns, int64_t h, int64_t na, int64_t batch);
/* optimise!(learner, batch) up to the gradient, as rlhip_dqn_grad_f32.  idx: optional explicit flat logical
 * indices (e.g. from rlhip_ring_sample_prioritized); NULL = the uniform BatchSampler draw of
 * rlhip_ring_sample_indices(seed, draw_ctr) evaluated inline.  td_out: optional |Q(s,a) - y| per sample
 * (priority write-back).  loss_out: mean Huber loss. */
int32_t rlhip_dqn3_grad_f32(const rlhip_ring* rb_host, int64_t h, int64_t na, int32_t act, const float* params,
                            const uint16_t* packed, const float* target_params, const uint16_t* target_packed,
                            int64_t batch, const int64_t* idx, float gamma, float huber_delta, uint64_t seed,
                            uint32_t draw_ctr, void* workspace, float* grad_out, float* loss_out, float* td_out,
                            rlhip_stream_t stream);
/* the same with importance-sampling weights (rlhip_per_is_weights_f32): loss = mean(weights .* huber(Q(s,a) - y)),
 * every sample's gradient scaled by its weight; td_out stays the unweighted |Q(s,a) - y| */
int32_t rlhip_dqn3_grad_w_f32(const rlhip_ring* rb_host, int64_t h, int64_t na, int32_t act, const float* params,
                              const uint16_t* packed, const float* target_params, const uint16_t* target_packed,
                              int64_t batch, const int64_t* idx, const float* weights, float gamma, float huber_delta,
                              void* workspace, float* grad_out, float* loss_out, float* td_out, rlhip_stream_t stream);
/* optimise!(learner, batch) of the 3-layer learner complete, in two launches: the gradient (as rlhip_dqn3_grad_f32
 * with the inline uniform draw), then reduce + clip-by-global-norm + Adam + the bf16 re-pack of W2 in one launch;
 * bit-identical to rlhip_dqn3_grad_f32, rlhip_clip_adam_f32, rlhip_mlp3_pack_bf16 in sequence.  `packed` is updated
 * in place.  The tail of `workspace` (rlhip_dqn3_workspace_bytes) holds the launch's counters: zero before the
 * first call, re-armed by every call. */
int32_t rlhip_dqn3_update_f32(const rlhip_ring* rb_host, int64_t h, int64_t na, int32_t act, float* params,
                              uint16_t* packed, const float* target_params, const uint16_t* target_packed,
                              int64_t batch, float gamma, float huber_delta, uint64_t seed, uint32_t draw_ctr,
                              void* workspace, float* grad_out, float* loss_out, float* m, float* v,
                              float* beta_pow, float grad_scale, float max_grad_norm, float lr, float beta1,
                              float beta2, float adam_eps, float* gn_out, rlhip_stream_t stream);

/* -------------------------------------------------------------------- priority sum-tree -- */
/* Prioritized replay: CircularArrayBuffers.SumTree (compat 0.1.12, RLCore/Project.toml:30) behind
 * ReinforcementLearningTrajectories 0.4 `CircularPrioritizedTraces` + the prioritized BatchSampler method
 * (`inds, priorities = rand(rng, sumtree, batchsize)`, `trajectory[:priority, keys] = p`) -- un-vendored, parity
 * unpinned; BASELINE.json configs[4] ("prioritized sampling gather").
 * tree: float[rlhip_sumtree_nodes(n_leaves)] device, ZERO-INITIALISED by the caller; implicit heap (root 1,
 * leaf k at P + k, P = next pow2 >= n_leaves).  Internal nodes are recomputed as left + right (drift-free).
 * tree[0] is not a heap node: rlhip_sumtree_update uses it as its arrival counter and leaves it 0.
 * Leaves are keyed by PHYSICAL ring position slot * n_env + env. */
int64_t rlhip_sumtree_nodes(int64_t n_leaves);
/* t[start+1 : start+count] .= value */
int32_t rlhip_sumtree_fill_range(float* tree, int64_t n_leaves, int64_t start, int64_t count, float value,
                                 rlhip_stream_t stream);
/* for (k, p) in zip(keys, prio): t[k] = p   (sequential semantics: the last duplicate wins).  0-based keys. */
int32_t rlhip_sumtree_update(float* tree, int64_t n_leaves, const int64_t* leaf, const float* prio, int64_t n,
                             rlhip_stream_t stream);
/* rand(rng, t, batch): v = u01_f32(Philox(seed, idx = b, blk 0, t = draw_ctr, SAMPLER).w2) * t.tree[1], descent
 * `v <= left ? left : (v -= left; right)` that never enters a zero-sum subtree.  prio_out may be NULL. */
int32_t rlhip_sumtree_sample(const float* tree, int64_t n_leaves, int64_t batch, uint64_t seed,
                             uint32_t draw_ctr, int64_t* leaf_out, float* prio_out, rlhip_stream_t stream);
/* PrioritizedDQN priority write-back value: out = (|td| + eps)^alpha (power in Float64, rounded once) */
int32_t rlhip_per_priority_f32(const float* td, int64_t n, float eps, float alpha, float* out,
                               rlhip_stream_t stream);
/* The two lines above and below as ONE launch -- PrioritizedDQN's `trajectory[:priority, keys] = (|td| .+ eps) .^ alpha` over
 * `CircularPrioritizedTraces` (RLTrajectories 0.4; un-vendored, PARITY UNPINNED): prio_out[i] = (|td[i]| + eps)^alpha for every i
 * (the power in Float64, rounded once; alpha == 1 takes no power), stored by item number whatever key[i] is, and tree[key] = prio_out
 * with the semantics of rlhip_sumtree_update (the last duplicate wins, out-of-range keys are never written, every parent is
 * left + right of its stored children, tree[0] is left at 0).  The tree (every node) and prio_out are byte for byte those of
 * rlhip_per_priority_f32(td -> prio_out) followed by rlhip_sumtree_update(tree, key, prio_out): the same kernels with the power of
 * td[item] as their value source, the same dispatch (one wave up to 64 keys, one workgroup up to 2^13 leaves, 32 / 128 / 256
 * workgroups above).  n == 0 returns without a launch.  prio_out is required and must not overlap td (workgroups read td while
 * others write prio_out): RLHIP_EINVAL before any launch.  Checks on eps, alpha, n and NULL pointers as the two entries. */
int32_t rlhip_per_writeback_f32(float* tree, int64_t n_leaves, const int64_t* key, const float* td, int64_t n, float eps,
                                float alpha, float* prio_out, rlhip_stream_t stream);
/* importance-sampling weights of the sampled batch (PrioritizedDQN, removed Zoo; Schaul et al. 2016):
 *   w = 1 ./ ((priorities .+ 1f-10) .^ beta);  w ./= maximum(w)      (powers in Float64, rounded once)
 * -- the N and total-priority factors of (N P(i))^-beta cancel in the normalisation.  PARITY UNPINNED. */
int32_t rlhip_per_is_weights_f32(const float* prio, int64_t n, float beta, float* w_out, rlhip_stream_t stream);
/* after rlhip_ring_push_transition: the n_env leaves of the newest transition frame := priority
 * (CircularPrioritizedTraces `default_priority`) */
int32_t rlhip_ring_push_priority(const rlhip_ring* rb_host, float* tree, float priority,
                                 rlhip_stream_t stream);
/* prioritized BatchSampler over the ring: idx_out = logical flat indices for rlhip_ring_gather, key_out =
 * physical leaf keys for rlhip_sumtree_update (may be NULL), prio_out = their priorities (may be NULL). */
int32_t rlhip_ring_sample_prioritized(const rlhip_ring* rb_host, const float* tree, int64_t batch,
                                      uint64_t seed, uint32_t draw_ctr, int64_t* idx_out, int64_t* key_out,
                                      float* prio_out, rlhip_stream_t stream);
/* The prioritized BatchSampler AND the gather of its batch in ONE launch (round 4): the draw of sample b is made by the
 * workgroup / lane that gathers it (same Philox draw, same descent: idx_out / key_out / prio_out and the gathered batch are
 * bit-identical to rlhip_ring_sample_prioritized followed by rlhip_ring_gather).  Frame-major rings (n_env = 1, frames of
 * >= 1 KB) and Float32 rings with <= 4 components; other layouts run the two launches.  Outputs as rlhip_ring_gather. */
int32_t rlhip_ring_sample_gather_prioritized(const rlhip_ring* rb_host, const float* tree, int64_t batch, uint64_t seed,
                                             uint32_t draw_ctr, int64_t* idx_out, int64_t* key_out, float* prio_out,
                                             void* s, int32_t* a, float* r, uint8_t* term, void* s_next,
                                             rlhip_stream_t stream);

/* The priority write-back of the PREVIOUS batch, the prioritized draw of the next one and the gather of its frames in ONE launch
 * (round 6): `trajectory[:priority, upd_key] = upd_prio` (as rlhip_sumtree_update: the last duplicate wins) is applied by one
 * wavefront of the launch before any workgroup draws; results -- the tree, idx / key / priority, the gathered batch -- are
 * bit-identical to rlhip_sumtree_update followed by rlhip_ring_sample_gather_prioritized, which is also what runs when the
 * combination has no fused form (n_upd > 64, n_upd == 0, rings that are not frame-major, sync == NULL).  `sync`: two device
 * words owned by the caller, zero before the first call and re-armed by every call (one pair per concurrently used stream).
 * The DQN-Atari step then is: plan! / act! / push! -> THIS -> gradient (which leaves the new priorities for the next call). */
int32_t rlhip_ring_update_sample_gather_prioritized(const rlhip_ring* rb_host, float* tree, const int64_t* upd_key,
                                                    const float* upd_prio, int64_t n_upd, int64_t batch, uint64_t seed,
                                                    uint32_t draw_ctr, int64_t* idx_out, int64_t* key_out, float* prio_out,
                                                    void* s, int32_t* a, float* r, uint8_t* term, void* s_next,
                                                    uint32_t* sync, rlhip_stream_t stream);

/* Prioritized n-step replay -- `sample(::NStepBatchSampler, ::CircularPrioritizedTraces)` of RLTrajectories 0.4 (un-vendored, PARITY
 * UNPINNED): the priorities times a validity mask ("n_step transitions lie at or after this start"), drawn from the product.  Here
 * the mask is kept in the tree: the leaves of the newest n_step - 1 transition frames are held at 0 and a frame receives its
 * priority only once n_step transitions lie at or after it, so the unchanged rlhip_ring_sample_prioritized -- whose descent never
 * enters a zero-sum subtree -- returns only valid window starts, distributed as p * valid / sum(p * valid).  Record rings only,
 * n_step in 1..32.  (Entry points added, no layout or signature changed: RLHIP_ABI_VERSION stays 2.)
 *   rlhip_ring_push_priority_nstep   after rlhip_ring_push_transition, in place of rlhip_ring_push_priority: first the n_env leaves of
 *                                    the newest frame := 0 (after a wrap that slot still carries the overwritten transition's
 *                                    priority), then, if length >= n_step, the n_env leaves of logical frame length - n_step :=
 *                                    priority.  n_step = 1 leaves the tree of rlhip_ring_push_priority bit for bit.
 *                                    n_step > capacity is RLHIP_EINVAL before anything moves.  Priorities written back with
 *                                    rlhip_sumtree_update must go to keys drawn since the last push: a masked leaf is never drawn, so
 *                                    it is never written.
 *   rlhip_per_sample_fold_nstep_f32  the prioritized draw and the n-step window fold in ONE launch: the lane that owns sample b makes
 *                                    the draw of rlhip_sumtree_sample, descends, maps the key to its logical index and walks the
 *                                    window as rlhip_ring_fold_nstep does (up to and including the first terminal step, never past the
 *                                    newest stored transition, right-to-left Float32 return); record b of slot 0 of `folded` is
 *                                    written as a whole 64-byte line and the counters of `folded` are set to "one stored vec-step".
 *                                    idx_out / key_out / prio_out / iota_out and the records are byte for byte those of
 *                                    rlhip_ring_sample_prioritized followed by rlhip_ring_fold_nstep on the same tree.  key_out,
 *                                    prio_out and iota_out may be NULL.  RLHIP_EINVAL when length < n_step (the masked tree has no
 *                                    mass).  A -DRLHIP_BOUNDS_CHECK build has no index to validate here: the indices are produced
 *                                    inside the launch (a key is clamped below capacity * n_env; every record read stays in the ring).
 *                                    Every DQN gradient entry point then runs unchanged on (folded, iota_out) with
 *                                    rlhip_gamma_pow(gamma, n_step), rlhip_dqn_fold_double_f32 / rlhip_dqn3_fold_double_f32 in place
 *                                    before it for Double DQN. */
int32_t rlhip_ring_push_priority_nstep(const rlhip_ring* rb_host, float* tree, float priority, int32_t n_step,
                                       rlhip_stream_t stream);
int32_t rlhip_per_sample_fold_nstep_f32(const rlhip_ring* rb_host, const float* tree, int64_t batch, int32_t n_step, float gamma,
                                        uint64_t seed, uint32_t draw_ctr, int64_t* idx_out, int64_t* key_out, float* prio_out,
                                        rlhip_ring* folded_host, int64_t* iota_out, rlhip_stream_t stream);
/* The same for FRAME rings (RLHIP_RING_FRAMES: UInt8 frames, Float32 observations with > 4 components; any n_env), where the n-step
 * transition is gathered (rlhip_ring_gather_nstep / rlhip_ring_gather_stacked_nstep), not folded.  (Entry points added:
 * RLHIP_ABI_VERSION stays 2.)
 *   rlhip_ring_push_priority_nstep_frames   the rule, the refusals and their order of rlhip_ring_push_priority_nstep -- the newest
 *                                    frame's n_env leaves := 0, then, if length >= n_step, the leaves of logical frame length - n_step
 *                                    := priority; n_step = 1 leaves the tree of rlhip_ring_push_priority bit for bit -- for frame
 *                                    rings; a record ring is RLHIP_EINVAL here as a frame ring is there.
 *   rlhip_ring_sample_gather_nstep_prioritized / rlhip_ring_sample_gather_stacked_nstep_prioritized
 *                                    the prioritized draw and the n-step gather of its batch in ONE launch.  idx_out / key_out /
 *                                    prio_out are byte for byte those of rlhip_ring_sample_prioritized on the same tree, every other
 *                                    output byte for byte that of rlhip_ring_gather_nstep / rlhip_ring_gather_stacked_nstep called
 *                                    with those indices, on all three routes (component-major for any n_env, Float32 and UInt8;
 *                                    frame-major; stack-at-sample).  key_out, prio_out and n_used may be NULL.  The call neither
 *                                    knows nor needs the mask: on a tree masked for n_step every window is complete, on an unmasked
 *                                    tree a window is cut at the newest stored transition, as the gathers define.
 *                                    RLHIP_EINVAL before any launch: what rlhip_ring_sample_prioritized or the gather it stands for
 *                                    refuses (n_step outside 1..32, a record ring, an empty ring, n_stack outside 1..8, n_env > 1 or
 *                                    a frame size that is no multiple of 16 bytes for the stacked call, the alignment conditions),
 *                                    NULL tree / idx_out / s / a / ret / term / s_next, a tree that is not 8-byte aligned, ring
 *                                    counters out of range.  batch == 0 is RLHIP_OK.  Memory safety: the tree holds
 *                                    rlhip_sumtree_nodes(capacity * n_env) floats and is 8-byte aligned (child pairs are read as one
 *                                    8-byte load, as the shipped sampler reads them); every tree read is below that size, and a drawn
 *                                    key is clamped below capacity * n_env, so every address formed from it stays inside the ring's
 *                                    allocations for ANY tree contents; a leaf outside the logical range (no push ABI puts mass
 *                                    there) gives a one-step window.  A -DRLHIP_BOUNDS_CHECK build has no
 *                                    caller index to validate here.
 *                                    Measured on the 84 x 84 UInt8 ring, capacity 2^17, full, n_step 3, n_stack 4, against the two
 *                                    launches (profiles/per_frames_nstep.md), us per call at batch 32 / 512 / 4096: frame-major 8.95 /
 *                                    8.55 / 27.99 against 15.50 / 14.52 / 29.95; stacked 15.73 / 23.36 / 80.34 against 18.35 / 26.33 /
 *                                    80.33.  The frame-major kernel publishes the drawn index behind a first barrier, so that every
 *                                    wave requests its state chunks while the window is fetched, and the next frame behind a second
 *                                    (the one-barrier schedule measured 30.5 us at batch 4096).  The stacked call launches its fused
 *                                    kernel for batch <= 1536 and the two launches it stands for beyond (fused measured 1.16 x / 1.10 x
 *                                    their time at batch 2048 / 4096; timed at n_stack 4 only): same bytes either way.  The component-major route is fused at
 *                                    every size and was not timed. */
int32_t rlhip_ring_push_priority_nstep_frames(const rlhip_ring* rb_host, float* tree, float priority, int32_t n_step,
                                              rlhip_stream_t stream);
int32_t rlhip_ring_sample_gather_nstep_prioritized(const rlhip_ring* rb_host, const float* tree, int64_t batch, int32_t n_step,
                                                   float gamma, uint64_t seed, uint32_t draw_ctr, int64_t* idx_out, int64_t* key_out,
                                                   float* prio_out, void* s, int32_t* a, float* ret, uint8_t* term, void* s_next,
                                                   int32_t* n_used, rlhip_stream_t stream);
int32_t rlhip_ring_sample_gather_stacked_nstep_prioritized(const rlhip_ring* rb_host, const float* tree, int64_t batch, int32_t n_stack,
                                                           int32_t n_step, float gamma, uint64_t seed, uint32_t draw_ctr,
                                                           int64_t* idx_out, int64_t* key_out, float* prio_out, void* s, int32_t* a,
                                                           float* ret, uint8_t* term, void* s_next, int32_t* n_used,
                                                           rlhip_stream_t stream);

/* ---------------------------------------------------------------------------------- MLP -- */
/* Chain(Dense(n_in, h, act), Dense(h, n_out)) with flat parameters in Flux.destructure order:
 *   W1 (h x n_in col-major) | b1 (h) | W2 (n_out x h col-major) | b2 (n_out).   act: 0 relu, 1 tanh.
 * FluxApproximator.forward  RLCore/policies/learners/flux_approximator.jl:43.
 * x: SoA (n_in x batch), out: SoA (n_out x batch). */
int64_t rlhip_mlp2_nparams(int64_t n_in, int64_t h, int64_t n_out);
int32_t rlhip_mlp2_forward_f32(const float* params, int64_t n_in, int64_t h, int64_t n_out,
                               int32_t act, const float* x, int64_t batch, float* out,
                               rlhip_stream_t stream);
/* glorot_uniform stand-in (Philox INIT stream; biases zero); net_id separates actor / critic / q */
int32_t rlhip_mlp2_init_f32(float* params, int64_t n_in, int64_t h, int64_t n_out, uint64_t seed,
                            uint32_t net_id, rlhip_stream_t stream);

/* ------------------------------------------------------------------------------ PPO path -- */
/* PPOPolicy hyper-parameters (removed Zoo; blog a_practical_introduction_to_RL.jl/index.html:15257-15278) */
typedef struct {
    float gamma, lambda, clip_range, max_grad_norm;
    float actor_loss_weight, critic_loss_weight, entropy_loss_weight;
    float lr, beta1, beta2, adam_eps;
    int32_t n_epochs, n_microbatches;
    int32_t hidden, act;
    int32_t continuous;          /* 0 categorical actor; 1 gaussian actor (mu, log sigma) */
    int32_t normalize_advantage; /* 0 or 1: the removed RLZoo PPO's option, per (epoch, micro-batch) of bm = n T / n_microbatches
                                  * samples: adv = (float)((adv - mean) / clamp(std, 1e-8, 1000)) with the Float64 mean and the
                                  * corrected two-pass std (divisor bm - 1, or 1 when bm <= 1); see rlhip_ppo_adv_normalize_f32.
                                  * Every grad / update entry point honours it (the multi-GPU ones only at world = 1) */
    int32_t layers;              /* 2 (default; 0 means 2): ns -> hidden -> nout on the VALU (ppo.hip / ppo_grad.hip);
                                  * 3: ns -> hidden -> hidden -> nout actor and critic with the hidden x hidden layer on the
                                  * bf16 MFMA, hidden = 128 (ppo3.hip) or 256 (ppo3w.hip), BASELINE configs[2]
                                  * "actor/critic MLP in bf16 MFMA"; CartPole (categorical) and Pendulum (Gaussian) */
} rlhip_ppo_cfg;
int32_t rlhip_ppo_default(rlhip_ppo_cfg* cfg_host);
/* parameter count of ActorCritic(actor = ns->hidden->na_out, critic = ns->hidden->1), flat = [actor | critic] */
int64_t rlhip_ppo_nparams(int32_t kind, const rlhip_ppo_cfg* cfg_host);

/* PPOTrajectory of one update period, time-major SoA device arrays (caller-owned):
 *   obs (T+1, ns, n) f32 | action_i (T, n) i32 | action_f (T, na, n) f32 | logp (T, n) f32 |
 *   value (T+1, n) f32 | reward (T, n) f32 | terminal (T, n) u8 | adv (T, n) f32 | ret (T, n) f32 */
typedef struct {
    float* obs;
    float* logp;
    float* value;
    float* reward;
    float* adv;
    float* ret;
    float* action_f;
    int32_t* action_i;
    uint8_t* terminal;
} rlhip_ppo_traj;

/* The blog's `_run(policy, env::MultiThreadEnv, ...)` inner loop (index.md:351-374) for T vec-steps in
 * ONE launch: per step  state(env) -> actor/critic forward -> sample action (+ log-prob) -> trajectory
 * write -> act! (+ auto-reset) -> reward / terminal write; finally obs[T], value[T].
 * vec_step0: global vec-step counter at entry (Philox t of the sampling streams). */
int32_t rlhip_ppo_rollout_f32(int32_t kind, const void* env_cfg_host, const rlhip_env_state* st_host,
                              int64_t n, int64_t T, const rlhip_ppo_cfg* cfg_host,
                              const float* params, uint64_t seed, uint32_t env_id_base,
                              uint32_t vec_step0, const rlhip_ppo_traj* traj_host,
                              rlhip_stream_t stream);
/* plan!(policy, env) of the vector env as ONE launch (the per-step form of the rollout above, same
 * device code and lane split, hence bit-identical to it): actor/critic forward on obs (SoA ns x n),
 * action sample (Gumbel-max categorical networks.jl:425-432, or gaussian :64-82), log-prob, value.
 * action_i (discrete) or action_f (continuous) must be non-NULL; logp / value are nullable. */
int32_t rlhip_ppo_plan_f32(int32_t kind, const rlhip_ppo_cfg* cfg_host, const float* params,
                           const float* obs, int64_t n, uint64_t seed, uint32_t env_id_base,
                           uint32_t vec_step, int32_t* action_i, float* action_f, float* logp,
                           float* value, rlhip_stream_t stream);
/* The per-step protocol's pushes into slot t of the time-major PPO traces, one launch each (agent_base.jl:45-59):
 * PreActStage: state (ns x n SoA), value, action_log_prob, action (action_i or action_f, the other NULL);
 * logp == NULL and no action = the bootstrap push of (state, value) into slot T.  PostActStage: reward, terminal. */
int32_t rlhip_ppo_push_preact_f32(const rlhip_ppo_traj* traj_host, int64_t t, int64_t ns, int64_t n, const float* obs,
                                  const float* value, const float* logp, const int32_t* action_i, const float* action_f,
                                  rlhip_stream_t stream);
int32_t rlhip_ppo_push_postact_f32(const rlhip_ppo_traj* traj_host, int64_t t, int64_t n, const float* reward,
                                   const uint8_t* done, rlhip_stream_t stream);
/* generalized_advantage_estimation(reward, values, gamma, lambda; dims = 2, terminal) + returns */
int32_t rlhip_ppo_gae_f32(const rlhip_ppo_cfg* cfg_host, int64_t n, int64_t T,
                          const rlhip_ppo_traj* traj_host, rlhip_stream_t stream);
/* workspace (device) needed by rlhip_ppo_grad_f32 / rlhip_ppo_update_f32, in bytes, for trajectories of up to n x T entries
 * (two-layer nets: partial gradient rows, the unit-record image, and 32 bytes per
 * trajectory entry for the sample records an update call packs once -- none above 2^24 entries).  It must be zero-initialised
 * once after allocation (it holds counters and epoch words that the kernels maintain themselves): rlhip_ppo_workspace_init
 * does that and registers its size. */
int64_t rlhip_ppo_workspace_bytes(int32_t kind, const rlhip_ppo_cfg* cfg_host, int64_t n, int64_t T);
/* Advantage normalisation (cfg.normalize_advantage = 1) of micro-batch `mb` of epoch `epoch_ctr`: the samples the epoch's keyed
 * permutation puts at positions [mb bm, (mb + 1) bm), bm = n T / n_microbatches.  adv_out[f] = (float)((adv[f] - mu) / sd) for
 * those trajectory entries f (all others untouched), stats_out (device, nullable): double[2] = {mu, sd}, the Float64 mean and
 * the clamped corrected std.  The sums run in a fixed tree (bit-identical from run to run; the oracle sums sequentially).
 * The gradient / update entry points run the same kernels for every micro-batch of an epoch at once, into a region behind the
 * flag-off workspace: rlhip_ppo_update*_f32 once per epoch; rlhip_ppo_grad*_f32 on every call (three launches over all n T
 * entries per micro-batch gradient -- the host-stepped sequences, the world = 1 sharded routes among them, pay that per step).
 * With the flag on, rlhip_ppo_workspace_bytes = R(W) + R(4 n T) + S, W = the flag-off size, R(x) = 256 ceil(x / 256), and
 *   S = R(4 n T) + R(8 ceil(n T / 1024) n_mb + 16 n_mb) + 256   for n_mb = n_microbatches <= 64,
 *   S = R(16 n_mb (ceil(bm / 2048) + 1))                         above
 * (the normalised plane; per-entry micro-batch indices, Float64 partial sums, statistics and a counter).  The sharded updates (rlhip_ppo_update_p2p_f32,
 * rlhip_ppo_update_comm_f32) return RLHIP_EINVAL with the flag on and world > 1: per-rank statistics are not those of one GPU
 * with a world-times larger batch. */
int32_t rlhip_ppo_adv_normalize_f32(const rlhip_ppo_cfg* cfg_host, int64_t n, int64_t T, const float* adv, uint64_t seed,
                                    uint32_t epoch_ctr, int32_t mb, float* adv_out, double* stats_out, rlhip_stream_t stream);
/* ABI 2: REGISTER a workspace before its first use: zero-fills `bytes` bytes on `stream` (the counters and epoch words the
 * kernels maintain) and records (pointer -> bytes) in a host-side table.  Every rlhip_ppo_grad* / rlhip_ppo_apply_f32 /
 * rlhip_ppo_update* call compares rlhip_ppo_workspace_bytes(kind, cfg, n, T) of THAT call with the registered size and returns
 * RLHIP_EINVAL when it is larger -- or when the workspace was never registered -- instead of writing sample records past the
 * allocation (ABI 1: "the ABI carries no size to check").  Re-registering a pointer replaces its entry;
 * rlhip_ppo_workspace_release drops it (call it before freeing the memory). */
int32_t rlhip_ppo_workspace_init(void* workspace, int64_t bytes, rlhip_stream_t stream);
int32_t rlhip_ppo_workspace_release(void* workspace);
/* loss + flat gradient of micro-batch `mb` of epoch `epoch_ctr` (samples = keyed permutation of the
 * T*n transitions).  grad_out: f32[nparams]; losses_out (nullable): f32[4] = loss, actor, critic, entropy */
int32_t rlhip_ppo_grad_f32(int32_t kind, const rlhip_ppo_cfg* cfg_host, int64_t n, int64_t T,
                           const rlhip_ppo_traj* traj_host, const float* params, uint64_t seed,
                           uint32_t epoch_ctr, int32_t mb, void* workspace, float* grad_out,
                           float* losses_out, rlhip_stream_t stream);
/* Multi-GPU optimiser step: after the host's all-reduce of grad_out, rlhip_ppo_apply_f32 does [grad_scale] ->
 * clip_by_global_norm! -> Adam AND refreshes the learner's internal weight records in one launch, so that the next
 * micro-batch can call rlhip_ppo_grad_fresh_f32 (= rlhip_ppo_grad_f32 without its re-pack launch).  The first
 * gradient of an update call must use rlhip_ppo_grad_f32 (the parameters may have been changed by anyone). */
int32_t rlhip_ppo_grad_fresh_f32(int32_t kind, const rlhip_ppo_cfg* cfg_host, int64_t n, int64_t T,
                                 const rlhip_ppo_traj* traj_host, const float* params, uint64_t seed,
                                 uint32_t epoch_ctr, int32_t mb, void* workspace, float* grad_out,
                                 float* losses_out, rlhip_stream_t stream);
int32_t rlhip_ppo_apply_f32(int32_t kind, const rlhip_ppo_cfg* cfg_host, int64_t n, int64_t T, float* params,
                            float* grad, float* m, float* v, float* beta_pow, float grad_scale, void* workspace,
                            float* gn_out, rlhip_stream_t stream);
/* optimise!(policy) of a policy sharded over `world` GPUs in ONE call: per optimiser step { rlhip_ppo_grad[_fresh]_f32
 * -> rlhip_p2p_allreduce_f32 -> rlhip_ppo_apply_f32(grad_scale = 1 / world) }, 4 launches on one stream, no host work
 * in between.  comm_bufs_host / comm_cap / status_dev / timeout_polls as rlhip_p2p_allreduce_f32; seq0 = the last
 * sequence number used (the call consumes seq0 + 1 .. seq0 + n_epochs * n_microbatches). */
int32_t rlhip_ppo_update_p2p_f32(int32_t kind, const rlhip_ppo_cfg* cfg_host, int64_t n, int64_t T,
                                 const rlhip_ppo_traj* traj_host, float* params, float* m, float* v,
                                 float* beta_pow, uint64_t seed, uint32_t update_ctr, void* workspace,
                                 float* grad_scratch, float* losses_out, int32_t rank, int32_t world,
                                 void* const* comm_bufs_host, int64_t comm_cap, uint32_t seq0,
                                 int64_t timeout_polls, int32_t* status_dev, rlhip_stream_t stream);
/* The same with a communicator (rlhip_comm_init): the fused peer-to-peer kernels when rlhip_p2p_setup activated them,
 * otherwise per optimiser step { gradient -> rlhip_allreduce_grads (ncclAllReduce on `stream`) -> rlhip_ppo_apply_f32 }.
 * world = 1 communicators without an RCCL side run rlhip_ppo_update_f32 (with one, the general sequence over a
 * one-rank ncclAllReduce: same bits).  Sequence numbers are kept inside the communicator. */
int32_t rlhip_ppo_update_comm_f32(int32_t kind, const rlhip_ppo_cfg* cfg_host, int64_t n, int64_t T,
                                  const rlhip_ppo_traj* traj_host, float* params, float* m, float* v,
                                  float* beta_pow, uint64_t seed, uint32_t update_ctr, void* workspace,
                                  float* grad_scratch, float* losses_out, rlhip_comm_t comm, rlhip_stream_t stream);
/* n_epochs x n_microbatches of { grad -> clip_by_global_norm! -> Adam } (single-GPU optimise!; multi-GPU hosts call
 * rlhip_ppo_update_comm_f32, or rlhip_ppo_grad_f32, all-reduce, rlhip_ppo_apply_f32).  update_ctr = number of previous
 * update calls.  Two-layer networks: two launches per optimiser step (gradient tiles -- the first one of a call also builds its
 * weight records from `params` and writes the sample records; then partial reduction + norm exchange + clip + Adam + record refresh).  WORKSPACE SIZE: the call writes 32 bytes per trajectory entry
 * (n * T of THIS call) of sample records behind the fixed part of the workspace -- the workspace must have been sized by
 * rlhip_ppo_workspace_bytes(kind, cfg, n, T) for the LARGEST n * T it is ever used with and registered with
 * rlhip_ppo_workspace_init; a call that needs more than was registered returns RLHIP_EINVAL (ABI 2). */
int32_t rlhip_ppo_update_f32(int32_t kind, const rlhip_ppo_cfg* cfg_host, int64_t n, int64_t T,
                             const rlhip_ppo_traj* traj_host, float* params, float* m, float* v,
                             float* beta_pow, uint64_t seed, uint32_t update_ctr, void* workspace,
                             float* grad_scratch, float* losses_out, rlhip_stream_t stream);

/* Device-resident counters: the same three calls with the vec-step counter (counters[0]) and the update
 * counter (counters[1]) read from device memory by the kernels instead of being baked into the launch
 * arguments, so that one whole iteration (rollout -> GAE -> update [-> all-reduces]) can be captured in a
 * HIP graph and replayed: the Philox streams still advance.  rlhip_counters_advance is the last node.
 * `epoch_local` = epoch index inside the current update (0 .. n_epochs-1). */
int32_t rlhip_ppo_rollout_dc_f32(int32_t kind, const void* env_cfg_host, const rlhip_env_state* st_host,
                                 int64_t n, int64_t T, const rlhip_ppo_cfg* cfg_host, const float* params,
                                 uint64_t seed, uint32_t env_id_base, const uint32_t* counters,
                                 const rlhip_ppo_traj* traj_host, rlhip_stream_t stream);
int32_t rlhip_ppo_grad_dc_f32(int32_t kind, const rlhip_ppo_cfg* cfg_host, int64_t n, int64_t T,
                              const rlhip_ppo_traj* traj_host, const float* params, uint64_t seed,
                              uint32_t epoch_local, const uint32_t* counters, int32_t mb, void* workspace,
                              float* grad_out, float* losses_out, rlhip_stream_t stream);
int32_t rlhip_ppo_update_dc_f32(int32_t kind, const rlhip_ppo_cfg* cfg_host, int64_t n, int64_t T,
                                const rlhip_ppo_traj* traj_host, float* params, float* m, float* v,
                                float* beta_pow, uint64_t seed, const uint32_t* counters, void* workspace,
                                float* grad_scratch, float* losses_out, rlhip_stream_t stream);
int32_t rlhip_counters_advance(uint32_t* counters, uint32_t d_vec_step, uint32_t d_update,
                               rlhip_stream_t stream);

/* ------------------------------------------------------------------------------ DQN path -- */
/* BasicDQN / DQN learner (removed Zoo; spec docs/src/rlcore.md:28, blog index.html:15121-15147):
 * q-net and target-net = mlp2 (ns -> h -> na).  One launch samples `batch` transitions from the ring
 * (BatchSampler draw `draw_ctr`), computes the TD target with the target net, the Huber loss and the
 * flat gradient.  workspace bytes: rlhip_dqn_workspace_bytes (allocate it zeroed: see rlhip_dqn_update_f32). */
int64_t rlhip_dqn_workspace_bytes(int64_t ns, int64_t h, int64_t na, int64_t batch);
int32_t rlhip_dqn_grad_f32(const rlhip_ring* rb_host, int64_t h, int64_t na, int32_t act,
                           const float* params, const float* target_params, int64_t batch,
                           float gamma, float huber_delta, uint64_t seed, uint32_t draw_ctr,
                           void* workspace, float* grad_out, float* loss_out,
                           rlhip_stream_t stream);
/* optimise!(learner, batch) complete -- gradient, then reduce + clip-by-global-norm + Adam -- in ONE launch up to 2048
 * samples (the gradient workgroup that departs last folds the partial rows, clips and steps), in two launches beyond;
 * bit-identical to rlhip_dqn_grad_f32 followed by rlhip_clip_adam_f32 (which is what runs for > 4096 parameters).
 * The last 64 bytes of `workspace` are its departure counters: zero before the first call, re-armed by every call. */
int32_t rlhip_dqn_update_f32(const rlhip_ring* rb_host, int64_t h, int64_t na, int32_t act, float* params,
                             const float* target_params, int64_t batch, float gamma, float huber_delta,
                             uint64_t seed, uint32_t draw_ctr, void* workspace, float* grad_out, float* loss_out,
                             float* m, float* v, float* beta_pow, float grad_scale, float max_grad_norm, float lr,
                             float beta1, float beta2, float adam_eps, float* gn_out, rlhip_stream_t stream);
/* The same learner step on explicit flat logical indices (e.g. from rlhip_ring_sample_prioritized, the prioritized
 * BatchSampler of RLTrajectories 0.4) with |Q(s,a) - y| per sample returned for the priority write-back. */
int32_t rlhip_dqn_grad_idx_f32(const rlhip_ring* rb_host, int64_t h, int64_t na, int32_t act,
                               const float* params, const float* target_params, int64_t batch,
                               const int64_t* idx, float gamma, float huber_delta, void* workspace,
                               float* grad_out, float* loss_out, float* td_out, rlhip_stream_t stream);
/* ... and with importance-sampling weights (prioritized replay with beta > 0): loss = mean(weights .* huber) */
int32_t rlhip_dqn_grad_idx_w_f32(const rlhip_ring* rb_host, int64_t h, int64_t na, int32_t act,
                                 const float* params, const float* target_params, int64_t batch,
                                 const int64_t* idx, const float* weights, float gamma, float huber_delta,
                                 void* workspace, float* grad_out, float* loss_out, float* td_out,
                                 rlhip_stream_t stream);
/* plan!(QBasedPolicy, env) for the vector env in one launch: q = forward(learner, state(env)) then
 * eps-greedy selection (q_based_policy.jl:30-32, abstract_learner.jl:37-39, epsilon_greedy_explorer.jl:108-112).
 * q_out (nullable): SoA (na x n). */
int32_t rlhip_dqn_plan_f32(const float* params, int64_t ns, int64_t h, int64_t na, int32_t act,
                           const float* obs, int64_t n, double eps, uint64_t seed,
                           uint32_t env_id_base, uint32_t step, int32_t* actions, float* q_out,
                           rlhip_stream_t stream);

/* ------------------------------------------------- DQN on observations of 5..16 components -- */
/* (csrc/dqn_batch.hip; AcrobotRK4Env has six.  Entry points added, no layout or signature changed: RLHIP_ABI_VERSION stays 2.)
 *
 * rlhip_dqn_plan_obsn_f32: rlhip_dqn_plan_f32 for ns in 5..16 (na 1..4, h >= 1, act 0 / 1; n = 0 is a no-op; ns <= 4 or ns > 16 is
 * RLHIP_EINVAL: 2..4 components take rlhip_dqn_plan_f32).  One lane per env.  q_out (nullable, SoA (na x n)) is byte for byte
 * rlhip_mlp2_forward_f32 -- z = b1[j], fmaf over k ascending; q = b2, fmaf over j ascending -- and `actions` byte for byte
 * rlhip_eps_greedy_select_f32 (no mask, no tie-break) on those values with the same (eps, seed, env_id_base, step). */
int32_t rlhip_dqn_plan_obsn_f32(const float* params, int64_t ns, int64_t h, int64_t na, int32_t act, const float* obs, int64_t n,
                                double eps, uint64_t seed, uint32_t env_id_base, uint32_t step, int32_t* actions, float* q_out,
                                rlhip_stream_t stream);
/* rlhip_dqn_grad_batch_f32: loss and flat gradient of the two-layer Float32 Q-network on a GATHERED batch -- s / s_next SoA
 * (ns x batch) as rlhip_ring_gather, rlhip_ring_gather_nstep and rlhip_ring_sample_gather_nstep_prioritized write them from a
 * frame-layout ring, a / r / term (batch).  ns 5..16, h a multiple of 4 and <= 256, na 1..4, act 0 / 1, batch >= 1; anything else
 * (and a NULL array other than the three nullable ones) is RLHIP_EINVAL before any launch.  workspace: at least
 * rlhip_dqn_batch_workspace_bytes(ns, h, na, batch) bytes (-1 for a shape this entry refuses); it needs no initialisation.
 *
 * Per sample i, in Float32 without contraction (oracle/rlo_learn.c rlo_dqn_loss_grad_f32):
 *     cont = term[i] ? 0 : 1
 *     disc = n_used ? rlhip_gamma_pow(gamma, clamp(n_used[i], 0, 32)) : gamma      (the 33 powers are computed on the host)
 *     sel  = max_o Qt(s')[o];  double_dqn != 0:  sel = Qt(s')[first argmax_o Q(s')[o]]  (strict >: the first maximum wins)
 *     G    = r[i] + (disc * cont) * sel
 *     d    = Q(s)[a[i]] - G;   e = |d|
 *     l    = e < delta ? (e * e) * 0.5 : delta * (e - 0.5 * delta)
 *     gi   = (e < delta ? d : sign(d) * delta) / (float)batch;   with weights:  gi *= weights[i],  l *= weights[i]
 *     loss_out[0] = (sum_i l) / (float)batch,   td_out[i] = e (td_out nullable),   grad_out = the back-propagation of gi through Q
 * a[i] is only ever compared (o == a[i]), never used as an index: an action outside 0 .. na - 1 cannot read or write out of bounds,
 * and such a sample contributes gi = 0, l = 0 and td_out[i] = 0.  The bounds-checked build (build.py --variant=bounds) refuses such
 * a batch with RLHIP_EINVAL instead (one more launch and a stream synchronisation).
 *
 * Summation order -- fixed, a function of (batch, h, ns, na) only; no float atomics; two calls on the same inputs give the same bytes:
 *   layer 1     z[j] = b1[j], then fmaf(W1[j, k], x[k], .) over k ascending -- the oracle's chain, so the ReLU mask is the oracle's
 *               bit for bit (rows are padded to a multiple of four inputs with fmaf(0, 0, z) behind the chain: z = -0 becomes +0)
 *   Q values    lane c of a 16-lane row sums fmaf(W2[o, j], h[j], .) over j = c, c + 16, .. ascending from 0; the sixteen partial sums
 *               meet in the xor tree (1, 2, half-row mirror, row mirror); b2[o] is added last
 *   dh          fmaf(dq[o], W2[o, j], .) over o ascending from 0
 *   batch sums  the batch is cut into tiles of 64 samples; workgroup g of nb = min(tiles, 256) owns tiles g, g + nb, ..
 *               dW1, db1, dW2: ONE fmaf / add chain per element over the workgroup's samples, ascending
 *               db2, loss: per sample slot (i mod 64) over the workgroup's tiles ascending, then the 64 slots in the xor tree
 *               (1, 2, half-row mirror, row mirror, 16, 32)
 *               across workgroups: the nb partial rows in four groups of ceil(nb / 4), ascending inside a group, ((g0 + g1) + g2) + g3;
 *               the partial losses lane-strided over 64 lanes, then the shift-down tree 32, 16, .., 1 */
int64_t rlhip_dqn_batch_workspace_bytes(int64_t ns, int64_t h, int64_t na, int64_t batch);
int32_t rlhip_dqn_grad_batch_f32(int64_t ns, int64_t h, int64_t na, int32_t act, const float* params, const float* target_params,
                                 const float* s, const int32_t* a, const float* r, const uint8_t* term, const float* s_next,
                                 int64_t batch, float gamma, const int32_t* n_used, const float* weights, int32_t double_dqn,
                                 float huber_delta, void* workspace, float* grad_out, float* loss_out, float* td_out,
                                 rlhip_stream_t stream);

/* ------------------------------------------------------------- Soft Actor-Critic (SAC) -- */
/* (csrc/sac.hip.  Entry points added, no layout or signature changed: RLHIP_ABI_VERSION stays 2.)
 *
 * The reference calls SoftGaussianNetwork "mainly used for SAC" (RLCore/src/utils/networks.jl:127-128) and its docs name SACPolicy on
 * Pendulum as the continuous off-policy baseline, but the Zoo's SACPolicy is not in the reference snapshot: parity with it is
 * unpinned, and THIS TEXT is the specification (tests/sac_ref.py replays it and differentiates it independently).
 *
 * Scope: record rings (Float32 observations, obs_dim = ns in 2..4), ONE action component, two-layer Float32 networks with h a
 * multiple of 4 and <= 256, act 0 relu / 1 tanh.  A frame ring, another obs_dim, h or act, batch < 1, an empty ring or a NULL array
 * that is not nullable is RLHIP_EINVAL before any launch.  All arithmetic is Float32 without contraction; fmaf only where written.
 *
 * Networks, flat as rlhip_mlp2_nparams / rlhip_mlp2_init_f32 lay them out:
 *     actor    = mlp2(ns, h, 2): pre = Dense(ns, h, act), mu = Dense(h, 1), sigma = Dense(h, 1, softplus) in one vector; output
 *                row 0 is mu, row 1 is rho (sigma before its softplus)
 *     critics  = [Q1 | Q2], each mlp2(ns + 1, h, 1) on vcat(s, u): input rows 0 .. ns - 1 the state, row ns the action
 *     targets  = a copy of the critics' vector           (init net_ids: 0 actor, 1 and 2 the critics)
 * EVERY forward pass is the chain of rlhip_mlp2_forward_f32: z[j] = b1[j], fmaf(W1[j, k], x[k], .) over k ascending; out[o] = b2[o],
 * fmaf(W2[o, j], act(z[j]), .) over j ascending -- one lane per (sample, network), no sum crosses lanes.
 *
 * Actor head (HeadLogp<1> of csrc/heads.hip at d = 1; softplus_nnlib, clampj, normal_draw, normlogpdf1 of csrc/head_device.h and
 * csrc/ppo_sample_device.h):
 *     raw  = softplus_nnlib(rho);  sg = clampj(raw, min_sigma, max_sigma);  pass = !(raw > max_sigma) && !(raw < min_sigma)
 *     z    = mu + sg * eps;        a  = tanhf(z);   u = action_scale * a
 *     logp = normlogpdf1(mu, sg, z) - 2.0f * ((0.6931472f - z) - softplus_nnlib(-2.0f * z))
 *
 * rlhip_sac_plan_f32 -- plan! for n envs in one launch, one lane per env.  obs SoA (ns x n); eps = normal_draw(seed, env_id_base + i,
 * step, 0); action_out[i] = u.  Nullable: logp_out, mu_out, rho_out, raw_sigma_out (n each).  mu_out / rho_out are byte for byte
 * rlhip_mlp2_forward_f32, action_out / action_scale and logp_out byte for byte rlhip_gaussian_head_sample_f32(soft = 1) on them.
 * deterministic != 0: u = action_scale * tanhf(mu), no draw, and logp_out must be NULL (RLHIP_EINVAL otherwise).  n = 0 is a no-op.
 *
 * rlhip_sac_critic_grad_f32 -- idx[i]: flat logical indices into the ring as in rlhip_dqn_grad_idx_f32 (the bounds-checked build
 * validates them first); the record is {s, a, r, t, s'}, its action word read as the Float32 whose bits it holds (what
 * rlhip_ring_push_transition stores when it is handed a Float32 action array).  alpha: device f32[1].  Per sample i:
 *     eps' = normal_draw(seed, i, step, 0)                                    (the id is the batch position i)
 *     u', logp' = the actor head at s';   x' = vcat(s', u')
 *     qt   = Qt2(x') < Qt1(x') ? Qt2(x') : Qt1(x')
 *     cont = t ? 0 : 1
 *     y    = r + (gamma * cont) * (qt - alpha * logp')
 *     x = vcat(s, a);  for c = 1, 2:  d_c = Q_c(x) - y;  l_c = d_c * d_c;  g_c = (2.0f * d_c) / (float)batch
 *     loss_out[c - 1] = (sum_i l_c) / (float)batch                           (Flux.Losses.mse; loss_out is f32[2])
 *     grad_out = [back-propagation of g_1 through Q1 | of g_2 through Q2]    (y is a constant; 2 mlp2_nparams(ns + 1, h, 1) floats)
 *     y_out (nullable) f32[batch]
 * Back-propagation of g through a critic, per sample and hidden unit j (hv = act(z[j]), act' = hv > 0 ? 1 : 0 for relu, 1 - hv hv
 * for tanh):  dW2[j] += fmaf(g, hv, .);  dz = (g * W2[j]) * act';  db1[j] += dz;  dW1[j, k] = fmaf(dz, x[k], .);  db2 += g.
 *
 * rlhip_sac_actor_grad_f32 -- `critics` are the ones the critic update has already stepped (the Zoo's order).  Per sample i:
 *     eps = normal_draw(seed, i, step, 1);  u, logp = the actor head at s;  x = vcat(s, u)
 *     sel = Q2(x) < Q1(x) ? 2 : 1;   q = Q_sel(x)
 *     l_i = alpha * logp - q;   stats_out = { (sum l_i) / fb, (sum q) / fb, (sum logp) / fb },  fb = (float)batch
 *     dlogp = alpha / fb;   dq = -1.0f / fb
 *     du   = 0, then over j ascending  fmaf((dq * W2_sel[j]) * act'(z_sel[j]), W1_sel[j, ns], du)    (the critics get no gradient)
 *     dact = action_scale * du
 *     (dmu, dsg) = the soft = 1 formulas of rlhip_gaussian_head_sample_bwd_f32 at d = 1, K = 1 with (dact, dlogp), the regenerated eps:
 *         s = sg + 1.0e-8f;  zz = (z - mu) / s;  w = zz / s;  dz = dlogp (2.0f a - w);  dz = dz + dact (1.0f - a a)
 *         dmu = dlogp w + dz;   dsg = dlogp ((zz zz - 1.0f) / s) + dz eps
 *     draw = pass ? dsg : +0.0f                                               (a select, never a product)
 *     drho = draw * (1.0f / (1.0f + expf(-rho)))
 *     grad_out = back-propagation of (dmu, drho) through the actor: dW2[o, j] = fmaf(d_o, hv, .);  dh = fmaf(drho, W2[1, j],
 *                fmaf(dmu, W2[0, j], 0));  dz = dh act';  db1[j] += dz;  dW1[j, k] = fmaf(dz, s[k], .);  db2[o] += d_o
 *     alpha step, if alpha_lr > 0 and alpha_out != NULL:  alpha_out[0] = alpha - alpha_lr * ((-stats_out[2]) - target_entropy)
 *         (alpha_out may be the pointer alpha: the gradient launch has read alpha before the fold writes it)
 *     sel_out (nullable) i32[batch],  logp_out (nullable) f32[batch]
 *
 * Summation order of both gradients -- fixed, a function of (batch, h, ns) only; no float atomics; two calls on the same inputs
 * give the same bytes:
 *   batch sums  the batch is cut into tiles of 64 samples; workgroup g of nb = min(tiles, 256) owns tiles g, g + nb, ..
 *               every gradient element, and every loss / statistic sum: ONE fmaf / add chain from +0 over the workgroup's samples in
 *               ascending batch position
 *   across workgroups: the nb partial rows in four groups of ceil(nb / 4), ascending inside a group, ((g0 + g1) + g2) + g3;
 *               the partial loss / statistic sums lane-strided over 64 lanes, then the shift-down tree 32, 16, .., 1; / (float)batch
 * workspace: at least rlhip_sac_workspace_bytes(ns, h, batch) bytes for either call (-1 for a refused shape); no initialisation.
 *
 * Stream separation.  One update = rlhip_ring_sample_indices -> critic gradient -> one rlhip_adam_f32 (rlhip_clip_adam_f32) over
 * [Q1 | Q2] -> actor gradient with the alpha step -> Adam over the actor -> rlhip_polyak_f32(targets, critics, rho = 1 - tau).  plan!
 * draws from the NORMAL stream under `seed` with step = the vec-step counter and id = the env; the two gradient launches of an update
 * draw under `seed + 1` with step = the update counter and id = the batch position, draw index 0 for the target action at s' and 1
 * for the actor's action at s.  No (seed, id, step, index) is used twice, so exploration noise and update noise are independent. */
int64_t rlhip_sac_workspace_bytes(int64_t ns, int64_t h, int64_t batch);
int32_t rlhip_sac_plan_f32(const float* actor, int64_t ns, int64_t h, int32_t act, const float* obs, int64_t n, float min_sigma,
                           float max_sigma, float action_scale, int32_t deterministic, uint64_t seed, uint32_t env_id_base,
                           uint32_t step, float* action_out, float* logp_out, float* mu_out, float* rho_out, float* raw_sigma_out,
                           rlhip_stream_t stream);
int32_t rlhip_sac_critic_grad_f32(const rlhip_ring* rb_host, int64_t h, int32_t act, const float* actor, const float* critics,
                                  const float* targets, int64_t batch, const int64_t* idx, const float* alpha, float gamma,
                                  float min_sigma, float max_sigma, float action_scale, uint64_t seed, uint32_t step, void* workspace,
                                  float* grad_out, float* loss_out, float* y_out, rlhip_stream_t stream);
int32_t rlhip_sac_actor_grad_f32(const rlhip_ring* rb_host, int64_t h, int32_t act, const float* actor, const float* critics,
                                 int64_t batch, const int64_t* idx, const float* alpha, float min_sigma, float max_sigma,
                                 float action_scale, uint64_t seed, uint32_t step, float alpha_lr, float target_entropy,
                                 float* alpha_out, void* workspace, float* grad_out, float* stats_out, int32_t* sel_out,
                                 float* logp_out, rlhip_stream_t stream);

/* ------------------------------------------ categorical (C51) distributional DQN learner -- */
/* (csrc/c51.hip.  Entry points added, no layout or signature changed: RLHIP_ABI_VERSION stays 2.)
 *
 * The reference's design blog names C51 and IQN as the distributional members of the QBasedPolicy family ("the estimation is not the
 * Q-values directly. But we can still fit them into the QBasedPolicy. The main change is to override ... plan! ... to use the Q value
 * distribution"), but the Zoo's RainbowLearner is not in the reference snapshot: parity with it is unpinned, and THIS TEXT is the
 * specification (tests/c51_ref.py replays it in Float32 and differentiates the mathematics independently in Float64).
 *
 * Network: the two-layer Float32 layout mlp2(ns, h, M) of rlhip_mlp2_nparams / rlhip_mlp2_init_f32 with M = na * n_atoms output rows;
 * row m = k + n_atoms * o holds atom k of action o (the column-major reshape (n_atoms, na, batch) of the Zoo).
 * Envelope: ns 2..16, h a multiple of 4 and <= 256, na 1..4, n_atoms 2..64, act 0 relu / 1 tanh, v_min < v_max both finite; anything
 * else (and a NULL array that is not nullable, n < 0, batch < 1) is RLHIP_EINVAL before any launch.
 *
 * All arithmetic is Float32 without contraction; fmaf only where written; "sum (k ascending)" is a chain of adds from +0.
 *     Delta  = (v_max - v_min) / (float)(n_atoms - 1)                         (host, once)
 *     z_k    = fmaf((float)k, Delta, v_min)
 *     hid[j] = act(zz),  zz = b1[j], then fmaf(W1[j, k], x[k], .) over k ascending
 *     l[m]   = b2[m], then fmaf(W2[m, j], hid[j], .) over j ascending         (one chain per logit, no sum crosses lanes)
 *     per action o:  mx = max_k l[k, o];  e_k = expf(l[k, o] - mx);  S = sum_k e_k (k ascending)
 *                    p[k, o] = e_k / S;   Q[o] = 0, then fmaf(z_k, p[k, o], .) over k ascending from 0
 *
 * rlhip_c51_forward_f32 -- forward(learner, s) for n observations, obs SoA (ns x n): q_out SoA (na x n); nullable probs_out and
 * logits_out, SoA ((n_atoms * na) x n) in row order m.  n = 0 is a no-op.
 * rlhip_c51_plan_f32 -- plan! in one launch: q_out (nullable) is byte for byte rlhip_c51_forward_f32 (the same kernel and the same
 * device function from logits to Q), `actions` byte for byte rlhip_eps_greedy_select_f32 (no mask, no tie-break) on those values with
 * the same (eps, seed, env_id_base, step).
 *
 * rlhip_c51_grad_batch_f32 -- loss and flat gradient on a GATHERED batch, exactly the arrays rlhip_dqn_grad_batch_f32 takes: s / s_next
 * SoA (ns x batch), a / r / term (batch), nullable n_used and weights.  Per sample i (l, p, Q of the online net unless marked t):
 *     cont = term[i] ? 0 : 1
 *     disc = n_used ? rlhip_gamma_pow(gamma, clamp(n_used[i], 0, 32)) : gamma      (the 33 powers are computed on the host)
 *     c    = disc * cont
 *     a*   = first argmax_o Qt(s')[o] (strict >);   double_dqn != 0:  first argmax_o Q(s')[o]              -> sel_out (i32[batch])
 *     pt_j = pt(s')[j, a*]
 *     Tz_j = min(max(r[i] + c * z_j, v_min), v_max)
 *     m_k  = 0, then fmaf(min(max(1 - |Tz_j - z_k| / Delta, 0), 1), pt_j, .) over j ascending   -> proj_out (n_atoms x batch SoA)
 *     lp_k = (l(s)[k, a_i] - mx) - logf(S)
 *     L_i  = -(0, then fmaf(m_k, lp_k, .) over k ascending)                                       -> ce_out (batch; UNWEIGHTED)
 *     Sm   = sum_k m_k (k ascending)
 *     g_k  = (p(s)[k, a_i] * Sm - m_k) / (float)batch;    with weights:  g_k *= weights[i],  L_i *= weights[i] in the loss
 *     loss_out[0] = (sum_i L_i) / (float)batch;   grad_out = the back-propagation of g through rows k + n_atoms * a_i only
 * The projection is the dense form (Dopamine / the Zoo's project_distribution), not the floor / ceil scatter: it has no hole where Tz
 * falls exactly on an atom and needs no scatter.  m, a* and the target are constants of the differentiation.
 * a[i] is only ever compared (o == a[i]), never used as an index: an action outside 0 .. na - 1 contributes nothing to the loss and the
 * gradient, and ce_out[i] = 0 (sel_out and proj_out are still written).  The bounds-checked build (build.py --variant=bounds) refuses
 * such a batch with RLHIP_EINVAL instead (one more launch and a stream synchronisation).
 *
 * Back-propagation and summation order -- fixed, a function of (batch, ns, h, na, n_atoms) only; no float atomics; two calls on the
 * same inputs give the same bytes.  The batch is cut into tiles of 8 samples; workgroup w of nb = min(tiles, 256, max(1, 16 MiB / the bytes
 * of one gradient row)) owns tiles w, w + nb, ..; "its samples" are the samples of those tiles in ascending batch position.  Every element below is ONE chain from +0:
 *     dW2[m, j]  fmaf(g_k, hid(s)[j], .) over the workgroup's samples with a_i = o (m = k + n_atoms o)
 *     db2[m]     adds of g_k over the same samples
 *     dh[j]      per sample: 0, then fmaf(g_k, W2[k + n_atoms a_i, j], .) over k ascending
 *     dz[j]      dh[j] * act',  act' = hid > 0 ? 1 : 0 for relu (the stored hid: both passes see one zz), 1 - hid hid for tanh
 *     dW1[j, k]  fmaf(dz[j], s[k], .) over the workgroup's samples;   db1[j]  adds of dz[j]
 *     loss       adds of L_i (weighted where weights are given) over the workgroup's samples
 *   across workgroups: the nb partial rows and partial losses in ascending w, adds from +0; the loss is then divided by (float)batch.
 * workspace: at least rlhip_c51_workspace_bytes(ns, h, na, n_atoms, batch) bytes (-1 for a refused shape); no initialisation.
 *
 * One update of rlhip.RainbowLearner = draw -> gather -> this gradient -> [rlhip_per_priority_f32 on ce_out: (ce + eps)^alpha, written
 * back under the drawn keys] -> rlhip_clip_adam_f32 -> target sync.  Out of scope: IQN, NoisyDense, a fused vec-step, a
 * gather inside the gradient launch, three-layer and bf16 nets, dueling distributional heads, sharded runs. */
int32_t rlhip_c51_forward_f32(const float* params, int64_t ns, int64_t h, int64_t na, int64_t n_atoms, int32_t act, float v_min,
                              float v_max, const float* obs, int64_t n, float* q_out, float* probs_out, float* logits_out,
                              rlhip_stream_t stream);
int32_t rlhip_c51_plan_f32(const float* params, int64_t ns, int64_t h, int64_t na, int64_t n_atoms, int32_t act, float v_min, float v_max,
                           const float* obs, int64_t n, double eps, uint64_t seed, uint32_t env_id_base, uint32_t step, int32_t* actions,
                           float* q_out, rlhip_stream_t stream);
int64_t rlhip_c51_workspace_bytes(int64_t ns, int64_t h, int64_t na, int64_t n_atoms, int64_t batch);
int32_t rlhip_c51_grad_batch_f32(int64_t ns, int64_t h, int64_t na, int64_t n_atoms, int32_t act, float v_min, float v_max,
                                 const float* params, const float* target_params, const float* s, const int32_t* a, const float* r,
                                 const uint8_t* term, const float* s_next, int64_t batch, float gamma, const int32_t* n_used,
                                 const float* weights, int32_t double_dqn, void* workspace, float* grad_out, float* loss_out,
                                 float* ce_out, float* proj_out, int32_t* sel_out, rlhip_stream_t stream);

/* ---------------------------------- quantile-regression (QR-DQN) distributional DQN learner -- */
/* (csrc/qrdqn.hip.  Entry points added, no layout or signature changed: RLHIP_ABI_VERSION stays 2.)
 *
 * The sibling of the categorical learner that needs no hand-chosen support: every action's value distribution is N quantiles at the fixed
 * levels tau_k, fitted by the quantile-Huber loss (Dabney et al. 2018).  The Zoo's QRDQNLearner is not in the reference snapshot either:
 * parity with it is unpinned, and THIS TEXT is the specification (tests/qrdqn_ref.py replays it in Float32 and differentiates the
 * mathematics independently in Float64).
 *
 * Network: mlp2(ns, h, M) with M = na * N output rows, N = n_quantiles; row m = k + N * o holds quantile k of action o.
 * Envelope: ns 2..16, h a multiple of 4 and <= 256, na 1..4, N 1..64, act 0 relu / 1 tanh, kappa finite and > 0; anything else (and a NULL
 * array that is not nullable, n < 0, batch < 1) is RLHIP_EINVAL before any launch.
 *
 * All arithmetic is Float32 without contraction; fmaf only where written; "sum (k ascending)" is a chain of adds from +0.
 *     hid[j], l[m]  exactly the C51 section's two chains (one fmaf chain per output row, no sum crosses lanes)
 *     th[k, o] = l[k + N o]                                                   (no softmax)
 *     Q[o]     = (sum_k th[k, o], k ascending) / (float)N
 *     tau_k    = (float)(2 k + 1) / (float)(2 N)
 *
 * rlhip_qrdqn_forward_f32 -- forward(learner, s) for n observations, obs SoA (ns x n): q_out SoA (na x n); nullable quantiles_out, SoA
 * ((N * na) x n) in row order m.  n = 0 is a no-op.
 * rlhip_qrdqn_plan_f32 -- plan! in one launch: q_out (nullable) is byte for byte rlhip_qrdqn_forward_f32 (the same kernel and the same
 * device function from rows to Q), `actions` byte for byte rlhip_eps_greedy_select_f32 (no mask, no tie-break) on those values with the
 * same (eps, seed, env_id_base, step).
 *
 * rlhip_qrdqn_grad_batch_f32 -- loss and flat gradient on a GATHERED batch, exactly the arrays rlhip_c51_grad_batch_f32 takes.  Per
 * sample i (th, Q of the online net unless marked t):
 *     cont, disc, c   as in the C51 section (gamma, or the 33 host-computed powers indexed by clamp(n_used[i], 0, 32)); c = disc * cont
 *     a*    = first argmax_o Qt(s')[o] (strict >);   double_dqn != 0:  first argmax_o Q(s')[o]              -> sel_out (i32[batch])
 *     T_j   = fmaf(c, th_t(s')[j, a*], r[i])                                                                -> target_out (N x batch SoA)
 *     per k, with th_k = th(s)[k, a_i], and per j:
 *         u    = T_j - th_k
 *         hub  = |u| <= kappa ? 0.5f * u * u : kappa * (|u| - 0.5f * kappa)
 *         dhub = min(max(u, -kappa), kappa)
 *         w    = u < 0 ? 1.0f - tau_k : tau_k
 *     rho_k = 0, then fmaf(w, hub  / kappa, .) over j ascending
 *     d_k   = 0, then fmaf(w, dhub / kappa, .) over j ascending
 *     L_i   = (sum_k rho_k, k ascending) / (float)N                                                         -> ql_out (batch; UNWEIGHTED)
 *     g_k   = -d_k / ((float)N * (float)batch)    (the divisor is ONE Float32 product);  with weights:  g_k *= weights[i],
 *             L_i *= weights[i] in the loss
 *     loss_out[0] = (sum_i L_i) / (float)batch;   grad_out = the back-propagation of g through rows k + N * a_i only
 * This is rho^kappa_tau(u) = |tau - 1{u < 0}| L_kappa(u) / kappa, summed over k and averaged over j.  T, a* and the target net are
 * constants of the differentiation.  With kappa > 0 the gradient is continuous in u: the only decisions are a* and, for relu, the sign of
 * a layer-1 pre-activation.
 * a[i] is only ever compared (o == a[i]), never used as an index: an action outside 0 .. na - 1 contributes nothing to the loss and the
 * gradient, and ql_out[i] = 0 (sel_out and target_out are still written).  The bounds-checked build (build.py --variant=bounds) refuses
 * such a batch with RLHIP_EINVAL instead (one more launch and a stream synchronisation).
 *
 * Back-propagation and summation order -- the C51 section's, word for word with N for n_atoms: tiles of 8 samples, workgroup w of
 * nb = min(tiles, 256, max(1, 16 MiB / the bytes of one gradient row)) owns tiles w, w + nb, ..; dW2 / db2 / dh / dz / dW1 / db1 / loss each
 * ONE chain from +0 over the workgroup's samples in ascending batch position (dh over k ascending); across workgroups the nb partial rows
 * and partial losses in ascending w, adds from +0; the loss is then divided by (float)batch.  No float atomics; two calls on the same
 * inputs give the same bytes.
 * workspace: at least rlhip_qrdqn_workspace_bytes(ns, h, na, N, batch) bytes (-1 for a refused shape); no initialisation.
 *
 * One update of rlhip.QRDQNLearner = draw -> gather -> this gradient -> [rlhip_per_priority_f32 on ql_out: (ql + eps)^alpha, written
 * back under the drawn keys] -> rlhip_clip_adam_f32 -> target sync.  Out of scope: IQN and FQF, kappa = 0 (the pure quantile loss, whose
 * gradient jumps at u = 0), NoisyDense, a fused vec-step, a gather inside the gradient launch, dueling, three-layer and bf16 nets,
 * sharded runs, UInt8 frames. */
int32_t rlhip_qrdqn_forward_f32(const float* params, int64_t ns, int64_t h, int64_t na, int64_t n_quantiles, int32_t act, const float* obs,
                                int64_t n, float* q_out, float* quantiles_out, rlhip_stream_t stream);
int32_t rlhip_qrdqn_plan_f32(const float* params, int64_t ns, int64_t h, int64_t na, int64_t n_quantiles, int32_t act, const float* obs,
                             int64_t n, double eps, uint64_t seed, uint32_t env_id_base, uint32_t step, int32_t* actions, float* q_out,
                             rlhip_stream_t stream);
int64_t rlhip_qrdqn_workspace_bytes(int64_t ns, int64_t h, int64_t na, int64_t n_quantiles, int64_t batch);
int32_t rlhip_qrdqn_grad_batch_f32(int64_t ns, int64_t h, int64_t na, int64_t n_quantiles, int32_t act, float kappa, const float* params,
                                   const float* target_params, const float* s, const int32_t* a, const float* r, const uint8_t* term,
                                   const float* s_next, int64_t batch, float gamma, const int32_t* n_used, const float* weights,
                                   int32_t double_dqn, void* workspace, float* grad_out, float* loss_out, float* ql_out, float* target_out,
                                   int32_t* sel_out, rlhip_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* RLHIP_H */

// fold_device.h -- the stages of the DQN replay fold kernels, each written once (device inline).
//
// A fold rewrites sampled transitions into complete 64-byte records of a batch-sized record ring, which every gradient kernel then
// takes unchanged: the n-step window fold {s, a, R, any(terminal), s_n} and the Double DQN fold {s, a, y, terminal = 1, s'}.  The
// kernels that are made of these stages keep their own launch shapes, LDS layouts and barriers:
//
//     fold_nstep_kernel (ring.hip)                    its own unrolled register walk            fold_store_record
//     fold_double_select_kernel (dqn_double.hip)      double_target                              fold_store_record
//     dqn_fold_double_kernel (dqn_double.hip)         biases, staging, two-net forward, target   fold_store_row
//     dqn_sample_fold_kernel (dqn_sample_fold.hip)    fold_window [+ the same four under DBL]    fold_store_row
//     per_sample_fold_nstep_kernel (per_nstep.hip)    sumtree_draw (sumtree_device.h), fold_window   fold_store_record
//
// Every stage has an independent second statement that the tests compare it with bit for bit: the CPU oracle (oracle/rlo_buffer.c,
// oracle/rlo_learn.c) for all of them, and for the window walk also fold_nstep_kernel, which deliberately does not call fold_window.
#pragma once
#include "mlp_device.h"
#include "ring_device.h"

namespace rlhip {

constexpr int FOLD_TILE = 64;         // samples per tile: one per lane of the gathering wavefront
constexpr int FOLD_THREADS = 1024;    // the tiled kernels: 16 waves, row = sample
constexpr int FOLD_MAX_BLOCKS = 512;  // ... grid-stride over the tiles beyond that
constexpr int FOLD_HMAX = 256;        // hidden units of a two-layer net staged in LDS
constexpr int FOLD_MAX_NSTEP = 32;    // the longest window: rows of the LDS reward column

// y = r + gamma * (1 - t) * Qt(s')[a*], a* = findmax(Q(s')) over the first `na` values (the first maximum wins: strict >): the
// gradient kernels' target line with Qt(s')[a*] in the place of the maximum.  (Scalars, not arrays: nothing to index at run time.)
__device__ __forceinline__ float double_target(float r, uint32_t term, float gamma, float q0, float q1, float q2, float q3, float t0,
                                               float t1, float t2, float t3, int na) {
    float m = q0, v = t0;
    if (na > 1 && q1 > m) m = q1, v = t1;
    if (na > 2 && q2 > m) m = q2, v = t2;
    if (na > 3 && q3 > m) m = q3, v = t3;
    const float cont = term ? 0.f : 1.f;
    return r + gamma * cont * v;
}

// the output biases of both nets (zeros beyond na): requested first, in flight across the staging and the barrier
template <int NS>
__device__ __forceinline__ void fold_load_out_biases(const float* params, const float* tparams, int h, int na, float bq[MAXO],
                                                     float btq[MAXO]) {
    const float* b2 = params + h * NS + h + na * h;
    const float* tb2 = tparams + h * NS + h + na * h;
#pragma unroll
    for (int o = 0; o < MAXO; ++o) {
        bq[o] = (o < na) ? b2[o] : 0.f;
        btq[o] = (o < na) ? tb2[o] : 0.f;
    }
}

// l_rec[net][j] = {W1[j, 0..3]}, {b1[j], W2[0..2, j]}, {W2[3, j], -, -, -} (rows beyond NS / na are zeros): dqn_grad_kernel's layout,
// net 0 = online, net 1 = target
using FoldNets = float4[2][FOLD_HMAX][3];

// both networks -> LDS, by all FOLD_THREADS lanes of the workgroup (the caller's barrier publishes them)
template <int NS>
__device__ __forceinline__ void fold_stage_two_nets(FoldNets& l_rec, const float* params, const float* tparams, int h, int na, int tid) {
    for (int q = tid; q < 2 * h; q += FOLD_THREADS) {
        const int net = q >= h ? 1 : 0, u = q - net * h;
        const float* P = net ? tparams : params;
        float w1[4] = {0.f, 0.f, 0.f, 0.f}, w2[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int k = 0; k < NS; ++k) w1[k] = P[u + h * k];
#pragma unroll
        for (int o = 0; o < MAXO; ++o)
            if (o < na) w2[o] = P[h * NS + h + o + na * u];
        l_rec[net][u][0] = make_float4(w1[0], w1[1], w1[2], w1[3]);
        l_rec[net][u][1] = make_float4(P[h * NS + u], w2[0], w2[1], w2[2]);
        l_rec[net][u][2] = make_float4(w2[3], 0.f, 0.f, 0.f);
    }
}

// Q(s') and Qt(s') of one sample on the 16 lanes of a DPP row: lane c walks hidden units c, c + 16, ... of both nets (the very
// accumulation order of the gradient kernel's Qt(s')), then group_sum_dpp<16> plus the bias.  q[o >= na] = qt[o >= na] = 0.
template <int NS, int ACT>
__device__ __forceinline__ void fold_two_net_q(const FoldNets& l_rec, nt_u32x4 sn, int h, int na, int c, const float bq[MAXO],
                                               const float btq[MAXO], float q[MAXO], float qt[MAXO]) {
    const float xn[4] = {__uint_as_float(sn[0]), __uint_as_float(sn[1]), __uint_as_float(sn[2]), __uint_as_float(sn[3])};
    float acc[MAXO] = {0.f, 0.f, 0.f, 0.f}, acn[MAXO] = {0.f, 0.f, 0.f, 0.f};  // online / target net, both on s'
#pragma unroll 2
    for (int jj = c; jj < h; jj += 16) {
        const float4 a0 = l_rec[0][jj][0], a1 = l_rec[0][jj][1], c0 = l_rec[1][jj][0], c1 = l_rec[1][jj][1];
        const float wa[4] = {a0.x, a0.y, a0.z, a0.w}, wc[4] = {c0.x, c0.y, c0.z, c0.w};
        float z = a1.x, zn = c1.x;
#pragma unroll
        for (int k = 0; k < NS; ++k) {
            z = fmaf(wa[k], xn[k], z);
            zn = fmaf(wc[k], xn[k], zn);
        }
        const float hv = act_fwd_t<ACT>(z), hn = act_fwd_t<ACT>(zn);
        acc[0] = fmaf(a1.y, hv, acc[0]);
        acn[0] = fmaf(c1.y, hn, acn[0]);
        acc[1] = fmaf(a1.z, hv, acc[1]);  // (rows o >= na are staged as zeros)
        acn[1] = fmaf(c1.z, hn, acn[1]);
        if (na > 2) {  // (uniform)
            acc[2] = fmaf(a1.w, hv, acc[2]);
            acn[2] = fmaf(c1.w, hn, acn[2]);
        }
        if (na == 4) {
            acc[3] = fmaf(l_rec[0][jj][2].x, hv, acc[3]);
            acn[3] = fmaf(l_rec[1][jj][2].x, hn, acn[3]);
        }
    }
#pragma unroll
    for (int o = 0; o < MAXO; ++o) {
        q[o] = 0.f, qt[o] = 0.f;
        if (o < na) {  // (uniform)
            q[o] = group_sum_dpp<16>(acc[o]) + bq[o];
            qt[o] = group_sum_dpp<16>(acn[o]) + btq[o];
        }
    }
}

// folded record b = {s, (a, r, term, 0), sn, zeros} stored by lanes c = 0..3 of a row: the four quarters of one 64-byte line, one
// store instruction.  `s` is read by lane 0 only (the callers hand in their LDS copy).
__device__ __forceinline__ void fold_store_row(uint8_t* out, int64_t* iota, int64_t b, int c, const nt_u32x4& s, uint32_t a, float r,
                                               uint32_t term, nt_u32x4 sn) {
    nt_u32x4 o4 = {0u, 0u, 0u, 0u};
    if (c == 0) o4 = s;
    else if (c == 1) o4 = nt_u32x4{a, __float_as_uint(r), term, 0u};
    else if (c == 2) o4 = sn;
    *reinterpret_cast<nt_u32x4*>(out + b * RING_REC_BYTES + 16 * c) = o4;
    if (c == 0 && iota) iota[b] = b;
}

// ... and by one lane: its own 64-byte line, all four quarters
__device__ __forceinline__ void fold_store_record(uint8_t* out, int64_t* iota, int64_t b, nt_u32x4 s, uint32_t a, float r, uint32_t term,
                                                  nt_u32x4 sn) {
    uint8_t* o = out + b * RING_REC_BYTES;
    *reinterpret_cast<nt_u32x4*>(o) = s;
    *reinterpret_cast<nt_u32x4*>(o + 16) = nt_u32x4{a, __float_as_uint(r), term, 0u};
    *reinterpret_cast<nt_u32x4*>(o + 32) = sn;
    *reinterpret_cast<nt_u32x4*>(o + 48) = nt_u32x4{0u, 0u, 0u, 0u};
    if (iota) iota[b] = b;
}

// The n-step window li .. li + ns - 1 of one env, up to and including the first terminal step and never past the newest stored
// transition (li + k < len_rt).  `cur` stands on the window's first record, whose reward r0, terminal flag `term` and s' `sn` the
// caller has loaded; each further record is one dependent 64-byte read, issued only once the step before is known not to be
// terminal.  The rewards wait in the lane's own LDS column l_rew[.][col] (consecutive dwords per step: conflict-free, no dynamically
// indexed register array, no barrier).  Leaves the last step's flag and s' in `term` / `sn` and returns discount_rewards_reduced over
// the window: gain = r[k] + gamma * gain from the window's end, Float32.
__device__ __forceinline__ float fold_window(float (&l_rew)[FOLD_MAX_NSTEP][FOLD_TILE], int col, RingCursor cur, int64_t li, int64_t len_rt,
                                             int n_step, float gamma, float r0, uint32_t& term, nt_u32x4& sn) {
    l_rew[0][col] = r0;
    int ns = 1;
    for (int k = 1; k < n_step && !term && li + k < len_rt; ++k) {
        const uint8_t* rk = cur.next();
        const nt_u32x4 kw = *reinterpret_cast<const nt_u32x4*>(rk + 16);
        sn = *reinterpret_cast<const nt_u32x4*>(rk + 32);
        l_rew[k][col] = __uint_as_float(kw[1]);
        term = (kw[2] & 0xffu) ? 1u : 0u;
        ns = k + 1;
    }
    float gain = 0.0f;
    for (int k = ns - 1; k >= 0; --k) gain = l_rew[k][col] + gamma * gain;
    return gain;
}

}  // namespace rlhip

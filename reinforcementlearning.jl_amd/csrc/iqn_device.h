// iqn_device.h -- the stages of an ImplicitQuantileNet's kernels that do not ask where the quantile levels come from, each written
// once: csrc/iqn.hip evaluates the network at levels it draws (Philox), csrc/fqf.hip at levels a fraction-proposal network places.
// Both read their levels from a per-sample LDS row, so everything behind that row is shared:
//   tile constants, iqn_nparams, IqnLds   the net-sized buffers in dynamic LDS
//   iqn_stage       Wphi | bphi (a straight copy: column-major h x n_cos is the B-operand image) and W2 | b2 of a net -> LDS
//   iqn_cos_block   c[row][e] = cospif((e + 1) tau_row) for a block of 32 rows -> LDS, rows 65 floats apart (the A-operand image)
//   iqn_phi_block   v_mfma_f32_32x32x2_f32: 32 rows x 32 hidden units per instruction, n_cos / 2 k-steps, bphi as the accumulator's
//                   initial value (the header's ascending-e fmaf chain bit for bit); wave w owns the unit blocks w, w + 4
//   iqn_head        one (row, head row): b2, then fmaf(W2[o, j], psi[j] * phi[j], .) over j ascending, operands from LDS
//   iqn_rows_all    the three above over all row blocks of a phase, every head row -> LDS
//   IQ_NET_BOUNDS   the bounds of the net, stated once
// include/rlhip.h (the IQN section) states the chains.
#pragma once
#include "dist_host.h"

namespace rlhip {

typedef float iq_f32x16 __attribute__((ext_vector_type(16)));

constexpr int IQ_T = 8;        // samples per tile
constexpr int IQ_NT = 256;     // threads
constexpr int IQ_RB = 32;      // rows per block (the M of the MFMA)
constexpr int IQ_MAXL = 64;    // levels per sample
constexpr int IQ_MAXC = 64;    // n_cos
constexpr int IQ_HMAX = 256;
constexpr int IQ_CS = IQ_MAXC + 1;          // cosine rows are 65 floats apart
constexpr int IQ_AS = IQ_MAXL + 1;          // per-sample level rows are 65 floats apart
constexpr int IQ_LS = MAXO * IQ_MAXL + 1;   // per-sample quantile rows (na * levels) are 257 floats apart
constexpr int IQ_W1U = (IQ_HMAX * 16 + IQ_HMAX + IQ_NT - 1) / IQ_NT;  // dW1 | db1 elements per thread (17)

__host__ __device__ __forceinline__ int64_t iqn_nparams(int64_t ns, int64_t h, int64_t na, int64_t nc) {
    return h * ns + h + h * nc + h + na * h + na;
}

// the net-sized buffers (dynamic LDS): Wphi | bphi, W2 as [o][j] | b2, psi [j][T], phi / dphi of a block [row][h + 1],
// dpsi / dz of the tile [i][h + 1] (gradient only)
struct IqnLds {
    float *wphi, *bphi, *w2, *psi, *phi, *dpsi;
};
__device__ __forceinline__ IqnLds iqn_lds(float* base, int h, int nc) {
    IqnLds L;
    L.wphi = base, L.bphi = L.wphi + nc * h, L.w2 = L.bphi + h, L.psi = L.w2 + MAXO * h + MAXO, L.phi = L.psi + h * IQ_T;
    L.dpsi = L.phi + IQ_RB * (h + 1);
    return L;
}
static size_t iqn_lds_bytes(int64_t h, int64_t nc, bool grad) {
    return sizeof(float) * (size_t)(nc * h + h + MAXO * h + MAXO + h * IQ_T + IQ_RB * (h + 1) + (grad ? IQ_T * (h + 1) : 0));
}

// Wphi | bphi (contiguous in the vector) and the head of net P -> LDS
__device__ __forceinline__ void iqn_stage(const float* __restrict__ P, int ns, int h, int na, int nc, const IqnLds& L) {
    const float* Wp = P + h * ns + h;
    const float4* src = reinterpret_cast<const float4*>(Wp);  // (h (ns + 1) floats into the vector: h is a multiple of 32)
    float4* dst = reinterpret_cast<float4*>(L.wphi);
    for (int q = threadIdx.x; q < (nc * h + h) / 4; q += IQ_NT) dst[q] = src[q];
    const float* W2 = Wp + nc * h + h;
    for (int q = threadIdx.x; q < MAXO * h; q += IQ_NT) {
        const int o = q / h, j = q - o * h;
        L.w2[q] = o < na ? W2[o + na * j] : 0.f;
    }
    if (threadIdx.x < MAXO) L.w2[MAXO * h + threadIdx.x] = (int)threadIdx.x < na ? W2[na * h + threadIdx.x] : 0.f;
}

// c[r][e] = cospif((float)(e + 1) * tau) for the rows row0 .. row0 + 31 of a phase whose row = level + NL * sample; rows beyond
// nrows and features beyond n_cos are zero (they are operands of the dWphi product)
__device__ __forceinline__ void iqn_cos_block(const float* l_tau, int NL, int row0, int nrows, int nc, float* l_c) {
    for (int q = threadIdx.x; q < IQ_RB * IQ_MAXC; q += IQ_NT) {
        const int r = q / IQ_MAXC, e = q % IQ_MAXC, row = row0 + r;
        float v = 0.f;
        if (row < nrows && e < nc) {
            const int i = row / NL;
            v = cospif((float)(e + 1) * l_tau[i * IQ_AS + (row - i * NL)]);
        }
        l_c[r * IQ_CS + e] = v;
    }
}

// phi[r][j] = max(bphi[j], then fmaf(Wphi[j, e], c[r][e], .) over e ascending, 0) for the block's 32 rows and all h units
__device__ __forceinline__ void iqn_phi_block(const IqnLds& L, const float* l_c, int h, int nc) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, c = lane & 31, kb = lane >> 5;
    for (int jb = wave; jb * 32 < h; jb += IQ_NT / 64) {
        const int j = jb * 32 + c;
        const float b = L.bphi[j];
        iq_f32x16 acc;
#pragma unroll
        for (int q = 0; q < 16; ++q) acc[q] = b;
        for (int ks = 0; ks < nc / 2; ++ks) {
            const int e = 2 * ks + kb;  // A[m = row c][k = e], B[k = e][n = unit j]
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(l_c[c * IQ_CS + e], L.wphi[e * h + j], acc, 0, 0, 0);
        }
#pragma unroll
        for (int q = 0; q < 16; ++q) L.phi[((q & 3) + 8 * (q >> 2) + 4 * kb) * (h + 1) + j] = fmaxf(acc[q], 0.f);
    }
}

// th of block row r (sample slot i), head row o: b2[o], then fmaf(W2[o, j], psi[j] * phi[j], .) over j ascending
__device__ __forceinline__ float iqn_head(const IqnLds& L, int h, int r, int i, int o) {
    const float* w = L.w2 + o * h;
    const float* ph = L.phi + r * (h + 1);
    const float* ps = L.psi + i;
    float acc = L.w2[MAXO * h + o];
    for (int j0 = 0; j0 < h; j0 += 8) {  // (h is a multiple of 32) the operands of eight steps in flight; the chain stays j ascending
        float m[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) m[u] = ps[(j0 + u) * IQ_T] * ph[j0 + u];
#pragma unroll
        for (int u = 0; u < 8; ++u) acc = fmaf(w[j0 + u], m[u], acc);
    }
    return acc;
}

// all na head rows of the nrows = nv * NL rows of a phase -> l_th[i][level + NL * o].  The net is staged and psi written by the
// caller (no barrier needed in between: the first one below orders them)
__device__ __forceinline__ void iqn_rows_all(const IqnLds& L, const float* l_tau, int NL, int nrows, int h, int na, int nc, float* l_c,
                                             float* l_th) {
    for (int row0 = 0; row0 < nrows; row0 += IQ_RB) {
        iqn_cos_block(l_tau, NL, row0, nrows, nc, l_c);
        __syncthreads();  // (also: the head of the previous block is done with phi)
        iqn_phi_block(L, l_c, h, nc);
        __syncthreads();
        const int r = threadIdx.x & 31, o = threadIdx.x >> 5, row = row0 + r;
        if (o < na && row < nrows) {
            const int i = row / NL;
            l_th[i * IQ_LS + o * NL + (row - i * NL)] = iqn_head(L, h, r, i, o);
        }
    }
    __syncthreads();
}

// the bounds of the net, each stated once (dist_host.h: a list of bounds hands each one to B)
#define IQ_NET_BOUNDS(B)                                                                  \
    B(ns >= 2 && ns <= 16, "obs dim must be 2..16");                                      \
    B(h >= 32 && h <= IQ_HMAX && h % 32 == 0, "hidden must be a multiple of 32, <= 256"); \
    B(na >= 1 && na <= MAXO, "na must be 1..4");                                          \
    B(n_cos >= 2 && n_cos <= IQ_MAXC && n_cos % 2 == 0, "n_cos must be even, 2..64")

static bool iqn_net_ok(int64_t ns, int64_t h, int64_t na, int64_t n_cos) {
    IQ_NET_BOUNDS(DIST_BOUND_HOLDS);
    return true;
}

#define IQ_REQUIRE_NET()           \
    IQ_NET_BOUNDS(RLHIP_REQUIRE);  \
    DIST_REQUIRE_ACT()

}  // namespace rlhip

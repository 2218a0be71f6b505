// ppo_advnorm.hip -- PPO advantage normalisation (rlhip_ppo_cfg.normalize_advantage = 1).
//
// The removed RLZoo PPO's option, as the oracle states it (oracle/rlo_learn.c, rlo_ppo_loss_grad_f32): per (epoch, micro-batch)
// of bm = n T / n_microbatches samples -- the ones the epoch's permutation puts at positions [mb bm, (mb + 1) bm) -- a Float64
// mean, the corrected two-pass std (divisor bm - 1, or 1 when bm <= 1) clamped to [1e-8, 1000], then
// adv = (float)((adv - mu) / sd), rounded once.  Samples left out of a ragged epoch belong to no micro-batch.
//
// Binned form (n_microbatches <= AB_MAX_BINS, every PPO configuration in use): three launches per epoch over the trajectory in
// its own order, one thread per 4 entries f, 1024 entries per workgroup -- adv is read coalesced and each entry is binned ONCE
// per epoch by its position in the permutation, p = invperm(f) (the Feistel rounds run backwards, then cycle-walk), bin p / bm:
//   pass 0  bin[f] stored; per-bin Float64 sums -> part[wg][bin]; the last workgroup out folds the rows -> mu[bin]
//   pass 1  per-bin sums of (x - mu)^2 -> part[wg][bin]; the last workgroup out -> sd[bin] (corrected, clamped)
//   pass 2  out[f] = (float)((x - mu[bin]) / sd[bin]), coalesced
// Every sum has a fixed order (per thread over its 4 entries, the __shfl_down / DPP wave tree, the four waves in index order,
// the workgroup rows through one fixed block tree), so results are bit-identical from run to run; they differ from the
// oracle's sequential sums only by the order of the Float64 additions.  Which workgroup leaves last does not matter: it folds
// all rows in the same order.  profiles/advnorm.md has the same-box A / B against the gather form below.
// Gather form (n_microbatches > AB_MAX_BINS: many small micro-batches, where per-bin rows would grow as n_mb x workgroups):
// one workgroup per 2048 positions of a micro-batch gathers adv[perm(p)] in three passes (sum, squared deviations, write).
// The device-counter form reads ctr[1] (the update counter) and derives the epoch keys in the kernel like ppo_grad_kernel:
// epoch = epoch_local + ctr[1] n_epochs.  No host work between the launches: graph-capturable.
#include "ppo_common.h"

namespace rlhip {

constexpr int AN_THREADS = 256;
constexpr int AN_PER = 8;                       // gather form: positions per thread
constexpr int AN_CHUNK = AN_THREADS * AN_PER;  // gather form: positions per workgroup
constexpr int AB_PER = 4;                       // binned form: entries per thread
constexpr int AB_CHUNK = AN_THREADS * AB_PER;  // binned form: entries per workgroup
constexpr int AB_MAX_BINS = 64;
constexpr uint32_t AB_NONE = 0xFFFFFFFFu;

// the inverse of permute() (common.h): the six rounds backwards, cycle-walking until the value is inside [0, n)
__host__ __device__ __forceinline__ uint32_t inv_permute(const PermKeys& pk, uint32_t y) {
    if (pk.n <= 1) return 0;
    uint32_t x = y;
    do {
        uint32_t L = (x >> pk.h) & pk.mask, R = x & pk.mask;
#pragma unroll
        for (int r = 5; r >= 0; --r) {
            const uint32_t pr = L;
            const uint32_t pl = R ^ (feistel_f(L, pk.k[r]) & pk.mask);
            L = pl;
            R = pr;
        }
        x = (L << pk.h) | R;
    } while (x >= pk.n);
    return x;
}

__device__ __forceinline__ double clamp_sd(double s2, uint32_t bm) {
    double sd = sqrt(s2 / (double)(bm > 1 ? bm - 1 : 1));
    if (sd < 1e-8) sd = 1e-8;
    if (sd > 1000.0) sd = 1000.0;
    return sd;
}

// ------------------------------------------------------------------------------------------------------------ binned form
struct AdvBinArgs {
    const float* adv;       // [total], trajectory order f = t n + i
    float* out;             // [total]
    uint32_t* bin;          // [total]: micro-batch of entry f in this epoch, AB_NONE for none (pass 0 writes, 1 and 2 read)
    double* part;           // [nwg][nbins] per-workgroup rows
    double* stats;          // [nbins][2] {mu, sd}
    unsigned int* counter;  // departure counter: zero between launches (the last workgroup out re-arms it)
    double* stats_out;      // nullable: {mu, sd} of bin `only` (pass 2)
    PermKeys pk;            // the epoch's keys ...
    const uint32_t* ctr;    // ... or, when non-NULL, derived in the kernel from ctr[1]
    uint64_t seed;
    uint32_t epoch_local, n_epochs;
    uint32_t total, bm;
    int nbins, nwg;
    int only;               // pass 2: write the entries of this micro-batch only (-1: all)
};

template <int PASS>
__global__ __launch_bounds__(AN_THREADS) void ppo_advnorm_bin_kernel(AdvBinArgs a) {
    __shared__ double l_w[AN_THREADS / 64][AB_MAX_BINS];
    __shared__ double l_s[16];
    __shared__ int l_last;
    const int lane = (int)threadIdx.x & 63, wid = (int)threadIdx.x >> 6;
    uint32_t f[AB_PER], b[AB_PER];
    float x[AB_PER];
    if (PASS == 0) {
        const PermKeys pk = a.ctr ? perm_keys(a.seed, a.epoch_local + a.ctr[1] * a.n_epochs, a.total) : a.pk;
        const uint32_t covered = (uint32_t)a.nbins * a.bm;
#pragma unroll
        for (int k = 0; k < AB_PER; ++k) {
            f[k] = blockIdx.x * AB_CHUNK + (uint32_t)(k * AN_THREADS) + threadIdx.x;
            b[k] = AB_NONE;
            if (f[k] < a.total) {
                const uint32_t p = inv_permute(pk, f[k]);
                b[k] = p < covered ? p / a.bm : AB_NONE;
                a.bin[f[k]] = b[k];
            }
        }
    } else {
#pragma unroll
        for (int k = 0; k < AB_PER; ++k) {
            f[k] = blockIdx.x * AB_CHUNK + (uint32_t)(k * AN_THREADS) + threadIdx.x;
            b[k] = f[k] < a.total ? a.bin[f[k]] : AB_NONE;
        }
    }
#pragma unroll
    for (int k = 0; k < AB_PER; ++k) x[k] = f[k] < a.total ? a.adv[f[k]] : 0.0f;
    if (PASS == 2) {
#pragma unroll
        for (int k = 0; k < AB_PER; ++k) {
            if (b[k] == AB_NONE || (a.only >= 0 && b[k] != (uint32_t)a.only)) continue;
            const double mu = a.stats[2 * b[k]], sd = a.stats[2 * b[k] + 1];
            a.out[f[k]] = (float)(((double)x[k] - mu) / sd);
        }
        if (a.stats_out && blockIdx.x == 0 && threadIdx.x == 0) {
            a.stats_out[0] = a.stats[2 * a.only];
            a.stats_out[1] = a.stats[2 * a.only + 1];
        }
        return;
    }
    // this workgroup's row: per bin, the thread's entries in k order -> wave tree -> waves in index order
    for (int bb = 0; bb < a.nbins; ++bb) {
        const double mu = PASS == 1 ? a.stats[2 * bb] : 0.0;
        double s = 0.0;
#pragma unroll
        for (int k = 0; k < AB_PER; ++k) {
            if (b[k] != (uint32_t)bb) continue;
            if (PASS == 0) {
                s += (double)x[k];
            } else {
                const double d = (double)x[k] - mu;
                s += d * d;
            }
        }
        s = wave_sum_down_f64_lane0(s);
        if (lane == 0) l_w[wid][bb] = s;
    }
    __syncthreads();
    if ((int)threadIdx.x < a.nbins) {
        double v = 0.0;
#pragma unroll
        for (int w = 0; w < AN_THREADS / 64; ++w) v += l_w[w][threadIdx.x];
        a.part[(int64_t)blockIdx.x * a.nbins + threadIdx.x] = v;
        __threadfence();  // release this workgroup's row (agent scope), by the threads that wrote it
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned int prev = __hip_atomic_fetch_add(a.counter, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
        l_last = prev == (unsigned int)a.nwg - 1u;
    }
    __syncthreads();
    if (!l_last) return;
    __threadfence();  // acquire every other workgroup's row
    // the last workgroup out folds the rows of every bin in one fixed order
    for (int bb = 0; bb < a.nbins; ++bb) {
        double s = 0.0;
        for (int w = (int)threadIdx.x; w < a.nwg; w += AN_THREADS) s += a.part[(int64_t)w * a.nbins + bb];
        s = block_sum_f64_dpp(s, l_s);
        if (threadIdx.x == 0) {
            if (PASS == 0) a.stats[2 * bb] = s / (double)a.bm;
            else a.stats[2 * bb + 1] = clamp_sd(s, a.bm);
        }
    }
    if (threadIdx.x == 0) __hip_atomic_store(a.counter, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ------------------------------------------------------------------------------------------------------------ gather form
struct AdvNormArgs {
    const float* adv;     // [total], trajectory order f = t n + i
    float* out;           // [total]: the normalised advantages of the micro-batches [mb0, mb0 + gridDim.x / chunks)
    double* part1;        // [n_mb][chunks] sums
    double* part2;        // [n_mb][chunks] sums of squared deviations
    double* stats;        // [n_mb][2] {mu, sd} (nullable)
    PermKeys pk;          // the epoch's keys ...
    const uint32_t* ctr;  // ... or, when non-NULL, derived in the kernel from ctr[1]
    uint64_t seed;
    uint32_t epoch_local, n_epochs;
    uint32_t total, bm, mb0;
    int chunks;
};

template <int PASS>
__global__ __launch_bounds__(AN_THREADS) void ppo_advnorm_kernel(AdvNormArgs a) {
    __shared__ double l_s[16];
    const PermKeys pk = a.ctr ? perm_keys(a.seed, a.epoch_local + a.ctr[1] * a.n_epochs, a.total) : a.pk;
    const int mb = (int)blockIdx.x / a.chunks, chunk = (int)blockIdx.x - mb * a.chunks;
    const uint32_t p0 = (a.mb0 + (uint32_t)mb) * a.bm;
    const uint32_t c0 = (uint32_t)chunk * AN_CHUNK;
    const uint32_t c1 = c0 + AN_CHUNK < a.bm ? c0 + AN_CHUNK : a.bm;
    const double* p1 = a.part1 + (int64_t)mb * a.chunks;
    double mu = 0.0, sd = 1.0;
    if (PASS >= 1) {
        double s = 0.0;
        for (int c = (int)threadIdx.x; c < a.chunks; c += AN_THREADS) s += p1[c];
        mu = block_sum_f64_dpp(s, l_s) / (double)a.bm;
    }
    if (PASS == 2) {
        const double* p2 = a.part2 + (int64_t)mb * a.chunks;
        double s = 0.0;
        for (int c = (int)threadIdx.x; c < a.chunks; c += AN_THREADS) s += p2[c];
        sd = clamp_sd(block_sum_f64_dpp(s, l_s), a.bm);
    }
    // all permutations first, then all loads
    uint32_t f[AN_PER];
    float x[AN_PER];
#pragma unroll
    for (int k = 0; k < AN_PER; ++k) {
        const uint32_t q = c0 + (uint32_t)threadIdx.x + (uint32_t)(k * AN_THREADS);
        f[k] = q < c1 ? permute(pk, p0 + q) : 0xFFFFFFFFu;
    }
#pragma unroll
    for (int k = 0; k < AN_PER; ++k) x[k] = f[k] != 0xFFFFFFFFu ? a.adv[f[k]] : 0.0f;
    if (PASS == 2) {
#pragma unroll
        for (int k = 0; k < AN_PER; ++k)
            if (f[k] != 0xFFFFFFFFu) a.out[f[k]] = (float)(((double)x[k] - mu) / sd);
        if (a.stats && chunk == 0 && threadIdx.x == 0) {
            a.stats[2 * mb] = mu;
            a.stats[2 * mb + 1] = sd;
        }
        return;
    }
    double acc = 0.0;
#pragma unroll
    for (int k = 0; k < AN_PER; ++k) {
        if (f[k] == 0xFFFFFFFFu) continue;
        if (PASS == 0) {
            acc += (double)x[k];
        } else {
            const double d = (double)x[k] - mu;
            acc += d * d;
        }
    }
    acc = block_sum_f64_dpp(acc, l_s);
    if (threadIdx.x == 0) (PASS == 0 ? a.part1 : a.part2)[(int64_t)mb * a.chunks + chunk] = acc;
}

// ------------------------------------------------------------------------------------------------------------------ host
static int64_t round256(int64_t b) { return (b + 255) / 256 * 256; }
static int advnorm_chunks(int64_t bm) { return (int)((bm + AN_CHUNK - 1) / AN_CHUNK); }
static bool binned(int64_t nmb) { return nmb <= AB_MAX_BINS; }
static bool g_force_gather = false;  // test / measurement hook: the gather form at any n_microbatches (fits the binned scratch)
static int64_t bin_wgs(int64_t total) { return (total + AB_CHUNK - 1) / AB_CHUNK; }

// scratch of one epoch's launches (after the plane): binned: bin [total] u32 | rows [nwg][n_mb] f64 | stats [n_mb][2] f64 |
// counter (64 B);  gather: part1, part2 [n_mb][chunks] f64 | stats [n_mb][2] f64
static int64_t scratch_bytes(int64_t total, int64_t nmb) {
    if (binned(nmb)) return round256(4 * total) + round256(8 * bin_wgs(total) * nmb + 16 * nmb) + 256;
    return round256(16 * nmb * ((int64_t)advnorm_chunks(total / nmb) + 1));
}

int64_t advnorm_region_bytes(const rlhip_ppo_cfg* c, int64_t n, int64_t T) {
    const int64_t total = n * T, nmb = c->n_microbatches;
    if (total < 1 || nmb < 1 || total / nmb < 1) return 0;
    return round256(4 * total) + scratch_bytes(total, nmb);
}

// scratch: scratch_bytes(total, n_mb) bytes, 256-aligned, its counter zero.  only = -1: every micro-batch into `out`.
static int32_t advnorm_launch(const rlhip_ppo_cfg* c, int64_t n, int64_t T, const float* adv, uint64_t seed, uint32_t epoch,
                              const uint32_t* ctr, int32_t only, float* out, char* scratch, double* stats_out, hipStream_t s) {
    RLHIP_REQUIRE(c != nullptr && adv != nullptr && out != nullptr, "NULL argument");
    RLHIP_REQUIRE(n >= 1 && T >= 1 && n * T <= 0x7FFFFFFFll, "n * T out of range");
    const int32_t nmb = c->n_microbatches;
    RLHIP_REQUIRE(nmb >= 1 && only >= -1 && only < nmb, "bad micro-batch index");
    const int64_t total = n * T, bm = total / nmb;
    RLHIP_REQUIRE(bm >= 1, "micro-batch is empty");
    const PermKeys pk = perm_keys(seed, epoch, (uint32_t)total);
    if (binned(nmb) && !g_force_gather) {
        AdvBinArgs a;
        a.adv = adv;
        a.out = out;
        a.bin = (uint32_t*)scratch;
        a.nwg = (int)bin_wgs(total);
        a.nbins = nmb;
        a.part = (double*)(scratch + round256(4 * total));
        a.stats = a.part + (int64_t)a.nwg * nmb;
        a.counter = (unsigned int*)(scratch + scratch_bytes(total, nmb) - 256);
        a.stats_out = only >= 0 ? stats_out : nullptr;
        a.pk = pk;
        a.ctr = ctr;
        a.seed = seed;
        a.epoch_local = epoch;
        a.n_epochs = (uint32_t)c->n_epochs;
        a.total = (uint32_t)total;
        a.bm = (uint32_t)bm;
        a.only = only;
        hipLaunchKernelGGL(ppo_advnorm_bin_kernel<0>, dim3((unsigned)a.nwg), dim3(AN_THREADS), 0, s, a);
        hipLaunchKernelGGL(ppo_advnorm_bin_kernel<1>, dim3((unsigned)a.nwg), dim3(AN_THREADS), 0, s, a);
        hipLaunchKernelGGL(ppo_advnorm_bin_kernel<2>, dim3((unsigned)a.nwg), dim3(AN_THREADS), 0, s, a);
        RLHIP_LAUNCH_CHECK();
        return RLHIP_OK;
    }
    const int32_t mb0 = only >= 0 ? only : 0, nrun = only >= 0 ? 1 : nmb;
    AdvNormArgs a;
    a.adv = adv;
    a.out = out;
    a.chunks = advnorm_chunks(bm);
    a.part1 = (double*)scratch;
    a.part2 = a.part1 + (int64_t)nrun * a.chunks;
    a.stats = only >= 0 && stats_out ? stats_out : a.part2 + (int64_t)nrun * a.chunks;
    a.pk = pk;
    a.ctr = ctr;
    a.seed = seed;
    a.epoch_local = epoch;
    a.n_epochs = (uint32_t)c->n_epochs;
    a.total = (uint32_t)total;
    a.bm = (uint32_t)bm;
    a.mb0 = (uint32_t)mb0;
    const int64_t nb = (int64_t)nrun * a.chunks;
    RLHIP_REQUIRE(nb <= 0x7FFFFFFFll, "too many workgroups");
    hipLaunchKernelGGL(ppo_advnorm_kernel<0>, dim3((unsigned)nb), dim3(AN_THREADS), 0, s, a);
    hipLaunchKernelGGL(ppo_advnorm_kernel<1>, dim3((unsigned)nb), dim3(AN_THREADS), 0, s, a);
    hipLaunchKernelGGL(ppo_advnorm_kernel<2>, dim3((unsigned)nb), dim3(AN_THREADS), 0, s, a);
    RLHIP_LAUNCH_CHECK();
    return RLHIP_OK;
}

// every micro-batch of one epoch into the plane of the workspace's normalisation region, which starts at the flag-off workspace
// size rounded up to 256 bytes.  epoch: the epoch counter, or with ctr the epoch inside the update call.
int32_t advnorm_epoch(int32_t kind, const rlhip_ppo_cfg* c, int64_t n, int64_t T, const float* adv, uint64_t seed,
                      uint32_t epoch, const uint32_t* ctr, void* workspace, float** plane, hipStream_t s) {
    RLHIP_REQUIRE(c != nullptr && workspace != nullptr && plane != nullptr, "NULL argument");
    rlhip_ppo_cfg off = *c;
    off.normalize_advantage = 0;
    const int64_t base = rlhip_ppo_workspace_bytes(kind, &off, n, T);
    RLHIP_REQUIRE(base > 0, "bad configuration");
    char* region = (char*)workspace + round256(base);
    float* out = (float*)region;
    int32_t rc = advnorm_launch(c, n, T, adv, seed, epoch, ctr, -1, out, region + round256(4 * n * T), nullptr, s);
    if (rc) return rc;
    *plane = out;
    return RLHIP_OK;
}

}  // namespace rlhip

using namespace rlhip;

/* measurement hook, not part of include/rlhip.h: 1 = the gather form for every configuration (profiles/advnorm.md A / B) */
extern "C" int32_t rlhip_debug_advnorm_gather(int32_t on) {
    g_force_gather = on != 0;
    return RLHIP_OK;
}

extern "C" int32_t rlhip_ppo_adv_normalize_f32(const rlhip_ppo_cfg* cfg, int64_t n, int64_t T, const float* adv, uint64_t seed,
                                               uint32_t epoch_ctr, int32_t mb, float* adv_out, double* stats_out,
                                               rlhip_stream_t stream) {
    RLHIP_REQUIRE(cfg != nullptr && adv != nullptr && adv_out != nullptr, "NULL argument");
    RLHIP_REQUIRE(n >= 1 && T >= 1 && n * T <= 0x7FFFFFFFll, "n * T out of range");
    RLHIP_REQUIRE(cfg->n_microbatches >= 1 && mb >= 0 && mb < cfg->n_microbatches, "bad micro-batch index");
    RLHIP_REQUIRE((n * T) / cfg->n_microbatches >= 1, "micro-batch is empty");
    // the launches' scratch lives in a stream-ordered allocation of this call (its departure counter zeroed)
    const int64_t bytes = scratch_bytes(n * T, cfg->n_microbatches);
    hipStream_t s = as_stream(stream);
    char* scratch = nullptr;
    RLHIP_CHECK_HIP(hipMallocAsync((void**)&scratch, (size_t)bytes, s));
    if (binned(cfg->n_microbatches)) RLHIP_CHECK_HIP(hipMemsetAsync(scratch + bytes - 256, 0, 256, s));
    int32_t rc = advnorm_launch(cfg, n, T, adv, seed, epoch_ctr, nullptr, mb, adv_out, scratch, stats_out, s);
    RLHIP_CHECK_HIP(hipFreeAsync(scratch, s));
    return rc;
}

// record_slot32.h -- position of flat parameter q in the unit-record image (ppo_grad_tile.h: pack_records), in 32-bit
// arithmetic.  No HIP header: a host program includes it as it stands (tests/record_slot32/record_slot32_check.cc compares
// it with the 64-bit formula of ppo_grad_tile.h `record_slot` for every parameter of every supported net).
//
// Why a second form: the Adam tail of reduce_apply_kernel (ppo_grad.hip) patches one word of the image per lane.  The
// 64-bit `%` and `/` of `record_slot` compile to ~440 lines of division code, and one wave per SIMD walks them with
// nothing to hide them behind.  The two-layer learner has h <= 256, ns <= 4, nout <= 3 (prepare_grad), so every quantity
// here is below 2^12: one 32-bit unsigned division by h (the remainder by a multiply and a subtract) and a division by
// the actor's output count, which is 1, 2 or 3 -- selected, so the compiler divides by constants.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define RLHIP_SLOT_HD __host__ __device__
#else
#define RLHIP_SLOT_HD
#endif

namespace rlhip {

constexpr uint32_t RECORD_FLOATS = 16;  // floats per unit record (= REC of ppo_grad_tile.h)

// q < np_a + (h ns + 2 h + 1), h >= 1, ns >= 1, 1 <= nout <= 3; np_a = h ns + h + nout h + nout
RLHIP_SLOT_HD inline uint32_t record_slot32(uint32_t q, uint32_t h, uint32_t ns, uint32_t nout, uint32_t np_a) {
    const uint32_t net = q >= np_a ? 1u : 0u;
    const uint32_t r = q - (net ? np_a : 0u);
    const uint32_t no = net ? 1u : nout;
    const uint32_t hn = h * ns;
    if (r < hn) {  // W1[j + h k] -> rec[j][2 k + net]
        const uint32_t k = r / h, j = r - k * h;
        return RECORD_FLOATS * j + 2u * k + net;
    }
    if (r < hn + h) return RECORD_FLOATS * (r - hn) + 8u + net;  // b1[j] -> rec[j][8 + net]
    const uint32_t w = r - (hn + h);
    if (w < no * h) {
        if (net) return RECORD_FLOATS * w + 11u;  // W2c[j] -> rec[j][11]
        const uint32_t j = no == 1u ? w : (no == 2u ? w / 2u : w / 3u), o = w - j * no;
        return RECORD_FLOATS * j + (o == 0u ? 10u : 11u + o);  // W2a[o + no j] -> rec[j][10 | 12 | 13]
    }
    return RECORD_FLOATS * h + (net ? 3u : w - no * h);  // output biases -> tail
}

}  // namespace rlhip

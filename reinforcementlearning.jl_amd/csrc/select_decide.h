// select_decide.h -- the two-action Gumbel-max decision without the log-sum-exp (the fused rollout's dependent chain,
// ppo.hip).  Plain C++: no HIP builtins, so that a host program can include it (tests/fast_select/fuzz_main.cpp fuzzes it
// against the exact rule).
//
// The exact rule (categorical_select1, select_device.h, two actions, no mask), RN32 / RN64 = round to nearest Float32 / Float64:
//     mx   = max(x0, x1)                      a_k  = RN32(x_k - mx)        one of a_0, a_1 is +0, the other is d <= 0
//     se   = RN32(1 + RN32(exp d))            lse  = RN32(log se)          0 <= lse <= RN32(log 2) < 0.6932
//     lp_k = RN32(a_k - lse)                  G_k  = RN64(nz_k + lp_k)     action = G_1 > G_0 ? 1 : 0
// The fast rule: D = RN64(RN64(nz_1 - nz_0) + (a_1 - a_0)) (a_1 - a_0 = +-d is exact in Float64), action = D > 0 ? 1 : 0,
// decided only when |D| > thr.  With D* = (nz_1 - nz_0) + (a_1 - a_0) in real arithmetic and u32 = 2^-24, u64 = 2^-53 the
// relative errors of one rounding (a Float32 difference that lands in the subnormals is exact), the four roundings of the
// exact rule move G_1 - G_0 away from D* by at most
//     two Float32 roundings of a_k - lse:  u32 (|a_0 - lse| + |a_1 - lse|) = u32 (|d| + 2 lse)       <= 2^-24 (|d| + 1.3864)
//     two Float64 roundings of nz_k + lp_k: u64 (|nz_0| + |nz_1| + |lp_0| + |lp_1|)                   <= 2^-53 (|nz_0| + |nz_1| + |d| + 1.4)
// (lse cancels in lp_1 - lp_0 up to exactly those roundings), and the two Float64 roundings of the fast rule move D away
// from D* by at most u64 |nz_1 - nz_0| + u64 |D|                                                       <= 2^-53 (2 |nz_0| + 2 |nz_1| + |d|) (1 + u64)
// Sum: E <= 2^-24 (|d| + 1.39) + 2^-53 * 3.01 (|nz_0| + |nz_1| + |d| + 1).  |D| > E implies that D and G_1 - G_0 have the same
// strict sign, i.e. both rules pick the same action (the exact rule's tie G_1 == G_0 -> action 0 cannot occur).  The shipped
// threshold keeps a factor of >= 4 over the Float32 part and >= 10 over the Float64 part (which also covers the roundings of
// evaluating thr itself):
//     thr = 2^-22 (|d| + 2) + 2^-48 (|nz_0| + |nz_1| + |d| + 2)
// `margin` (>= 1; RLHIP_ROLLOUT_SELECT_MARGIN) multiplies it; at +inf nothing is decided.
// Non-finite operands: a NaN logit, d = -inf or inf - inf make d (hence thr) NaN or inf; an infinite or NaN noise makes thr
// inf or NaN; an overflowing nz_1 - nz_0 implies an overflowing |nz_0| + |nz_1|.  `!(|D| > thr)` is true in all of them:
// undecided, the caller runs the exact rule.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define RLHIP_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define RLHIP_HD inline
#endif

namespace rlhip {

// The rule in two halves, so that the rollout kernel evaluates the half that depends on (env, step) alone with the noise, off
// the dependent chain.  With e = RN32(x_1 - x_0): for finite logits a_1 - a_0 = e and d = -|e| (rounding is symmetric under
// negation and x - x = +0), so
//     D   = RN64(dn + e)                         dn = RN64(nz_1 - nz_0)
//     thr = tn + km |e|                          tn = margin (2^-21 + 2^-48 (|nz_0| + |nz_1| + 2)),  km = margin (2^-22 + 2^-48)
// which is the threshold above with its terms regrouped (its own roundings are ~2^-52 relative, inside the spare factor).
// Non-finite logits make e -- hence D or thr -- inf or NaN: undecided.
RLHIP_HD void decide2_noise_terms(double nz0, double nz1, double margin, double* dn, double* tn) {
    *dn = nz1 - nz0;
    *tn = margin * (0x1p-21 + 0x1p-48 * (__builtin_fabs(nz0) + __builtin_fabs(nz1) + 2.0));
}
RLHIP_HD double decide2_slope(double margin) { return margin * (0x1p-22 + 0x1p-48); }

// Returns the rule's action (D > 0 ? 1 : 0: the exact rule's action when *decided) and e.
RLHIP_HD int decide2_logits(float x0, float x1, double dn, double tn, double km, float* e_out, bool* decided) {
    const float e = x1 - x0;
    const double D = dn + (double)e;
    const double thr = tn + km * __builtin_fabs((double)e);
    const bool undecided = !(__builtin_fabs(D) > thr);  // this form: a NaN on either side is undecided
    *e_out = e;
    *decided = !undecided;
    return (D > 0.0) ? 1 : 0;
}

// The operands of logp = a_best - lse, se = 1 + exp(d), of a DECIDED draw (finite logits) that took `action`: bit for bit
// what select2_operands gives (tests/fast_select/fuzz_main.cpp compares them).
RLHIP_HD void decide2_operands(float x0, float x1, float e, int action, float* a_best, float* d) {
    const bool gt = x1 > x0;  // the maximum is x_1: a_1 = +0, a_0 = d
    const float d_ = gt ? -e : e;
    *d = d_;
    *a_best = ((action != 0) == gt) ? 0.0f : d_;
}

// mx, other and the differences exactly as categorical_select1 forms them, any operands: a_k = RN32(x_k - mx), d = RN32(other - mx)
RLHIP_HD void select2_operands(float x0, float x1, float* a0, float* a1, float* d) {
    float mx = -__builtin_inff();
    if (x0 > mx) mx = x0;
    if (x1 > mx) mx = x1;
    const float other = (x1 > x0) ? x0 : x1;
    *a0 = x0 - mx;
    *a1 = x1 - mx;
    *d = other - mx;
}

// both halves at once: the action, a_best and d of the rule, and whether it decided
RLHIP_HD int categorical_decide2(float x0, float x1, double nz0, double nz1, double margin, float* a_best, float* d, bool* decided) {
    double dn, tn;
    float e;
    decide2_noise_terms(nz0, nz1, margin, &dn, &tn);
    const int action = decide2_logits(x0, x1, dn, tn, decide2_slope(margin), &e, decided);
    decide2_operands(x0, x1, e, action, a_best, d);
    return action;
}

}  // namespace rlhip

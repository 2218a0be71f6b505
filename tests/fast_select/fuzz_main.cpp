// Fuzz of categorical_decide2 (csrc/select_decide.h) against the exact two-action Gumbel-max rule of categorical_select1
// (csrc/select_device.h), restated here with the host libm evaluated in Float64 and rounded once, as the oracle does.
//   fuzz_main <random draws> <near-tie draws> [threads]
// prints one line of counts: key=value pairs (tests/test_fast_select_rule.py asserts on them).
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <thread>
#include <vector>

#include "select_decide.h"

namespace {

struct Rng {  // splitmix64
    uint64_t s;
    uint64_t next() {
        uint64_t z = (s += 0x9E3779B97F4A7C15ull);
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
        return z ^ (z >> 31);
    }
    double u01() { return ((double)(next() >> 11) + 0.5) * 0x1p-53; }  // (0, 1)
    double gumbel() { return -std::log(-std::log(u01())); }
    void normal2(double* a, double* b) {
        const double r = std::sqrt(-2.0 * std::log(u01())), t = 6.283185307179586 * u01();
        *a = r * std::cos(t);
        *b = r * std::sin(t);
    }
};

struct Exact {
    int action;
    float lp[2];
};

// categorical_select1, na = 2, no mask: the same operations in the same order
Exact exact_rule(float x0, float x1, double nz0, double nz1) {
    float mx = -INFINITY;
    if (x0 > mx) mx = x0;
    if (x1 > mx) mx = x1;
    const float other = (x1 > x0) ? x0 : x1;
    const float se = 1.0f + (float)std::exp((double)(other - mx));
    const float lse = (float)std::log((double)se);
    Exact e;
    e.lp[0] = (x0 - mx) - lse;
    e.lp[1] = (x1 - mx) - lse;
    const double g0 = nz0 + (double)e.lp[0], g1 = nz1 + (double)e.lp[1];
    e.action = (g1 > g0) ? 1 : 0;
    return e;
}

struct Counts {
    uint64_t draws = 0, decided = 0, wrong = 0, undecided = 0;
    void add(const Counts& o) {
        draws += o.draws;
        decided += o.decided;
        wrong += o.wrong;
        undecided += o.undecided;
    }
};

inline void check(float x0, float x1, double nz0, double nz1, Counts& c) {
    float ab, d;
    bool decided;
    const int action = rlhip::categorical_decide2(x0, x1, nz0, nz1, 1.0, &ab, &d, &decided);
    ++c.draws;
    if (!decided) {
        ++c.undecided;
        return;
    }
    ++c.decided;
    // the action is the exact rule's; a_best and d are, bit for bit, the operands the exact rule forms
    const Exact e = exact_rule(x0, x1, nz0, nz1);
    float s[3], f[2] = {ab, d};
    rlhip::select2_operands(x0, x1, &s[0], &s[1], &s[2]);
    const float g[2] = {s[action], s[2]};
    if (action != e.action || std::memcmp(f, g, sizeof f) != 0) ++c.wrong;
}

const float SCALES[3] = {0.05f, 1.0f, 10.0f};

void random_draws(uint64_t n, uint64_t seed, Counts& c) {
    Rng g{seed};
    for (uint64_t i = 0; i < n; ++i) {
        double a, b;
        g.normal2(&a, &b);
        const float sc = SCALES[i % 3];
        check(sc * (float)a, sc * (float)b, g.gumbel(), g.gumbel(), c);
    }
}

// the second noise placed within +-2^-20 (|d| + 2) of the exact rule's tie
void near_tie_draws(uint64_t n, uint64_t seed, Counts& c) {
    Rng g{seed};
    for (uint64_t i = 0; i < n; ++i) {
        double a, b;
        g.normal2(&a, &b);
        const float sc = SCALES[i % 3];
        const float x0 = sc * (float)a, x1 = sc * (float)b;
        const double nz0 = g.gumbel();
        const Exact e = exact_rule(x0, x1, nz0, 0.0);
        const double d = std::fabs((double)x0 - (double)x1);
        const double nz1 = nz0 + ((double)e.lp[0] - (double)e.lp[1]) + (2.0 * g.u01() - 1.0) * 0x1p-20 * (d + 2.0);
        check(x0, x1, nz0, nz1, c);
    }
}

// finite corner cases of the logits, random and near-tie noise: x0 == x1, d subnormal, d tiny, d large
void corner_draws(uint64_t n, uint64_t seed, Counts& c) {
    Rng g{seed};
    const float pairs[][2] = {{0.0f, 0.0f},     {1.5f, 1.5f},        {-0.0f, 0.0f},      {1e-40f, 0.0f},   {0.0f, 3e-45f},
                              {-1e-39f, 1e-41f}, {1.0f, 1.0000001f}, {-80.0f, 30.0f},    {100.0f, -100.0f}, {3e38f, -3e38f},
                              {1e-38f, -1e-38f}, {0.25f, 0.2500001f}};
    for (const auto& p : pairs)
        for (uint64_t i = 0; i < n; ++i) {
            const double nz0 = g.gumbel();
            check(p[0], p[1], nz0, g.gumbel(), c);
            const Exact e = exact_rule(p[0], p[1], nz0, 0.0);
            const double d = std::fabs((double)p[0] - (double)p[1]);
            check(p[0], p[1], nz0, nz0 + ((double)e.lp[0] - (double)e.lp[1]) + (2.0 * g.u01() - 1.0) * 0x1p-20 * (d + 2.0), c);
            check(p[0], p[1], nz0, nz0 + ((double)e.lp[0] - (double)e.lp[1]), c);  // the tie itself
        }
}

// every case here must be left to the exact path
void nonfinite_cases(Counts& c) {
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    const double dinf = std::numeric_limits<double>::infinity(), dnan = std::numeric_limits<double>::quiet_NaN();
    const float xs[] = {0.0f, 1.0f, -3.5f, 1e-40f, 3e38f};
    const double ns[] = {0.0, 0.3, -2.0, 30.0, 1e300};
    Rng g{99};
    for (float x : xs)
        for (double nza : ns)
            for (double nzb : ns) {
                const float lx[][2] = {{nan, x}, {x, nan}, {nan, nan}, {-inf, x}, {x, -inf}, {inf, x}, {x, inf}, {inf, inf}, {-inf, -inf},
                                       {inf, -inf}};
                for (const auto& l : lx) check(l[0], l[1], nza, nzb, c);
                const double nn[][2] = {{dinf, nzb}, {nza, dinf}, {-dinf, nzb}, {nza, -dinf}, {dinf, dinf}, {-dinf, -dinf}, {dinf, -dinf},
                                        {dnan, nzb}, {nza, dnan}, {dnan, dnan}, {1.7e308, -1.7e308}};
                for (const auto& q : nn) check(x, xs[g.next() % 5], q[0], q[1], c);
            }
}

}  // namespace

int main(int argc, char** argv) {
    const uint64_t n_random = argc > 1 ? std::strtoull(argv[1], nullptr, 10) : 100000000ull;
    const uint64_t n_tie = argc > 2 ? std::strtoull(argv[2], nullptr, 10) : 10000000ull;
    unsigned nt = argc > 3 ? (unsigned)std::atoi(argv[3]) : std::thread::hardware_concurrency();
    if (nt < 1) nt = 1;
    if (nt > 16) nt = 16;
    std::vector<Counts> cr(nt), ct(nt);
    std::vector<std::thread> th;
    for (unsigned k = 0; k < nt; ++k)
        th.emplace_back([&, k] {
            const uint64_t r0 = n_random / nt + (k < n_random % nt ? 1 : 0), t0 = n_tie / nt + (k < n_tie % nt ? 1 : 0);
            random_draws(r0, 0x1234 + 7919ull * k, cr[k]);
            near_tie_draws(t0, 0xABCD + 104729ull * k, ct[k]);
        });
    Counts corner, nonfin;
    corner_draws(20000, 5, corner);
    nonfinite_cases(nonfin);
    for (auto& t : th) t.join();
    Counts r, t;
    for (unsigned k = 0; k < nt; ++k) {
        r.add(cr[k]);
        t.add(ct[k]);
    }
    // margin = +inf: nothing is decided
    float ab, d;
    bool m_decided, m_decided0;
    rlhip::categorical_decide2(0.5f, -0.5f, 3.0, -1.0, std::numeric_limits<double>::infinity(), &ab, &d, &m_decided);
    rlhip::categorical_decide2(0.5f, 0.5f, 3.0, -1.0, std::numeric_limits<double>::infinity(), &ab, &d, &m_decided0);
    m_decided = m_decided || m_decided0;
    std::printf("random_draws=%llu random_undecided=%llu random_wrong=%llu tie_draws=%llu tie_decided=%llu tie_wrong=%llu "
                "corner_draws=%llu corner_decided=%llu corner_wrong=%llu nonfinite_cases=%llu nonfinite_decided=%llu inf_margin_decided=%d\n",
                (unsigned long long)r.draws, (unsigned long long)r.undecided, (unsigned long long)r.wrong,
                (unsigned long long)t.draws, (unsigned long long)t.decided, (unsigned long long)t.wrong,
                (unsigned long long)corner.draws, (unsigned long long)corner.decided, (unsigned long long)corner.wrong,
                (unsigned long long)nonfin.draws, (unsigned long long)nonfin.decided, (int)m_decided);
    return 0;
}

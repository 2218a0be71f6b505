// Stand-alone host check of csrc/record_slot32.h (tests/test_record_slot32.py compiles it with -fsanitize=address,undefined and
// runs it): for every net the fused two-layer PPO learner supports -- h in 8, 16, .., 256; ns in {2, 3, 4}; nout in {1, 2, 3} --
//   1. record_slot32 equals the 64-bit formula of ppo_grad_tile.h `record_slot` (restated below, operator for operator) for
//      every flat parameter q < np;
//   2. the slots of the net's np parameters are a permutation of the image positions pack_records writes a parameter to
//      (restated below from its loop: per unit record the ns W1 pairs, the bias pair, the head weights; then the bias tail).
// Prints one line and exits 0, or the first mismatch and exits 1.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "record_slot32.h"

namespace {

constexpr int REC = 16;

int64_t record_slot64(int64_t q, int h, int ns, int nout, int64_t np_a) {
    const int net = q >= np_a ? 1 : 0;
    const int64_t r = q - (net ? np_a : 0);
    const int no = net ? 1 : nout;
    if (r < (int64_t)h * ns) return REC * (r % h) + 2 * (r / h) + net;
    if (r < (int64_t)h * ns + h) return REC * (r - (int64_t)h * ns) + 8 + net;
    const int64_t w = r - ((int64_t)h * ns + h);
    if (w < (int64_t)no * h) {
        if (net) return REC * w + 11;
        const int64_t j = w / no, o = w % no;
        return REC * j + (o == 0 ? 10 : 11 + o);
    }
    return (int64_t)REC * h + (net ? 3 : (w - (int64_t)no * h));
}

// image position -> the flat parameter index pack_records copies there (-1: a zero pad)
std::vector<int64_t> pack_sources(int h, int ns, int nout, int64_t np_a) {
    std::vector<int64_t> src((size_t)REC * h + 4, -1);
    const int64_t W1a = 0, b1a = W1a + (int64_t)h * ns, W2a = b1a + h, b2a = W2a + (int64_t)nout * h;
    const int64_t W1c = np_a, b1c = W1c + (int64_t)h * ns, W2c = b1c + h, b2c = W2c + h;
    for (int j = 0; j < h; ++j) {
        int64_t* rec = &src[(size_t)REC * j];
        for (int k = 0; k < 4; ++k)
            if (k < ns) {
                rec[2 * k] = W1a + j + (int64_t)h * k;
                rec[2 * k + 1] = W1c + j + (int64_t)h * k;
            }
        rec[8] = b1a + j;
        rec[9] = b1c + j;
        rec[10] = W2a + 0 + (int64_t)nout * j;
        rec[11] = W2c + j;
        if (nout > 1) rec[12] = W2a + 1 + (int64_t)nout * j;
        if (nout > 2) rec[13] = W2a + 2 + (int64_t)nout * j;
    }
    int64_t* t = &src[(size_t)REC * h];
    for (int o = 0; o < 3; ++o)
        if (o < nout) t[o] = b2a + o;
    t[3] = b2c;
    return src;
}

}  // namespace

int main() {
    long nets = 0, params = 0;
    for (int h = 8; h <= 256; h += 8)
        for (int ns = 2; ns <= 4; ++ns)
            for (int nout = 1; nout <= 3; ++nout) {
                const int64_t np_a = (int64_t)h * ns + h + (int64_t)nout * h + nout;
                const int64_t np = np_a + (int64_t)h * ns + h + h + 1;
                const std::vector<int64_t> src = pack_sources(h, ns, nout, np_a);
                std::vector<int> hits(src.size(), 0);
                for (int64_t q = 0; q < np; ++q) {
                    const int64_t want = record_slot64(q, h, ns, nout, np_a);
                    const uint32_t got = rlhip::record_slot32((uint32_t)q, (uint32_t)h, (uint32_t)ns, (uint32_t)nout, (uint32_t)np_a);
                    if ((int64_t)got != want) {
                        std::printf("h %d ns %d nout %d q %lld: 32-bit slot %u, 64-bit slot %lld\n", h, ns, nout, (long long)q, got,
                                    (long long)want);
                        return 1;
                    }
                    if (got >= src.size() || src[got] != q) {
                        std::printf("h %d ns %d nout %d q %lld: slot %u holds parameter %lld in pack_records' image\n", h, ns, nout,
                                    (long long)q, got, got < src.size() ? (long long)src[got] : -2ll);
                        return 1;
                    }
                    ++hits[got];
                }
                for (size_t s = 0; s < src.size(); ++s)
                    if (hits[s] != (src[s] >= 0 ? 1 : 0)) {
                        std::printf("h %d ns %d nout %d: image position %zu is written %d times (%s)\n", h, ns, nout, s, hits[s],
                                    src[s] >= 0 ? "a parameter" : "a pad");
                        return 1;
                    }
                ++nets;
                params += (long)np;
            }
    std::printf("record_slot32 ok: %ld nets, %ld parameters\n", nets, params);
    return 0;
}

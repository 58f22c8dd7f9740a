// mrnnt_sample.h -- what the path sampler's two implementations (mrnnt_sample.hip, mrnnt_cpu.cpp) must do identically:
// the counter-based random numbers and the decision rule of one step (mrnnt_sample in include/mrnnt.h). Included by
// host and device code; integer code and plain fp64 only.
#pragma once

#include <math.h>
#include <stdint.h>

#ifdef __HIPCC__
#define MRNNT_HD __host__ __device__ __forceinline__
#else
#define MRNNT_HD inline
#endif

namespace mrnnt {

constexpr uint32_t kSampleTag = 0x4D524E54u;  // "MRNT": the fourth counter word of every sampler block

// Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11): counter c[4], key (k0, k1);
// the output overwrites c.
MRNNT_HD void philox4x32_10(uint32_t c[4], uint32_t k0, uint32_t k1) {
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c[0];
        const uint64_t p1 = (uint64_t)0xCD9E8D57u * c[2];
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c[1] ^ k0;
        const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c[3] ^ k1;
        c[1] = (uint32_t)p1;
        c[3] = (uint32_t)p0;
        c[0] = n0;
        c[2] = n2;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
}

// The four words of frames 4q .. 4q + 3 of sample `sample` of utterance b: frame t uses word t & 3 of block t >> 2.
MRNNT_HD void sample_block(uint64_t seed, uint32_t q, uint32_t sample, uint32_t b, uint32_t w[4]) {
    w[0] = q;
    w[1] = sample;
    w[2] = b;
    w[3] = kSampleTag;
    philox4x32_10(w, (uint32_t)seed, (uint32_t)(seed >> 32));
}

// u in the open interval (0, 1): (word + 0.5) * 2^-32, exact in fp64
MRNNT_HD double sample_uniform(uint32_t word) { return ((double)word + 0.5) * (1.0 / 4294967296.0); }

// Probability of the label arc out of a row: x = lpb + beta(t+1, s) (the blank arc; -inf when it would leave the
// band), y = lpe + beta(t+1, s+1) (the label arc; -inf at s = S). Normalised over the two arcs, so the pair sums to
// exactly 1. A NaN result emits blank (u < NaN is false).
MRNNT_HD double sample_p_label(double x, double y) {
    const double ninf = -HUGE_VAL;
    if (y == ninf) return 0.0;
    if (x == ninf) return 1.0;
    return 1.0 / (1.0 + exp(x - y));
}

}  // namespace mrnnt

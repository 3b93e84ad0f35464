// kanpyo_amd/csrc/kgpu_prob_core.h -- the rule of the lattice probabilities (include/kanpyo_gpu.h, "lattice probabilities"), written once for the host
// (kgpu_prob_host.cpp) and for the device (kgpu_prob.hip): the same statements decide both.  Plain C++ without a HIP include.
//   kexp, klog     exp on [-32, 0] and log on the positive normals from IEEE-754 double + - x, explicit fma, comparisons and integer operations: no libm
//                  function, no division, no contraction the source does not spell (the pragma below) -- host and device round every step alike
//   fix            a term of a sum as an unsigned 40-bit fixed-point integer: the sums are integer sums, which no order changes
//   the weight     of an edge, the uniform of a (seed, sentence, sample, target, predecessor) and its Gumbel, the marginal of a node
#pragma once
#include <cstdint>
#include <cstring>

#include "kgpu_nbest_core.h"   // nbest_record: the record of a node

// No a * b + c below may become one fma unless it is written as one: the device would fuse (v_fmac_f64) what the host keeps apart.  The pragma holds for the
// rest of the file that includes this header: the kernels of kgpu_prob.hip and the loops of kgpu_prob_host.cpp stand under it too.
#pragma clang fp contract(off)

namespace kgpu {

static_assert(KGPU_THETA_MAX == 18446744073709551616.0, "the header's cap is the one the weights are sized for");

constexpr double PROB_THETA_MAX = 18446744073709551616.0;   // 2^64 (KGPU_THETA_MAX): an edge is at most 2^17 in size and a path has fewer than 2^24 of them, so every weight and every log-sum stays finite
constexpr uint64_t PROB_MAX_NODES = 1ull << 24;   // a sum of N terms of at most 2^40 stays below 2^64

KGPU_NORM_HD double prob_from_bits(uint64_t b) { double d; memcpy(&d, &b, 8); return d; }
KGPU_NORM_HD uint64_t prob_bits(double d) { uint64_t b; memcpy(&b, &d, 8); return b; }
KGPU_NORM_HD double prob_neg_inf() { return prob_from_bits(0xFFF0000000000000ull); }
KGPU_NORM_HD bool prob_finite(double x) { return x > prob_neg_inf(); }   // (of a log-sum: -inf or finite; false for a NaN)

// u64 -> double in one rounding: the high word times 2^32 is exact, the addition rounds.
KGPU_NORM_HD double prob_u64_to_double(uint64_t v) { return (double)(uint32_t)(v >> 32) * 4294967296.0 + (double)(uint32_t)v; }

// exp(x) for x <= 0: exactly 0 below -32 (and for a NaN), exactly 1 at 0, absolute error <= 2^-46 (measured: tests/test_prob_cpu.py).
// x = k ln 2 + r with |r| <= 0.35 (+ a rounding of k), the Taylor polynomial of degree 13 in r (its remainder is below 1e-17), times 2^k built from its bits.
KGPU_NORM_HD double kexp(double x) {
    if (!(x >= -32.0)) return 0.0;
    if (x > 0.0) x = 0.0;
    const int32_t k = (int32_t)(x * 0x1.71547652b82fep+0 - 0.5);   // about the nearest integer to x / ln 2: -47 .. 0
    const double kd = (double)k;
    double r = __builtin_fma(-kd, 0x1.62e42fee00000p-1, x);        // exact: ln2_hi has 32 bits
    r = __builtin_fma(-kd, 0x1.a39ef35793c76p-33, r);
    double p = 0x1.6124613a86d09p-33;                              // 1 / 13!
    p = __builtin_fma(p, r, 0x1.1eed8eff8d898p-29);
    p = __builtin_fma(p, r, 0x1.ae64567f544e4p-26);
    p = __builtin_fma(p, r, 0x1.27e4fb7789f5cp-22);
    p = __builtin_fma(p, r, 0x1.71de3a556c734p-19);
    p = __builtin_fma(p, r, 0x1.a01a01a01a01ap-16);
    p = __builtin_fma(p, r, 0x1.a01a01a01a01ap-13);
    p = __builtin_fma(p, r, 0x1.6c16c16c16c17p-10);
    p = __builtin_fma(p, r, 0x1.1111111111111p-7);
    p = __builtin_fma(p, r, 0x1.5555555555555p-5);
    p = __builtin_fma(p, r, 0x1.5555555555555p-3);
    p = __builtin_fma(p, r, 0.5);
    p = __builtin_fma(p, r, 1.0);
    p = __builtin_fma(p, r, 1.0);
    return p * prob_from_bits((uint64_t)(1023 + k) << 52);         // exact: a power of two, no subnormal
}

// log(x) for a positive normal x: error <= 2^-46 max(1, |log x|) (measured: tests/test_prob_cpu.py).
// x = 2^e m with m in [1, 2); the top five mantissa bits pick c ~ 1 / m (12 bits, so m c - 1 is one exact fma) and -log c from two tables;
// log m = -log c + log1p(m c - 1), |m c - 1| <= 1/32, the series to degree 11.  From m = 1.5 on the entry is that of m / 2 and e is one more, and the
// two bins next to 1 have c = 1 and c = 1/2 with -log c = 0: near 1 the result is the series of the exact x - 1, relative accuracy.
KGPU_NORM_HD double klog(double x) {
    constexpr double RC[32] = {
        0x1.0000000000000p+0, 0x1.e920000000000p-1, 0x1.dae0000000000p-1, 0x1.cd80000000000p-1, 0x1.c0e0000000000p-1, 0x1.b4e0000000000p-1, 0x1.a980000000000p-1, 0x1.9ec0000000000p-1,
        0x1.9480000000000p-1, 0x1.8ac0000000000p-1, 0x1.8180000000000p-1, 0x1.78a0000000000p-1, 0x1.7020000000000p-1, 0x1.6820000000000p-1, 0x1.6060000000000p-1, 0x1.58e0000000000p-1,
        0x1.51e0000000000p-1, 0x1.4b00000000000p-1, 0x1.4460000000000p-1, 0x1.3e20000000000p-1, 0x1.3820000000000p-1, 0x1.3240000000000p-1, 0x1.2ca0000000000p-1, 0x1.2740000000000p-1,
        0x1.2200000000000p-1, 0x1.1d00000000000p-1, 0x1.1820000000000p-1, 0x1.1360000000000p-1, 0x1.0ec0000000000p-1, 0x1.0a60000000000p-1, 0x1.0620000000000p-1, 0x1.0000000000000p-1};
    constexpr double NL[32] = {
        0x0.0p+0, 0x1.766d923c20ff8p-5, 0x1.345179b63dd42p-4, 0x1.a956d3ecade63p-4, 0x1.0d79e7cd48e5ap-3, 0x1.44f8b726f8efbp-3, 0x1.7b0091651528cp-3, 0x1.af6895610dbaep-3,
        0x1.e2a877a6b2c12p-3, 0x1.0a504e97bb40cp-2, 0x1.22981fbef797bp-2, 0x1.3a71c56bb48c6p-2, 0x1.51d1d9310456cp-2, 0x1.68518244cfb0ep-2, 0x1.7e9883fa49fecp-2, 0x1.94a042803643ap-2,
        -0x1.1c2895218f2c0p-2, -0x1.071b85fcd590dp-2, -0x1.e4ceeda61dda6p-3, -0x1.bcf6736f7d6c7p-3, -0x1.95f7ac2b3b4f5p-3, -0x1.6f0d28ae56b4cp-3, -0x1.4915d832fb562p-3, -0x1.2423113ba50e3p-3,
        -0x1.fec9131dbeabbp-4, -0x1.b78c82bb0eda1p-4, -0x1.70e12b325c82ap-4, -0x1.2ad449eff2316p-4, -0x1.cae72fb95c20bp-5, -0x1.4572e981cad90p-5, -0x1.83624fba83bd7p-6, 0x0.0p+0};
    const uint64_t b = prob_bits(x);
    const uint32_t i = (uint32_t)(b >> 47) & 31u;
    const double ed = (double)((int32_t)((b >> 52) & 0x7FFu) - 1023 + (int32_t)(i >> 4));
    const double m = prob_from_bits((b & 0x000FFFFFFFFFFFFFull) | 0x3FF0000000000000ull);
    const double r = __builtin_fma(m, RC[i], -1.0);
    double q = 0x1.745d1745d1746p-4;                               // 1 / 11
    q = __builtin_fma(q, r, -0x1.999999999999ap-4);
    q = __builtin_fma(q, r, 0x1.c71c71c71c71cp-4);
    q = __builtin_fma(q, r, -0x1.0000000000000p-3);
    q = __builtin_fma(q, r, 0x1.2492492492492p-3);
    q = __builtin_fma(q, r, -0x1.5555555555555p-3);
    q = __builtin_fma(q, r, 0x1.999999999999ap-3);
    q = __builtin_fma(q, r, -0x1.0000000000000p-2);
    q = __builtin_fma(q, r, 0x1.5555555555555p-2);
    q = __builtin_fma(q, r, -0.5);
    const double p = __builtin_fma(r * r, q, r);                   // log1p(r)
    const double t = __builtin_fma(ed, 0x1.a39ef35793c76p-33, p);
    return (t + NL[i]) + ed * 0x1.62e42fee00000p-1;                // (e ln2_hi is exact)
}

// x in [0, 1] -> x 2^40 rounded to the nearest integer (ties to even): adding 2^52 does the rounding.
KGPU_NORM_HD uint64_t prob_fix(double x) { return prob_bits(x * 1099511627776.0 + 4503599627370496.0) & 0x000FFFFFFFFFFFFFull; }
// m + log(S 2^-40): the log-sum of terms whose maximum is m and whose fixed-point sum around m is S >= 2^40
KGPU_NORM_HD double prob_logsum(double m, uint64_t S) { return m + klog(prob_u64_to_double(S) * 0x1p-40); }

// w(j, t) = -theta (M[j.right_id][t.left_id] + t.cost): the integer sum is exact, then one multiplication
KGPU_NORM_HD double prob_weight(double theta, int32_t conn_cost, int32_t word_cost) { return -theta * (double)(conn_cost + word_cost); }

// a_j = alpha[j] + w(j, t): a term of the forward sum (and beta[t] + w(j, t): of the backward one)
KGPU_NORM_HD double prob_term(double ab, double theta, int32_t conn_cost, int32_t word_cost) { return ab + prob_weight(theta, conn_cost, word_cost); }

// A node's marginal: exp(min(0, alpha + beta - log_z)), the additions in that order.
KGPU_NORM_HD double prob_marginal(double alpha, double beta, double log_z) {
    const double d = (alpha + beta) - log_z;
    return kexp(d < 0.0 ? d : 0.0);
}

// splitmix64's output function over a counter word
KGPU_NORM_HD uint64_t prob_mix(uint64_t z) {
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
// The hash of (seed, sentence, sample, target): one mix per word; prob_gumbel adds the predecessor.
KGPU_NORM_HD uint64_t prob_hash_target(uint64_t seed, uint64_t sentence, uint64_t sample, uint64_t target) {
    return prob_mix(prob_mix(prob_mix(prob_mix(seed) ^ sentence) ^ sample) ^ target);
}
// u = (2 h + 1) 2^-53 with h the hash's top 52 bits: an odd 53-bit numerator, exactly a double, strictly inside (0, 1); -log u is in [1.1e-16, 36.8],
// a positive normal (klog is relative-accurate next to 1).  G = -log(-log u).
KGPU_NORM_HD double prob_gumbel(uint64_t target_hash, uint64_t pred) {
    const uint64_t h = prob_mix(target_hash ^ pred) >> 12;
    const double u = prob_u64_to_double(2 * h + 1) * 0x1p-53;
    return -klog(-klog(u));
}

// int64 -> int32, saturating: a sampled path's cost
KGPU_NORM_HD int32_t prob_sat32(int64_t v) { return v > 2147483647ll ? 2147483647 : v < -2147483648ll ? (int32_t)-2147483648ll : (int32_t)v; }

}  // namespace kgpu

// gpcc_rng.h -- the random numbers of gpcc_sample_batch for BOTH sides of the boundary: the host picks the rows of
// mixture draws before any device work, the device generates the standard normals of every draw inside gpcc_sample_tiles.
//   generator  Philox4x64-10 (Salmon et al., SC'11; Random123's multipliers and Weyl constants), key (seed, 0); integer operations
//              only, so host and device produce the same bits
//   normal     element j of draw s of row m: counter (j / 4, s, m, 0) -- m = 2^64 - 1 for draws of the mixture, whose noise then does
//              not depend on the row they picked --, Box-Muller over the word pairs (0, 1) and (2, 3):
//              z = sqrt(-2 log u1) (cos, sin)(2 pi u2), u1 = ((x0 >> 11) + 1) 2^-53 in (0, 1], u2 = (x1 >> 11) 2^-53 in [0, 1)
//   row choice draw s of the mixture: u = (x0 >> 11) 2^-53 of counter (s, 0, 2^64 - 1, 1); the first m with u c_{M-1} < c_m and
//              w_m > 0, c_m = sum_{k <= m} w_k summed in row order
//   points     the linear-time draws: block e of draw s of row m from counter (e, s, m, 2), normal4_stream
// gpcc_amd/rng.py is the numpy mirror (tests/test_sample_cpu.py checks this header against it, and it against numpy's Philox).
#pragma once
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define GPCC_RNG_HD __host__ __device__
#else
#define GPCC_RNG_HD
#endif

namespace gpccrng {

struct u64x4 { uint64_t v[4]; };

GPCC_RNG_HD inline uint64_t mulhi64(uint64_t a, uint64_t b)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __umul64hi(a, b);
#else
    return (uint64_t)(((unsigned __int128)a * b) >> 64);
#endif
}

// Philox4x64-10 of counter (c0, c1, c2, c3) under key (k0, k1)
GPCC_RNG_HD inline u64x4 philox4x64(uint64_t c0, uint64_t c1, uint64_t c2, uint64_t c3, uint64_t k0, uint64_t k1)
{
    const uint64_t M0 = 0xD2E7470EE14C6C93ULL, M1 = 0xCA5A826395121157ULL;
    const uint64_t W0 = 0x9E3779B97F4A7C15ULL, W1 = 0xBB67AE8584CAA73BULL;
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        if (r > 0) { k0 += W0; k1 += W1; }
        const uint64_t hi0 = mulhi64(M0, c0), lo0 = M0 * c0;
        const uint64_t hi1 = mulhi64(M1, c2), lo1 = M1 * c2;
        const uint64_t n0 = hi1 ^ c1 ^ k0, n2 = hi0 ^ c3 ^ k1;
        c0 = n0; c1 = lo1; c2 = n2; c3 = lo0;
    }
    u64x4 o;
    o.v[0] = c0; o.v[1] = c1; o.v[2] = c2; o.v[3] = c3;
    return o;
}

GPCC_RNG_HD inline double uniform53(uint64_t x) { return (double)(x >> 11) * 0x1.0p-53; }        // [0, 1)
GPCC_RNG_HD inline double uniform53_open0(uint64_t x) { return (double)((x >> 11) + 1) * 0x1.0p-53; }   // (0, 1]

// the four normals of test indices 4 blk .. 4 blk + 3 of draw s of row m (m = ~0: a mixture draw)
GPCC_RNG_HD inline void normal4(uint64_t seed, uint64_t blk, uint64_t s, uint64_t m, double z[4])
{
#pragma clang fp contract(off)
    const double TWO_PI = 6.283185307179586476925286766559;
    const u64x4 x = philox4x64(blk, s, m, 0, seed, 0);
#pragma unroll
    for (int p = 0; p < 2; ++p) {
        const double u1 = uniform53_open0(x.v[2 * p]), u2 = uniform53(x.v[2 * p + 1]);
        const double r = sqrt(-2.0 * log(u1)), th = TWO_PI * u2;
        z[2 * p] = r * cos(th);
        z[2 * p + 1] = r * sin(th);
    }
}

// the same four normals from counter (blk, s, m, stream): stream 0 is normal4's, 1 the row picks', 2 the point blocks of the linear-time
// draws (gpcc_sample_markov_batch, DESIGN.md 4.19: blk indexes a point -- training points in gpcc_create's order, then the test points
// in the caller's order, then one block for the offsets)
GPCC_RNG_HD inline void normal4_stream(uint64_t seed, uint64_t blk, uint64_t s, uint64_t m, uint64_t stream, double z[4])
{
#pragma clang fp contract(off)
    const double TWO_PI = 6.283185307179586476925286766559;
    const u64x4 x = philox4x64(blk, s, m, stream, seed, 0);
#pragma unroll
    for (int p = 0; p < 2; ++p) {
        const double u1 = uniform53_open0(x.v[2 * p]), u2 = uniform53(x.v[2 * p + 1]);
        const double r = sqrt(-2.0 * log(u1)), th = TWO_PI * u2;
        z[2 * p] = r * cos(th);
        z[2 * p + 1] = r * sin(th);
    }
}

// the uniform that picks the row of mixture draw s
GPCC_RNG_HD inline double pick_uniform(uint64_t seed, uint64_t s)
{
    return uniform53(philox4x64(s, 0, ~0ULL, 1, seed, 0).v[0]);
}

// the row of mixture draw s: c = the cumulative weights (c[m] = c[m-1] + w[m] in row order, c[M-1] > 0), w = the weights.  c is
// non-decreasing, so the first m with x < c[m] is found by bisection; it has w[m] > 0 (c[m] > c[m-1]) -- the loop after it only
// guards that statement.
GPCC_RNG_HD inline int pick_row(uint64_t seed, uint64_t s, const double *c, const double *w, int M)
{
#pragma clang fp contract(off)
    const double x = pick_uniform(seed, s) * c[M - 1];
    int lo = 0, hi = M - 1;   // answer in [lo, hi]: c[M-1] > x since u < 1
    while (lo < hi) {
        const int mid = lo + (hi - lo) / 2;
        if (x < c[mid]) hi = mid;
        else lo = mid + 1;
    }
    while (lo < M - 1 && !(w[lo] > 0.0)) ++lo;
    return lo;
}

}  // namespace gpccrng

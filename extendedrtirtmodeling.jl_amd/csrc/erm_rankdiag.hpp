// erm_rankdiag.hpp -- the integer and ordering parts of the rank-normalised convergence diagnostics (Vehtari, Gelman, Simpson, Carpenter and
// Buerkner 2021), as PURE functions usable from host and device.  Every decision the diagnostics take before the normal quantile is called is an ordering of
// the draws or an integer, and all of them are here:
//     rk_key        the order-preserving 64-bit key of a double: a < b  <=>  rk_key(a) < rk_key(b) for all non-NaN a, b, -inf and +inf included, and
//                   rk_key(-0.0) == rk_key(+0.0) (the two zeros compare equal, so they must tie in a ranking)
//     rk_avg_rank   the average rank (1-based) shared by the tie run that occupies the sorted positions first .. last (0-based): the mean of first + 1 .. last + 1
//     rk_prob       rank -> probability: (r - 3/8) / (S + 1/4) (Blom 1958), one fp64 subtraction, one addition and one division
//     rk_tail_k     the order statistic of the 5 % tail: ceil(S / 20) in integers
// The same header is compiled by g++ with -fsanitize=undefined into tests/rankdiag_check (tests/test_rankdiag_host.py).  No HIP, no allocation, no environment.
#pragma once
#include <cstdint>
#include <cstring>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define ERM_RK_FN __host__ __device__ inline
#else
#define ERM_RK_FN inline
#endif

namespace erm {

// the largest number of used draws S = 2 * n_chain * floor((n_iter - n_burnin) / 2) of a column the rank kernel takes: its sort buffer (16 + 2 bytes per padded
// draw) and the transformed series (8 bytes per draw) are resident in the 160 KB of LDS of one gfx950 workgroup
constexpr int RK_MAX_DRAWS = 8192;

ERM_RK_FN uint64_t rk_key(double x)
{
    uint64_t b;
    memcpy(&b, &x, sizeof(b));
    const uint64_t sign = 0x8000000000000000ull;
    if (b == sign) b = 0;                          // -0.0 ties with +0.0
    return (b & sign) ? ~b : (b | sign);           // negative: all bits flipped (larger magnitude = smaller key); non-negative: above every negative
}
ERM_RK_FN double rk_avg_rank(long long first, long long last) { return 0.5 * (double)(first + last) + 1.0; }      // exact: first + last < 2^53
ERM_RK_FN double rk_prob(double r, long long S) { return (r - 0.375) / ((double)S + 0.25); }
ERM_RK_FN long long rk_tail_k(long long S) { return (S + 19) / 20; }
// the padded length of the sorting network: the smallest power of two >= S
ERM_RK_FN int rk_pad(int S) { int P = 1; while (P < S) P <<= 1; return P; }

}  // namespace erm

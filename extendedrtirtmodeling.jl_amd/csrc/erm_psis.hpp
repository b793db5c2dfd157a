// erm_psis.hpp -- the scalar parts of Pareto-smoothed importance sampling behind the marginal PSIS-LOO (include/ertirt.h: erm_get_marginal_loo;
// Vehtari, Gelman and Gabry 2017; Vehtari, Simpson, Gelman, Yao and Gabry 2024; the fit: Zhang and Stephens 2009), as PURE functions usable from host and device:
//     psis_tail_len    M = min(ceil(S / 5), ceil(3 sqrt(S))) in integers (ceil(3 sqrt(S)) = the smallest m with m^2 >= 9 S; the arms cross at S = 225)
//     psis_grid        G = 30 + floor(sqrt(M)), in integers
//     psis_xstar       the index of x* = x[floor(M / 4 + 0.5)] (1-based), in integers
//     psis_b, psis_mean_log1p, psis_profile   one point of the fit's grid: b_j, k_j = mean_i log1p(-b_j x_i) (i = 1..M IN ORDER), L_j = M (log(-b_j / k_j) - k_j - 1)
//     psis_finish      the grid's L_j, b_j -> b^ = sum_j b_j exp(L_j - LSE(L)) (j IN ORDER), k_raw, sigma, k^ = (M k_raw + 5) / (M + 10), and the unfittable rule
//     psis_fit         the whole fit of M ascending exceedances, composed of the above (what psis_kernel does with one lane per grid point)
//     psis_quantile    sigma expm1(-k log1p(-p)) / k with its k = 0 limit -sigma log1p(-p)
//     psis_smooth      the smoothed tail value number i (1-based): min(0, log(exp(c) + quantile((i - 1/2) / M)))
//     psis_unkey       the inverse of rk_key (erm_rankdiag.hpp)
// The same header is compiled by g++ with -fsanitize=undefined into tests/psis_check (tests/test_psis_host.py).  No HIP, no allocation, no environment.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define ERM_PS_FN __host__ __device__ inline
#else
#define ERM_PS_FN inline
#endif

namespace erm {

// the rows a unit may have: the lower limit gives M >= 5, the upper one is the LDS sort's (RK_MAX_DRAWS of erm_rankdiag.hpp)
constexpr int PSIS_MIN_ROWS = 25, PSIS_MAX_ROWS = 8192;
constexpr int PSIS_MAX_TAIL = 272, PSIS_MAX_GRID = 46;      // M and G at S = 8192
constexpr double PSIS_K_BAD = 0.7;                          // k^ above this: the estimate is unreliable whatever S (Vehtari et al. 2024)
enum { PSIS_ELPD = 0, PSIS_P = 1, PSIS_KHAT = 2, PSIS_NEFF = 3, PSIS_COLS = 4 };

// the smallest m with m * m >= v (v >= 0)
ERM_PS_FN long long psis_ceil_sqrt(long long v)
{
    long long m = (long long)sqrt((double)v);
    while (m * m < v) ++m;
    while (m > 0 && (m - 1) * (m - 1) >= v) --m;
    return m;
}
// the largest m with m * m <= v
ERM_PS_FN long long psis_floor_sqrt(long long v)
{
    long long m = (long long)sqrt((double)v);
    while (m * m > v) --m;
    while ((m + 1) * (m + 1) <= v) ++m;
    return m;
}
ERM_PS_FN int psis_tail_len(long long S)
{
    const long long a = (S + 4) / 5, b = psis_ceil_sqrt(9 * S);
    return (int)(a < b ? a : b);
}
ERM_PS_FN int psis_grid(int M) { return 30 + (int)psis_floor_sqrt(M); }
// 0-based index of x* = x[floor(M / 4 + 0.5)] (1-based): floor((M + 2) / 4) - 1
ERM_PS_FN int psis_xstar(int M) { return (M + 2) / 4 - 1; }
// the sample-size dependent threshold of k^: min(1 - 1 / log10(S), 0.7)
ERM_PS_FN double psis_k_threshold(long long S) { const double t = 1.0 - 1.0 / log10((double)S); return t < PSIS_K_BAD ? t : PSIS_K_BAD; }

ERM_PS_FN double psis_unkey(uint64_t k)
{
    const uint64_t sign = 0x8000000000000000ull;
    const uint64_t b = (k & sign) ? (k & ~sign) : ~k;
    double x;
    memcpy(&x, &b, sizeof(x));
    return x;
}

// grid point j = 1..G
ERM_PS_FN double psis_b(int j, int G, double xM, double xstar) { return 1.0 / xM + (1.0 - sqrt((double)G / ((double)j - 0.5))) / (3.0 * xstar); }
ERM_PS_FN double psis_mean_log1p(double b, const double* x, int M)
{
    double s = 0.0;
    for (int i = 0; i < M; ++i) s += log1p(-b * x[i]);
    return s / (double)M;
}
ERM_PS_FN double psis_profile(double b, double k, int M) { return (double)M * (log(-b / k) - k - 1.0); }

struct PsisFit { double khat, sigma; bool ok; };      // ok = false: the tail cannot be fitted, k^ = +Inf and the weights stay as they are

ERM_PS_FN bool psis_fittable(const double* x, int M) { return x[psis_xstar(M)] > 0.0 && x[M - 1] - x[0] > 0.0; }
ERM_PS_FN PsisFit psis_finish(const double* L, const double* b, int G, const double* x, int M)
{
    const PsisFit bad{(double)INFINITY, 0.0, false};
    if (!psis_fittable(x, M)) return bad;
    double mx = L[0];
    for (int j = 1; j < G; ++j) if (!(L[j] <= mx)) mx = L[j];      // (a NaN is taken up and spoils the sum: unfittable)
    double se = 0.0;
    for (int j = 0; j < G; ++j) se += exp(L[j] - mx);
    const double lse = mx + log(se);
    double bh = 0.0;
    for (int j = 0; j < G; ++j) bh += b[j] * exp(L[j] - lse);
    const double kr = psis_mean_log1p(bh, x, M);
    const double sigma = -kr / bh;
    const double khat = ((double)M * kr + 5.0) / ((double)M + 10.0);
    if (!(std::isfinite(bh) && std::isfinite(sigma) && std::isfinite(khat))) return bad;
    return PsisFit{khat, sigma, true};
}
// x: the M exceedances, ascending; L, b: G doubles of scratch each
ERM_PS_FN PsisFit psis_fit(const double* x, int M, double* L, double* b)
{
    const int G = psis_grid(M);
    if (psis_fittable(x, M)) {
        const double xs = x[psis_xstar(M)], xM = x[M - 1];
        for (int j = 1; j <= G; ++j) { b[j - 1] = psis_b(j, G, xM, xs); L[j - 1] = psis_profile(b[j - 1], psis_mean_log1p(b[j - 1], x, M), M); }
    }
    return psis_finish(L, b, G, x, M);
}

ERM_PS_FN double psis_quantile(double p, double k, double sigma)
{
    const double t = log1p(-p);
    return k == 0.0 ? -sigma * t : sigma * expm1(-k * t) / k;
}
// i = 1..M
ERM_PS_FN double psis_smooth(int i, int M, double expc, double k, double sigma)
{
    const double v = log(expc + psis_quantile(((double)i - 0.5) / (double)M, k, sigma));
    return v < 0.0 ? v : (v == v ? 0.0 : v);
}

}  // namespace erm

// erm_pointwise.hpp -- streaming accumulators of the pointwise log-likelihood behind WAIC, as PURE functions usable from host and device.
//
// For one unit u (a subject or a cell) the engine sees l_u^(s), the unit's log-likelihood at post-burn-in trace row s, once per sweep and never again.
// Four doubles per unit carry everything WAIC needs:
//     m     running maximum of l
//     s     sum_s exp(l^(s) - m), rescaled by exp(m_old - m_new) whenever the maximum grows (never overflows: every term is <= 1)
//     mean  Welford mean of l
//     m2    Welford sum of squared deviations
// Rows are applied in trace order, so the accumulators of a chain are bit-reproducible and do not depend on how its sweeps are split into erm_run calls.
//     lppd_u = m + log(s / n)           p_u = m2 / (n - 1)
// The same header is compiled by g++ with -fsanitize=undefined into tests/pointwise_check (tests/test_pointwise_accumulators.py): streaming against
// two-pass evaluation in long double.  No HIP, no allocation, no environment.
#pragma once
#include <cmath>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define ERM_PW_FN __host__ __device__ inline
#else
#define ERM_PW_FN inline
#endif

namespace erm {

enum { PW_OFF = 0, PW_SUBJECT = 1, PW_CELL = 2 };
constexpr double PW_VAR_WARN = 0.4;       // p_u above this: the usual warning threshold (Vehtari, Gelman and Gabry 2017)

struct PwAcc { double m, s, mean, m2; };  // all zero = no row applied yet

// applies row number k (1-based count of the rows applied to this unit, this one included)
ERM_PW_FN void pw_update(PwAcc& a, double l, long long k)
{
    if (k <= 1) { a.m = l; a.s = 1.0; a.mean = l; a.m2 = 0.0; return; }
    if (l > a.m) { a.s = a.s * exp(a.m - l) + 1.0; a.m = l; }
    else a.s += exp(l - a.m);
    const double d = l - a.mean;
    a.mean += d / (double)k;
    a.m2 += d * (l - a.mean);
}
// log of the mean over the n rows applied of exp(l)
ERM_PW_FN double pw_lppd(const PwAcc& a, long long n) { return a.m + log(a.s / (double)n); }
// sample variance of l over the n >= 2 rows applied
ERM_PW_FN double pw_var(const PwAcc& a, long long n) { return a.m2 / (double)(n - 1); }

}  // namespace erm

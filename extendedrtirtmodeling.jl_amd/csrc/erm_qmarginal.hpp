// erm_qmarginal.hpp -- the response-time term of the marginal log-likelihood of GibbsRtIrtLatentQr with the quantile weight nu_i and the speed zeta_i integrated
// out (include/ertirt.h: erm_get_quantile_marginal_waic), as PURE functions usable from host and device.  Everything else of the rule -- the law of
// theta, B(theta), the nodes, (M, S) -- is erm_marginal.hpp's, unchanged.
//
// The model has zeta | theta, nu ~ N(m + k1 nu, s k2 nu), m = m0 + m1 theta, s = Sigma_p[2,2], and its nu draw is the conditional under nu ~ Exponential(mean s).
// Integrating nu out leaves the asymmetric Laplace law
//     log p(zeta | theta) = log(q (1 - q) / s) - u (q - [u < 0]),  u = (zeta - m) / s                                  (q = q_rt; MargLaw::v carries s)
// and the response times stay Gaussian in zeta: with g_j = 1 / sig2t_j, d0_j = lambda_j - t_j and MargSums' P, R0, D0, L (rho = 0),
//     bU = R0 - q / s,  bL = R0 + (1 - q) / s
//     up = bU^2 / (2 P) + q m / s       + logPhi(-(m - bU / P) sqrt(P))                                                (the part zeta >= m)
//     lo = bL^2 / (2 P) - (1 - q) m / s + logPhi( (m - bL / P) sqrt(P))                                                (the part zeta <  m)
//     T(theta) = -(J / 2) log 2 pi - L / 2 - D0 / 2 + log(q (1 - q) / s) + 1/2 log(2 pi / P) + logaddexp(up, lo)
// T needs s > 0, P > 0 and 0 < q < 1; the callers refuse anything else before a kernel runs.
//
// logPhi (qmarg_log_ndtr) has three arms, the same on host and device -- erfc, log, log1p and nothing a host compiler lacks:
//     x >= 0          log1p(-erfc(x / sqrt 2) / 2)
//     -36 <= x < 0    log(erfc(-x / sqrt 2) / 2)                      erfc is a normal number down to x = -37.5
//     x < -36         -x^2 / 2 - log(-x) - 1/2 log 2 pi + log1p(-r + 3 r^2 - 15 r^3 + ... + 2027025 r^8),  r = 1 / x^2,  by Horner's rule from the last term
// The asymptotic series' first omitted term is 34459425 r^9 < 4e-21 at x = -36.
// The same header is compiled by g++ with -fsanitize=undefined into tests/qmarginal_check (tests/test_qmarginal_host.py): logPhi against erfcl in long double,
// T against a brute-force zeta grid in long double split at m.  No HIP, no allocation, no environment.
#pragma once
#include "erm_marginal.hpp"

namespace erm {

// the one model served: LatentQr.  (CrossQr: with nu_ij integrated out every cell's time is asymmetric Laplace in zeta -- J kinks that move with theta.)
constexpr bool qmarg_served(int model) { return model == LATENTQR; }
constexpr bool qmarg_level_ok(double q) { return q > 0.0 && q < 1.0; }

constexpr double QMARG_SERIES_X = -36.0;          // below it: the asymptotic series
constexpr double QMARG_SQRT1_2 = 0.70710678118654752440;

ERM_MG_FN double qmarg_log_ndtr(double x)
{
    if (x >= 0.0) return log1p(-0.5 * erfc(x * QMARG_SQRT1_2));
    if (x >= QMARG_SERIES_X) return log(0.5 * erfc(-x * QMARG_SQRT1_2));
    const double r = 1.0 / (x * x);
    double p = 2027025.0;
    p = -135135.0 + r * p; p = 10395.0 + r * p; p = -945.0 + r * p; p = 105.0 + r * p; p = -15.0 + r * p; p = 3.0 + r * p; p = -1.0 + r * p;
    return -0.5 * x * x - log(-x) - 0.5 * MARG_LOG_2PI + log1p(r * p);
}
// log(e^a + e^b)
ERM_MG_FN double qmarg_logaddexp(double a, double b) { return fmax(a, b) + log1p(exp(-fabs(a - b))); }

// T(theta) above: w.v is the scale s, the sums are marg_item_sums' with rho = 0
ERM_MG_FN double qmarg_T(const MargSums& ms, int J, const MargLaw& w, double theta, double q)
{
    const double s = w.v, m = w.m0 + w.m1 * theta, P = ms.P, rP = sqrt(P);
    const double bU = ms.R0 - q / s, bL = ms.R0 + (1.0 - q) / s;
    const double up = bU * bU / (2.0 * P) + q * m / s + qmarg_log_ndtr(-(m - bU / P) * rP);
    const double lo = bL * bL / (2.0 * P) - (1.0 - q) * m / s + qmarg_log_ndtr((m - bL / P) * rP);
    return -0.5 * (double)J * MARG_LOG_2PI - 0.5 * ms.L - 0.5 * ms.D0 + log(q * (1.0 - q) / s) + 0.5 * (MARG_LOG_2PI - log(P)) + qmarg_logaddexp(up, lo);
}

}  // namespace erm

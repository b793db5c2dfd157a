// erm_marginal.hpp -- the marginal pointwise log-likelihood behind the marginal WAIC (include/ertirt.h: erm_get_marginal_waic), as PURE functions
// usable from host and device.
//
// For subject i at parameter row s the person parameters are integrated out: zeta_i analytically, theta_i by a fixed rule of Q equally spaced nodes.
//     population law   theta ~ N(mu, sd^2),  zeta | theta ~ N(m0 + m1 theta, v)                                  (MargLaw, from the row's structural part)
//     responses        B(theta) = sum_j [ y_j eta_j - log(1 + e^eta_j) ],  eta_j = a_j (theta - b_j)             (the caller's loop: the kernel, the CPU check)
//     response times   T(theta) = log N(t; lambda - rho theta - m 1, diag(sig2t) + v 1 1'),  m = m0 + m1 theta   (marg_T, from six sums over the items)
//     rule             z_q = -6 + q h, h = 12 / (Q - 1), theta_q = mu + sd z_q, e_q = log h - 1/2 log 2 pi - 1/2 z_q^2 + B(theta_q) + T(theta_q)
//     l = log sum_q exp(e_q) = M + log S,  M = max_q e_q,  S = sum_q exp(e_q - M)                               (MargMS: streaming, and a merge of two partial sums)
// T has no 1 / v: a Sigma_p of correlation +-1 (v = 0) is an ordinary case.  S < 2 says that one node carries more than half the mass: the rule is too coarse
// for that subject's posterior (MARG_COARSE_S).
// The same header is compiled by g++ with -fsanitize=undefined into tests/marginal_check (tests/test_marginal_host.py): T against a brute-force zeta grid in long
// double, the merge against a one-pass log-sum.  No HIP, no allocation, no environment.
#pragma once
#include <cmath>
#include "erm_model.hpp"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define ERM_MG_FN __host__ __device__ inline
#else
#define ERM_MG_FN inline
#endif

namespace erm {

constexpr int MARG_NODES_DEFAULT = 61, MARG_NODES_MIN = 3, MARG_NODES_MAX = 1025;
constexpr double MARG_Z_MAX = 6.0;        // the rule covers mu +- 6 sd of the population law
constexpr double MARG_COARSE_S = 2.0;
constexpr double MARG_LOG_2PI = 1.8378770664093454836;

constexpr bool marg_nodes_ok(int Q) { return Q >= MARG_NODES_MIN && Q <= MARG_NODES_MAX && (Q & 1) == 1; }
// the models whose zeta integral is Gaussian (the quantile models' is not: nu has to be integrated out with it -- LatentQr: erm_qmarginal.hpp)
constexpr bool marg_served(int model) { return model == MLIRT || model == RTIRT || model == NULLM || model == CROSS || model == LATENT; }

struct MargLaw { double mu, sd, m0, m1, v; };
// [1 x] beta over F covariate columns, added in order
ERM_MG_FN double marg_xb(const double* beta, int F, const double* x)
{
    double t = beta[0];
    for (int f = 0; f < F; ++f) t += x[f] * beta[1 + f];
    return t;
}
// The law from the structural part of an item-trace row: xb0 / xb1 = [1 x] times beta's first / second column (MlIrt, Latent: the one column, without the theta
// slot; models that see no covariates: 0), bth = Latent's coefficient of theta, S = vec(Sigma_p).  v is returned as computed: a caller that must go on clamps it at 0.
ERM_MG_FN MargLaw marg_law(int model, double xb0, double xb1, double bth, const double* S)
{
    if (model == MLIRT) return {xb0, 1.0, 0.0, 0.0, 0.0};
    const double s11 = S[0], s12 = 0.5 * (S[1] + S[2]), s22 = S[3];
    if (model == LATENT || model == LATENTQR) return {0.0, sqrt(s11), xb0, bth, s22};      // (LatentQr: v is the scale of zeta's asymmetric Laplace law)
    const double m1 = s12 / s11;
    return {model == RTIRT ? xb0 : 0.0, sqrt(s11), model == RTIRT ? xb1 - m1 * xb0 : 0.0, m1, s22 - s12 * s12 / s11};
}
// the same from a row's small part of qr (q = row + 4 J, tiny_publish's order) and the subject's covariates over the Fk columns the kernels see
ERM_MG_FN MargLaw marg_law_row(int model, const double* q, int J, int Fk, const double* x)
{
    const ModelTraits t = model_traits(model);
    double xb0 = 0.0, xb1 = 0.0, bth = 0.0;
    if (t.beta == BETA_VEC || t.beta == BETA_LATENT || t.beta == BETA_PAIR) xb0 = marg_xb(q, Fk, x);
    if (t.beta == BETA_PAIR) xb1 = marg_xb(q + Fk + 1, Fk, x);
    if (t.beta == BETA_LATENT) bth = q[Fk + 1];
    return marg_law(model, xb0, xb1, bth, q + qr_sigp_off(model, J, Fk));
}

// log(1 + e^x) without a branch: every lane of a wave takes the same path whatever the sign of its eta.  The values are those of the two-armed form the
// log-likelihood kernels use (x > 0 ? x + log1p(exp(-x)) : log1p(exp(x))) bit for bit: 0 + y = y.
ERM_MG_FN double marg_log1pexp(double x) { return fmax(x, 0.0) + log1p(exp(-fabs(x))); }

// The six sums over a subject's items at one row, with g_j = 1 / sig2t_j and d0_j = lambda_j - t_j:
//   P = sum g, R0 = sum g d0, R1 = sum g rho, D0 = sum g d0^2, D1 = sum g d0 rho, D2 = sum g rho^2, L = sum log sig2t
struct MargSums { double P, R0, R1, D0, D1, D2, L; };
ERM_MG_FN void marg_sums_add(MargSums& s, double g, double logsig, double d0, double rho)
{
    s.P += g; s.R0 += g * d0; s.R1 += g * rho; s.D0 += g * d0 * d0; s.D1 += g * d0 * rho; s.D2 += g * rho * rho; s.L += logsig;
}
ERM_MG_FN double marg_T(const MargSums& s, int J, const MargLaw& w, double theta)
{
    const double R = s.R0 - theta * s.R1, D = s.D0 - 2.0 * theta * s.D1 + theta * theta * s.D2, m = w.m0 + w.m1 * theta, vP = w.v * s.P;
    return -0.5 * (double)J * MARG_LOG_2PI - 0.5 * s.L - 0.5 * log1p(vP) - 0.5 * (D + (s.P * m * m - 2.0 * R * m - w.v * R * R) / (1.0 + vP));
}

// the rule
ERM_MG_FN double marg_step(int Q) { return 2.0 * MARG_Z_MAX / (double)(Q - 1); }
ERM_MG_FN double marg_node(int q, double h) { return -MARG_Z_MAX + (double)q * h; }
ERM_MG_FN double marg_log_weight(double z, double log_h) { return log_h - 0.5 * MARG_LOG_2PI - 0.5 * z * z; }

// log sum exp, streaming: S = sum exp(e - M) with M the largest term so far.  S = 0 is the empty sum (M is then not read).
struct MargMS { double M, S; };
ERM_MG_FN void marg_ms_add(MargMS& a, double e)
{
    if (!(a.S > 0.0)) { a.M = e; a.S = 1.0; return; }
    if (e > a.M) { a.S = a.S * exp(a.M - e) + 1.0; a.M = e; }
    else a.S += exp(e - a.M);
}
// two partial sums; symmetric in its arguments bit for bit (a + b = b + a), so both partners of a butterfly step hold the same pair afterwards
ERM_MG_FN MargMS marg_ms_merge(const MargMS& a, const MargMS& b)
{
    if (!(b.S > 0.0)) return a;
    if (!(a.S > 0.0)) return b;
    if (a.M >= b.M) return {a.M, a.S + b.S * exp(b.M - a.M)};
    return {b.M, b.S + a.S * exp(a.M - b.M)};
}
ERM_MG_FN double marg_ms_log(const MargMS& a) { return a.M + log(a.S); }

}  // namespace erm

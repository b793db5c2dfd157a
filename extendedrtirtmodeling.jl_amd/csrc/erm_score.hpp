// erm_score.hpp -- the scores of respondents (include/ertirt.h: erm_get_scores): posterior mean and sd of theta_i and zeta_i from the item trace, as
// PURE functions usable from host and device, beside erm_marginal.hpp whose law, item sums and node rule they use.
//
// At row s the posterior of theta_i lies on the rule's nodes with weights w_q = exp(e_q - M) / S; zeta_i given theta_i and the response times is Gaussian:
//     theta at the row   Z1 = sum w_q z_q, Z2 = sum w_q z_q^2;  E = mu + sd Z1,  V = sd^2 (Z2 - Z1^2), clamped at 0      (ScoreMS: M, S and the two sums S1 = S Z1,
//                        S2 = S Z2, streamed and merged under the running maximum exactly as MargMS is -- M and S are MargMS's bit for bit)
//     zeta at the row    zeta | theta, t ~ N(c0 + c1 theta, u),  u = v / (1 + v P),  c0 = (m0 + v R0) / (1 + v P),  c1 = (m1 - v R1) / (1 + v P)      (score_zeta)
//                        hence Ez = c0 + c1 E,  Vz = u + c1^2 V,  C = c1 V.  No 1 / v: v = 0 is an ordinary case.
//     across the rows    weight omega_s = 1 (SCORE_EQUAL) or exp(l_s - Lambda), l_s = M + log S, Lambda the running maximum (SCORE_LIKELIHOOD): West's weighted
//                        Welford on the pair (E, Ez) with its co-moment, the weighted means of V, Vz and C, sum omega and sum omega^2 -- eleven doubles (ScoreAcc).
//     the law of total variance   theta = mean E,  theta_sd^2 = mean V + M2_E / W,  cov = mean C + C_EEz / W,  zeta likewise,  row_ess = W^2 / sum omega^2.
// The same header is compiled by g++ with -fsanitize=undefined into tests/score_check (tests/test_score_host.py).  No HIP, no allocation, no environment.
#pragma once
#include "erm_marginal.hpp"

namespace erm {

constexpr int SCORE_EQUAL = 0, SCORE_LIKELIHOOD = 1;
constexpr int SCORE_THETA = 0, SCORE_THETA_SD = 1, SCORE_ZETA = 2, SCORE_ZETA_SD = 3, SCORE_COV = 4, SCORE_ROW_ESS = 5, SCORE_COARSE = 6, SCORE_COLS = 7;
constexpr bool score_weighting_ok(int w) { return w == SCORE_EQUAL || w == SCORE_LIKELIHOOD; }

// zeta | theta, t ~ N(c0 + c1 theta, u): every d_j = lambda_j - t_j - rho_j theta is an observation of zeta with variance sig2t_j, the prior is N(m0 + m1 theta, v)
struct ScoreZeta { double c0, c1, u; };
ERM_MG_FN ScoreZeta score_zeta(const MargSums& s, const MargLaw& w)
{
    const double d = 1.0 + w.v * s.P;
    return {(w.m0 + w.v * s.R0) / d, (w.m1 - w.v * s.R1) / d, w.v / d};
}

// S = sum exp(e - M), S1 = sum exp(e - M) z, S2 = sum exp(e - M) z^2 with M the largest term so far.  S = 0 is the empty sum.
struct ScoreMS { double M, S, S1, S2; };
ERM_MG_FN void score_ms_add(ScoreMS& a, double e, double z)
{
    if (!(a.S > 0.0)) { a.M = e; a.S = 1.0; a.S1 = z; a.S2 = z * z; return; }
    if (e > a.M) { const double f = exp(a.M - e); a.S = a.S * f + 1.0; a.S1 = a.S1 * f + z; a.S2 = a.S2 * f + z * z; a.M = e; }
    else { const double f = exp(e - a.M); a.S += f; a.S1 += f * z; a.S2 += f * (z * z); }
}
// two partial sums; symmetric in its arguments bit for bit, as marg_ms_merge is
ERM_MG_FN ScoreMS score_ms_merge(const ScoreMS& a, const ScoreMS& b)
{
    if (!(b.S > 0.0)) return a;
    if (!(a.S > 0.0)) return b;
    if (a.M >= b.M) { const double f = exp(b.M - a.M); return {a.M, a.S + b.S * f, a.S1 + b.S1 * f, a.S2 + b.S2 * f}; }
    const double f = exp(a.M - b.M);
    return {b.M, b.S + a.S * f, b.S1 + a.S1 * f, b.S2 + a.S2 * f};
}

// the moments of (theta, zeta) at one row, and l = M + log S
struct ScoreRow { double E, V, Ez, Vz, C, l; };
ERM_MG_FN ScoreRow score_row(const ScoreMS& p, const MargLaw& w, const ScoreZeta& k)
{
    const double Z1 = p.S1 / p.S, Z2 = p.S2 / p.S;
    const double E = w.mu + w.sd * Z1, V = fmax(w.sd * w.sd * (Z2 - Z1 * Z1), 0.0);
    return {E, V, k.c0 + k.c1 * E, k.u + k.c1 * k.c1 * V, k.c1 * V, p.M + log(p.S)};
}

// The rows, in trace order.  W = sum omega, W2 = sum omega^2 (both relative to exp(Lam)), the weighted means of E, Ez, V, Vz, C and the weighted central
// second moments of (E, Ez).  W = 0 is the empty accumulator (Lam is then not read).
struct ScoreAcc { double W, W2, Lam, mE, mZ, M2E, M2Z, CEZ, mV, mVz, mC; };
ERM_MG_FN void score_acc_add(ScoreAcc& a, const ScoreRow& r, bool weighted)
{
    double om = 1.0;
    if (weighted) {
        if (!(a.W > 0.0)) a.Lam = r.l;
        else if (r.l > a.Lam) {      // the maximum rises: what is held becomes relative to the new one
            const double f = exp(a.Lam - r.l);
            a.W *= f; a.W2 *= f * f; a.M2E *= f; a.M2Z *= f; a.CEZ *= f; a.Lam = r.l;
        }
        else om = exp(r.l - a.Lam);
    }
    a.W += om; a.W2 += om * om;
    const double g = om / a.W, dE = r.E - a.mE, dZ = r.Ez - a.mZ;
    a.mE += g * dE; a.mZ += g * dZ;
    a.M2E += om * dE * (r.E - a.mE); a.M2Z += om * dZ * (r.Ez - a.mZ); a.CEZ += om * dE * (r.Ez - a.mZ);
    a.mV += g * (r.V - a.mV); a.mVz += g * (r.Vz - a.mVz); a.mC += g * (r.C - a.mC);
}
// out[SCORE_THETA .. SCORE_ROW_ESS]; a model without zeta (has_zeta = false) gets NaN in its zeta columns and its covariance
ERM_MG_FN void score_finish(const ScoreAcc& a, bool has_zeta, double* out)
{
    const double nan = NAN;
    out[SCORE_THETA] = a.mE;
    out[SCORE_THETA_SD] = sqrt(fmax(a.mV + a.M2E / a.W, 0.0));
    out[SCORE_ZETA] = has_zeta ? a.mZ : nan;
    out[SCORE_ZETA_SD] = has_zeta ? sqrt(fmax(a.mVz + a.M2Z / a.W, 0.0)) : nan;
    out[SCORE_COV] = has_zeta ? a.mC + a.CEZ / a.W : nan;
    out[SCORE_ROW_ESS] = a.W * a.W / a.W2;
}

}  // namespace erm

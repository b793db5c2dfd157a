// erm_fit.hpp -- person fit from the item trace (include/ertirt.h: erm_get_person_fit): whether a respondent's responses and response times are
// probable under the model for that person, as PURE functions usable from host and device, beside erm_score.hpp whose law, item sums and node rule they use.
//
// At row s the posterior of theta_i lies on the rule's nodes with weights w_q = exp(e_q - M) / S.  At node theta_q, over the observed items:
//     responses        eta_j = a_j (theta_q - b_j), t_j = e^-|eta_j|, r_j = t_j / (1 + t_j) if (y_j = 1) <=> (eta_j >= 0), else 1 / (1 + t_j)      (fit_cell)
//                      W = sum (2 y_j - 1) r_j eta_j = l0 - E[l0 | theta],  Vw = sum eta_j^2 t_j / (1 + t_j)^2 = Var[l0 | theta],  l0 = sum y eta - log(1 + e^eta)
//                      lz = W / sqrt(Vw), 0 when Vw = 0 (Drasgow, Levine and Williams 1985; negative: misfit).  No difference of large sums anywhere.
//     response times   Qf = D + (P m^2 - 2 R m - v R^2) / (1 + v P), clamped at 0: -2 (marg_T - its constants), the Mahalanobis form of the log-times given theta
//                      with zeta integrated out, exactly chi^2_n (fit_rt_quad).  tail = P(chi^2_n >= Qf), the finite sum for integer n (fit_chi2_tail);
//                      ltz = Wilson-Hilferty's z of Qf (fit_wh; descriptive, positive: misfit -- not used for the tail).
//     at the row       LZ = sum w_q lz, PY = sum w_q Phi(lz), LTZ = sum w_q ltz, PT = sum w_q tail: six running sums S, S LZ, S PY, S LTZ, S PT and M that stream
//                      and merge under the running maximum exactly as ScoreMS does (FitMS) -- M and S are MargMS's bit for bit.
//     across the rows  weight omega_s = 1 (SCORE_EQUAL) or exp(l_s - Lambda) with score_acc_add's rescale (SCORE_LIKELIHOOD): the weighted running means of the
//                      four row values, sum omega and sum omega^2 (FitAcc).  row_ess = (sum omega)^2 / sum omega^2.
// PY and PT are posterior predictive p-values with a realised discrepancy (Gelman, Meng and Stern 1996); small means misfit for both.
// The same header is compiled by g++ with -fsanitize=undefined into tests/fit_check (tests/test_fit_host.py).  No HIP, no allocation, no environment.
#pragma once
#include "erm_score.hpp"

namespace erm {

constexpr int FIT_LZ = 0, FIT_P_RESP = 1, FIT_LTZ = 2, FIT_P_TIME = 3, FIT_ROW_ESS = 4, FIT_COARSE = 5, FIT_COLS = 6;
constexpr double FIT_SQRT_HALF = 0.70710678118654752440, FIT_TWO_OVER_SQRT_PI = 1.12837916709551257390;
constexpr double FIT_TAIL_Y_MAX = 700.0;      // past it e^-y leaves the normal range and the tail is below 1e-300 for every n <= 896: 0

// one cell at one node, from ONE exp: log(1 + e^eta) with marg_log1pexp's bits into lse, the cell's terms into W and Vw
ERM_MG_FN void fit_cell(double eta, bool y, double& lse, double& W, double& Vw)
{
    const double t = exp(-fabs(eta)), inv = 1.0 / (1.0 + t), small = t * inv;      // small <= 1/2 <= inv: the two probabilities of the cell
    lse += fmax(eta, 0.0) + log1p(t);
    const double r = (y == (eta >= 0.0)) ? small : inv;
    W += (y ? r : -r) * eta;
    Vw += eta * eta * (small * inv);
}
ERM_MG_FN double fit_lz(double W, double Vw) { return Vw > 0.0 ? W / sqrt(Vw) : 0.0; }
ERM_MG_FN double fit_phi(double x) { return 0.5 * erfc(-x * FIT_SQRT_HALF); }

// the quadratic form of the log-times at theta, zeta integrated out: -2 (marg_T - its constants), clamped at 0
ERM_MG_FN double fit_rt_quad(const MargSums& s, const MargLaw& w, double theta)
{
    const double R = s.R0 - theta * s.R1, D = s.D0 - 2.0 * theta * s.D1 + theta * theta * s.D2, m = w.m0 + w.m1 * theta, vP = w.v * s.P;
    return fmax(D + (s.P * m * m - 2.0 * R * m - w.v * R * R) / (1.0 + vP), 0.0);
}
// P(chi^2_n >= Qf[c]) for C values at once: with y = Qf / 2, o = n mod 2, m = n / 2:  base = o ? erfc(sqrt y) : 0,  t_0 = e^-y (o ? 2 sqrt(y / pi) : 1),
// t_k = t_(k-1) y / (k + o / 2),  tail = base + sum_(k < m) t_k;  0 for y > 700.  Every term is at most 1.  One reciprocal per k serves the C values.
// In two steps, so that a kernel can take its C chains through the special functions one after the other and through the terms together:
// fit_tail_start gives y, t_0 and returns base; fit_tail_sum adds the m terms to tail (= base on entry) for C values at once.
ERM_MG_FN double fit_tail_start(double Qf, int n, double& y, double& t0)
{
    const bool o = (n & 1) != 0;
    y = 0.5 * Qf;
    const double rt = sqrt(y);
    t0 = exp(-y) * (o ? FIT_TWO_OVER_SQRT_PI * rt : 1.0);
    return o ? erfc(rt) : 0.0;
}
template <int C>
ERM_MG_FN void fit_tail_sum(const double (&y)[C], double (&t)[C], int n, double (&tail)[C])
{
    const int o = n & 1, m = n >> 1;
    for (int k = 0; k < m; ++k) {
        const double rc = 1.0 / ((double)(k + 1) + 0.5 * (double)o);
        for (int c = 0; c < C; ++c) { tail[c] += t[c]; t[c] *= y[c] * rc; }
    }
    for (int c = 0; c < C; ++c) if (y[c] > FIT_TAIL_Y_MAX) tail[c] = 0.0;
}
template <int C>
ERM_MG_FN void fit_chi2_tails(const double (&Qf)[C], int n, double (&tail)[C])
{
    double y[C], t[C];
    for (int c = 0; c < C; ++c) tail[c] = fit_tail_start(Qf[c], n, y[c], t[c]);
    fit_tail_sum<C>(y, t, n, tail);
}
ERM_MG_FN double fit_chi2_tail(double Qf, int n)
{
    const double q[1] = {Qf};
    double t[1];
    fit_chi2_tails<1>(q, n, t);
    return t[0];
}
// Wilson-Hilferty: ((Qf / n)^(1/3) - (1 - 2 / (9 n))) / sqrt(2 / (9 n)); n = 0 has no statistic (fit_finish reports NaN): 0
ERM_MG_FN double fit_wh(double Qf, int n)
{
    if (n <= 0) return 0.0;
    const double c = 2.0 / (9.0 * (double)n);
    return (cbrt(Qf / (double)n) - (1.0 - c)) / sqrt(c);
}

// S = sum exp(e - M) and the four sums of exp(e - M) times (lz, Phi(lz), ltz, tail), M the largest term so far.  S = 0 is the empty sum.
struct FitMS { double M, S, LZ, PY, LTZ, PT; };
ERM_MG_FN void fit_ms_add(FitMS& a, double e, double lz, double py, double ltz, double pt)
{
    if (!(a.S > 0.0)) { a.M = e; a.S = 1.0; a.LZ = lz; a.PY = py; a.LTZ = ltz; a.PT = pt; return; }
    if (e > a.M) {
        const double f = exp(a.M - e);
        a.S = a.S * f + 1.0; a.LZ = a.LZ * f + lz; a.PY = a.PY * f + py; a.LTZ = a.LTZ * f + ltz; a.PT = a.PT * f + pt; a.M = e;
    }
    else { const double f = exp(e - a.M); a.S += f; a.LZ += f * lz; a.PY += f * py; a.LTZ += f * ltz; a.PT += f * pt; }
}
// two partial sums; symmetric in its arguments bit for bit, as score_ms_merge is
ERM_MG_FN FitMS fit_ms_merge(const FitMS& a, const FitMS& b)
{
    if (!(b.S > 0.0)) return a;
    if (!(a.S > 0.0)) return b;
    if (a.M >= b.M) { const double f = exp(b.M - a.M); return {a.M, a.S + b.S * f, a.LZ + b.LZ * f, a.PY + b.PY * f, a.LTZ + b.LTZ * f, a.PT + b.PT * f}; }
    const double f = exp(a.M - b.M);
    return {b.M, b.S + a.S * f, b.LZ + a.LZ * f, b.PY + a.PY * f, b.LTZ + a.LTZ * f, b.PT + a.PT * f};
}

// the four weighted means at one row, and l = M + log S
struct FitRow { double v[4]; double l; };
ERM_MG_FN FitRow fit_row(const FitMS& p) { return {{p.LZ / p.S, p.PY / p.S, p.LTZ / p.S, p.PT / p.S}, p.M + log(p.S)}; }

// The rows, in trace order.  W = sum omega, W2 = sum omega^2 (both relative to exp(Lam)) and the weighted running means of the four row values.
// W = 0 is the empty accumulator (Lam is then not read).
struct FitAcc { double W, W2, Lam, m[4]; };
ERM_MG_FN void fit_acc_add(FitAcc& a, const FitRow& r, bool weighted)
{
    double om = 1.0;
    if (weighted) {
        if (!(a.W > 0.0)) a.Lam = r.l;
        else if (r.l > a.Lam) { const double f = exp(a.Lam - r.l); a.W *= f; a.W2 *= f * f; a.Lam = r.l; }      // the maximum rises, as in score_acc_add
        else om = exp(r.l - a.Lam);
    }
    a.W += om; a.W2 += om * om;
    const double g = om / a.W;
    for (int c = 0; c < 4; ++c) a.m[c] += g * (r.v[c] - a.m[c]);
}
// out[FIT_LZ .. FIT_ROW_ESS]; a model without response times (has_rt = false) gets NaN in LTZ and P_TIME, a subject without an observed cell (n = 0) in all four
ERM_MG_FN void fit_finish(const FitAcc& a, bool has_rt, int n, double* out)
{
    const double nan = NAN;
    out[FIT_LZ] = n > 0 ? a.m[0] : nan;
    out[FIT_P_RESP] = n > 0 ? a.m[1] : nan;
    out[FIT_LTZ] = has_rt && n > 0 ? a.m[2] : nan;
    out[FIT_P_TIME] = has_rt && n > 0 ? a.m[3] : nan;
    out[FIT_ROW_ESS] = a.W * a.W / a.W2;
}

}  // namespace erm

// qmarginal_check.cpp -- LatentQr's marginal response-time term (extendedrtirtmodeling.jl_amd/csrc/erm_qmarginal.hpp) on the CPU, built with
// UndefinedBehaviorSanitizer by tests/test_qmarginal_host.py.  The header the kernel includes against independent arithmetic:
//   - qmarg_log_ndtr against logl(0.5L * erfcl(-x / sqrtl(2))) in long double on the grid x = -140, -140 + 1/64, ..., 9 and at the joins of its three arms
//     (x = -36 and its two neighbours, +-0, +-1e-300).  The reference's own error is measured at every x against the same value in __float128
//     (x < 0: logq(erfcq / 2); x >= 0: log1pq(-erfcq / 2), since the long-double form loses its digits as Phi approaches 1);
//   - qmarg_T(theta) against a brute-force zeta integral in long double of the product of the J normal densities and zeta's asymmetric Laplace law, split at its
//     kink zeta = m: 20-point Gauss-Legendre on 400 panels per side (the closed form is used to PLACE the panels only), for J in {1, 7, 65}, q in {0.15, 0.5, 0.85},
//     s in {0.05, 0.2, 1, 6}, random rows, subjects and covariates, five nodes of the rule.  The reference's own error is measured by halving the panels.
// Bound at every point: the larger of 1e-11 and ten times the reference's own error there, relative.
// Prints the largest errors and "failures N".  `qmarginal_check L q Q J F row.. y.. t.. x..` prints one l = M + log S of the rule from the header's host build
// (for the extremes of tests/test_qmarginal_host.py and tests/test_gpu_quantile_marginal.py).
#include <quadmath.h>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>
#include "erm_qmarginal.hpp"

using namespace erm;
typedef long double ld;
typedef __float128 qd;

static int failures = 0;
static void check(bool ok, const char* what, double at, double got, double want)
{
    if (!ok) { ++failures; printf("FAIL %s at %.17g: got %.17g want %.17g\n", what, at, got, want); }
}

static const ld PI_L = 3.141592653589793238462643383279502884L;
static ld norm_logpdf(ld x, ld mu, ld var) { return -0.5L * logl(2.0L * PI_L * var) - 0.5L * (x - mu) * (x - mu) / var; }
static ld ald_logpdf(ld z, ld m, ld s, ld q) { const ld u = (z - m) / s; return logl(q * (1.0L - q) / s) - u * (q - (u < 0.0L ? 1.0L : 0.0L)); }

// ---- logPhi
static ld ref_log_ndtr(double x) { return logl(0.5L * erfcl(-(ld)x / sqrtl(2.0L))); }
static qd ref_log_ndtr_q(double x)
{
    const qd y = (qd)x / sqrtq((qd)2.0);
    return x >= 0.0 ? log1pq(-(qd)0.5 * erfcq(y)) : logq((qd)0.5 * erfcq(-y));
}
static double max_ndtr_err = 0.0, max_ndtr_ref_neg = 0.0, max_ndtr_ref_pos = 0.0;
static void check_ndtr(double x)
{
    const double got = qmarg_log_ndtr(x);
    const ld want = ref_log_ndtr(x);
    const qd wq = ref_log_ndtr_q(x);
    const double ref_err = (double)(fabsq((qd)want - wq) / fabsq(wq)), err_q = (double)(fabsq((qd)got - wq) / fabsq(wq));
    if (x < 0.0) max_ndtr_ref_neg = fmax(max_ndtr_ref_neg, ref_err); else max_ndtr_ref_pos = fmax(max_ndtr_ref_pos, ref_err);
    max_ndtr_err = fmax(max_ndtr_err, err_q);
    check(fabsl((ld)got - want) <= fmaxl(1e-11L, 10.0L * ref_err) * fabsl(want), "logPhi against long double", x, got, (double)want);
    check(err_q <= 1e-11, "logPhi against __float128", x, got, (double)wq);
}
static void run_ndtr()
{
    for (int k = 0; k <= 149 * 64; ++k) check_ndtr(-140.0 + k / 64.0);
    const double joins[] = {QMARG_SERIES_X, nextafter(QMARG_SERIES_X, -1e9), nextafter(QMARG_SERIES_X, 0.0), 0.0, -0.0, 1e-300, -1e-300};
    for (double x : joins) check_ndtr(x);
    // the arms meet: the series and the erfc form one step apart at the join agree far inside the bound
    const double a = qmarg_log_ndtr(nextafter(QMARG_SERIES_X, -1e9)), b = qmarg_log_ndtr(QMARG_SERIES_X);
    check(fabs(a - b) <= 4e-13 * fabs(b), "join of the series and the erfc arm", QMARG_SERIES_X, a, b);
    check(qmarg_log_ndtr(0.0) == qmarg_log_ndtr(-0.0) && fabs(qmarg_log_ndtr(0.0) + log(2.0)) <= 1e-16, "logPhi(0) = -log 2", 0.0, qmarg_log_ndtr(0.0), -log(2.0));
    check(qmarg_served(LATENTQR) && !qmarg_served(CROSSQR) && !qmarg_served(LATENT) && !qmarg_served(RTIRT) && !qmarg_served(MLIRT) && !qmarg_served(NULLM) && !qmarg_served(CROSS), "served", 0, 0, 0);
    check(qmarg_level_ok(0.5) && !qmarg_level_ok(0.0) && !qmarg_level_ok(1.0) && !qmarg_level_ok(-0.1) && !qmarg_level_ok(NAN), "levels", 0, 0, 0);
}

// ---- Gauss-Legendre nodes and weights on [-1, 1] in long double (Newton's iteration on P_n)
static void gauss_legendre(int n, std::vector<ld>& x, std::vector<ld>& w)
{
    x.resize(n); w.resize(n);
    for (int i = 0; i < n; ++i) {
        ld z = cosl(PI_L * (i + 0.75L) / (n + 0.5L)), pp = 0.0L;
        for (int it = 0; it < 100; ++it) {
            ld p1 = 1.0L, p2 = 0.0L;
            for (int j = 1; j <= n; ++j) { const ld p3 = p2; p2 = p1; p1 = ((2.0L * j - 1.0L) * z * p2 - (j - 1.0L) * p3) / j; }
            pp = n * (z * p1 - p2) / (z * z - 1.0L);
            const ld dz = p1 / pp;
            z -= dz;
            if (fabsl(dz) < 1e-19L) break;
        }
        x[i] = z; w[i] = 2.0L / ((1.0L - z * z) * pp * pp);
    }
}
// log of the integral over zeta of prod_j N(t_j; lambda_j - zeta, sig2t_j) ALD(zeta; m, s, q): each side of the kink on `panels` panels from the kink to where the
// side's integrand has fallen 60 nats below its peak
static ld brute_T(int J, const double* t, const double* lam, const double* sg, ld m, ld s, ld q, int panels)
{
    static std::vector<ld> gx, gw;
    if (gx.empty()) gauss_legendre(20, gx, gw);
    auto logf = [&](ld zeta) { ld e = ald_logpdf(zeta, m, s, q); for (int j = 0; j < J; ++j) e += norm_logpdf((ld)t[j], (ld)lam[j] - zeta, (ld)sg[j]); return e; };
    ld P = 0.0L, R0 = 0.0L;
    for (int j = 0; j < J; ++j) { const ld g = 1.0L / (ld)sg[j]; P += g; R0 += g * ((ld)lam[j] - (ld)t[j]); }
    const ld cU = (R0 - q / s) / P, cL = (R0 + (1.0L - q) / s) / P;                 // the centres of the two sides' Gaussians: used to PLACE the panels only
    const ld pU = fmaxl(m, cU), pL = fminl(m, cL);
    const ld hi = cU + sqrtl((pU - cU) * (pU - cU) + 120.0L / P), lo = cL - sqrtl((cL - pL) * (cL - pL) + 120.0L / P);
    const ld top = fmaxl(logf(pU), logf(pL));
    ld sum = 0.0L;
    for (int side = 0; side < 2; ++side) {
        const ld a = side == 0 ? lo : m, b = side == 0 ? m : hi, hp = (b - a) / panels;
        for (int k = 0; k < panels; ++k) {
            const ld c = a + (k + 0.5L) * hp;
            for (size_t i = 0; i < gx.size(); ++i) sum += 0.5L * hp * gw[i] * expl(logf(c + 0.5L * hp * gx[i]) - top);
        }
    }
    return top + logl(sum);
}

static double max_T_err = 0.0, max_T_ref = 0.0;
static void run_T(std::mt19937_64& g, int J, int F, double s, double q, int reps)
{
    std::normal_distribution<double> nd(0.0, 1.0);
    std::uniform_real_distribution<double> ud(0.0, 1.0);
    const int64_t wi = item_trace_width(LATENTQR, J, F);
    for (int rep = 0; rep < reps; ++rep) {
        std::vector<double> row((size_t)wi), t(J), x(F > 0 ? F : 1, 0.0);
        for (int j = 0; j < J; ++j) { row[j] = 0.5 + 1.5 * ud(g); row[J + j] = nd(g); row[2 * J + j] = 4.0 + 0.5 * nd(g); row[3 * J + j] = 0.1 + ud(g); t[j] = 4.0 + nd(g); }
        double* qr = row.data() + 4 * J;
        for (int k = 0; k < F + 2; ++k) qr[k] = 0.4 * nd(g);
        for (int f = 0; f < F; ++f) x[f] = nd(g);
        double* S = qr + qr_sigp_off(LATENTQR, J, F);
        S[0] = 0.5 + ud(g); S[1] = S[2] = 0.0; S[3] = s;
        const MargLaw w = marg_law_row(LATENTQR, qr, J, F, x.data());
        ld m0 = qr[0];
        for (int f = 0; f < F; ++f) m0 += (ld)x[f] * qr[1 + f];
        check(w.mu == 0.0 && w.v == s && fabs(w.sd - sqrt(S[0])) <= 1e-15 && w.m1 == qr[F + 1] && fabs((double)(w.m0 - m0)) <= 1e-14 * (1 + fabsl(m0)), "law", s, w.m0, (double)m0);
        MargSums ms{0, 0, 0, 0, 0, 0, 0};
        for (int j = 0; j < J; ++j) marg_sums_add(ms, 1.0 / row[3 * J + j], log(row[3 * J + j]), row[2 * J + j] - t[j], 0.0);
        for (int k = 0; k < 5; ++k) {
            const double theta = w.mu + w.sd * (-6.0 + 3.0 * k);
            const double got = qmarg_T(ms, J, w, theta, q);
            const ld m = (ld)w.m0 + (ld)w.m1 * theta;
            const ld want = brute_T(J, t.data(), row.data() + 2 * J, row.data() + 3 * J, m, (ld)s, (ld)q, 400);
            const ld half = brute_T(J, t.data(), row.data() + 2 * J, row.data() + 3 * J, m, (ld)s, (ld)q, 200);
            const double ref_err = (double)(fabsl(want - half) / fabsl(want)), err = (double)(fabsl((ld)got - want) / fabsl(want));
            max_T_ref = fmax(max_T_ref, ref_err); max_T_err = fmax(max_T_err, err);
            check(err <= fmax(1e-11, 10.0 * ref_err), "T", theta, got, (double)want);
        }
    }
}

// one l of the rule from the header's host build: q Q J F | row [item_trace_width] | y [J] | t [J] | x [F]
static int one_l(int argc, char** argv)
{
    if (argc < 6) return 2;
    const double q = atof(argv[2]);
    const int Q = atoi(argv[3]), J = atoi(argv[4]), F = atoi(argv[5]);
    const int64_t wi = item_trace_width(LATENTQR, J, F);
    if (!marg_nodes_ok(Q) || J < 1 || F < 0 || argc != 6 + wi + 2 * J + F) return 2;
    std::vector<double> v;
    for (int k = 6; k < argc; ++k) v.push_back(strtod(argv[k], nullptr));
    const double *row = v.data(), *y = row + wi, *t = y + J, *x = t + J;
    const MargLaw w = marg_law_row(LATENTQR, row + 4 * J, J, F, x);
    MargSums ms{0, 0, 0, 0, 0, 0, 0};
    double A1 = 0.0, A0 = 0.0;
    for (int j = 0; j < J; ++j) {
        if (y[j] != 0.0) { A1 += row[j]; A0 += row[j] * row[J + j]; }
        marg_sums_add(ms, 1.0 / row[3 * J + j], log(row[3 * J + j]), row[2 * J + j] - t[j], 0.0);
    }
    const double h = marg_step(Q), log_h = log(h);
    MargMS part{0.0, 0.0};
    for (int k = 0; k < Q; ++k) {
        const double z = marg_node(k, h), th = w.mu + w.sd * z;
        double lse = 0.0;
        for (int j = 0; j < J; ++j) lse += marg_log1pexp(row[j] * (th - row[J + j]));
        marg_ms_add(part, marg_log_weight(z, log_h) + (th * A1 - A0 - lse) + qmarg_T(ms, J, w, th, q));
    }
    printf("l=%.17g S=%.17g\n", marg_ms_log(part), part.S);
    return 0;
}

int main(int argc, char** argv)
{
    if (argc >= 2 && strcmp(argv[1], "L") == 0) return one_l(argc, argv);
    run_ndtr();
    std::mt19937_64 g(20250314);
    for (int J : {1, 7, 65}) for (double q : {0.15, 0.5, 0.85}) for (double s : {0.05, 0.2, 1.0, 6.0}) run_T(g, J, J == 7 ? 3 : 0, s, q, 2);
    printf("logPhi: max rel err against __float128 %.3g; the long-double reference's own: %.3g (x < 0), %.3g (x >= 0)\n", max_ndtr_err, max_ndtr_ref_neg, max_ndtr_ref_pos);
    printf("T: max rel err against the zeta integral %.3g; the reference's own (400 against 200 panels) %.3g\n", max_T_err, max_T_ref);
    printf("failures %d\n", failures);
    return failures ? 1 : 0;
}

// fit_check.cpp -- the pieces of the person fit (extendedrtirtmodeling.jl_amd/csrc/erm_fit.hpp) on the CPU, built with UndefinedBehaviorSanitizer and -ftrapv by
// tests/test_fit_host.py.  The header the kernel includes against independent arithmetic in long double:
//   self        - fit_cell's W and Vw against l0 - E[l0 | theta] and Var[l0 | theta] by enumeration of all 2^J response patterns, J <= 10, theta near the items and
//                 far from every b_j at a_j = 8 (|eta| > 30, where theta A1 - A0 - sum p eta has no digit left); lse against marg_log1pexp bit for bit;
//               - fit_wh against its formula in long double; fit_chi2_tails<4> against fit_chi2_tail bit for bit;
//               - the FitMS merge, the terms dealt to eight lanes and joined by the butterfly the kernel uses, against one-pass long-double sums over terms
//                 spanning -1400 ... 0; M and S equal to MargMS's bit for bit; every lane holds the same six afterwards;
//               - FitAcc against a two-pass long-double computation, weights spanning e^-1400 ... 1 and equal; fit_finish's NaN rules.
//   tail x n .. - prints fit_chi2_tail(x, n) for every pair, for the comparison with scipy.stats.chi2.sf
//   quad J theta m0 m1 v  then J times (sig2t lambda t rho)  - prints fit_rt_quad from the sums marg_sums_add builds, for the comparison with numpy.linalg.solve
// "self" prints "failures N".
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>
#include "erm_fit.hpp"

using namespace erm;
typedef long double ld;

static int failures = 0;
static void check(bool ok, const char* what, double got, double want)
{
    if (!ok) { ++failures; printf("FAIL %s: got %.17g want %.17g\n", what, got, want); }
}

// l0's cell in the form without cancellation, in long double
static ld cell_l0(ld eta, int y) { const ld t = expl(-fabsl(eta)); return ((y == 1) == (eta >= 0.0L) ? 0.0L : -fabsl(eta)) - log1pl(t); }

static void run_cells(std::mt19937_64& g)
{
    std::normal_distribution<double> nd(0.0, 1.0);
    std::uniform_real_distribution<double> ud(0.0, 1.0);
    for (int rep = 0; rep < 24; ++rep) {
        const int J = 1 + rep % 10;
        const bool far = rep % 3 == 2;
        std::vector<double> a(J), b(J);
        for (int j = 0; j < J; ++j) { a[j] = far ? 8.0 : 0.5 + 1.5 * ud(g); b[j] = far ? 2.0 * ud(g) - 1.0 : nd(g); }
        const double theta = far ? (rep % 2 ? 6.0 : -6.0) : nd(g);
        std::vector<ld> eta(J), p1(J);
        for (int j = 0; j < J; ++j) { eta[j] = (ld)(a[j] * (theta - b[j])); const ld t = expl(-fabsl(eta[j])); p1[j] = eta[j] >= 0.0L ? 1.0L / (1.0L + t) : t / (1.0L + t); }
        if (far) for (int j = 0; j < J; ++j) check(fabsl(eta[j]) > 30.0L, "far: |eta| > 30", (double)eta[j], 30.0);
        // enumeration: E and Var of l0 over all patterns
        ld E = 0.0L;
        std::vector<ld> l0(1u << J), pr(1u << J);
        for (unsigned y = 0; y < (1u << J); ++y) {
            ld l = 0.0L, p = 1.0L;
            for (int j = 0; j < J; ++j) { const int yj = (y >> j) & 1; l += cell_l0(eta[j], yj); p *= yj ? p1[j] : 1.0L - p1[j]; }
            if (far) {      // 1 - p1 cancels when p1 is near 1: take the small probability directly
                p = 1.0L;
                for (int j = 0; j < J; ++j) { const int yj = (y >> j) & 1; const ld t = expl(-fabsl(eta[j])); p *= ((yj == 1) == (eta[j] >= 0.0L)) ? 1.0L / (1.0L + t) : t / (1.0L + t); }
            }
            l0[y] = l; pr[y] = p; E += p * l;
        }
        ld Var = 0.0L;
        for (unsigned y = 0; y < (1u << J); ++y) Var += pr[y] * (l0[y] - E) * (l0[y] - E);
        for (unsigned y = 0; y < (1u << J); ++y) {
            double lse = 0.0, W = 0.0, Vw = 0.0, lse_ref = 0.0;
            ld scale = 0.0L;
            for (int j = 0; j < J; ++j) {
                const double e = a[j] * (theta - b[j]);
                fit_cell(e, ((y >> j) & 1) != 0, lse, W, Vw);
                lse_ref += marg_log1pexp(e);
                const ld t = expl(-fabsl(eta[j]));
                scale += fabsl(eta[j]) * (((((y >> j) & 1) == 1) == (eta[j] >= 0.0L)) ? t / (1.0L + t) : 1.0L / (1.0L + t));
            }
            check(lse == lse_ref, "lse is marg_log1pexp's bit for bit", lse, lse_ref);
            check(fabsl((ld)W - (l0[y] - E)) <= 1e-13L * scale + 1e-17L * fabsl(E), "W = l0 - E l0", W, (double)(l0[y] - E));
            check(fabsl((ld)Vw - Var) <= 1e-13L * Var, "Vw = Var l0", Vw, (double)Var);
        }
    }
    check(fit_lz(1.0, 0.0) == 0.0 && fit_phi(0.0) == 0.5 && fit_lz(-3.0, 4.0) == -1.5, "lz at Vw = 0 and its Phi", fit_phi(0.0), 0.5);
    check(fabs(fit_phi(-1.959963984540054) - 0.025) <= 1e-16 && fabs(fit_phi(1.0) + fit_phi(-1.0) - 1.0) <= 2e-16, "Phi", fit_phi(-1.959963984540054), 0.025);
}

static void run_wh_and_chunks(std::mt19937_64& g)
{
    std::uniform_real_distribution<double> ud(0.0, 1.0);
    for (int n : {1, 2, 3, 12, 65, 896}) for (int rep = 0; rep < 20; ++rep) {
        const double x = rep == 0 ? 0.0 : (double)n * 3.0 * ud(g);
        const ld c = 2.0L / (9.0L * n), want = (cbrtl((ld)x / n) - (1.0L - c)) / sqrtl(c);
        // the difference of two numbers near 1, each within a few ulp, divided by sqrt(c): 8 ulp of (cbrt + 1) / sqrt(c)
        check(fabsl((ld)fit_wh(x, n) - want) <= 8.0L * 1.12e-16L * (cbrtl((ld)x / n) + 1.0L) / sqrtl(c), "Wilson-Hilferty", fit_wh(x, n), (double)want);
        const double q[4] = {x, 0.5 * x, 2.0 * x + 1.0, 1500.0};
        double t4[4];
        fit_chi2_tails<4>(q, n, t4);
        for (int c4 = 0; c4 < 4; ++c4) { const double one = fit_chi2_tail(q[c4], n); check(memcmp(&one, &t4[c4], sizeof(double)) == 0, "four tails at once: bit for bit", t4[c4], one); }
        check(t4[3] == 0.0, "tail past y = 700", t4[3], 0.0);
    }
    check(fit_chi2_tail(0.0, 1) == 1.0 && fit_chi2_tail(0.0, 2) == 1.0 && fit_chi2_tail(0.0, 896) == 1.0 && fit_chi2_tail(3.0, 0) == 0.0 && fit_wh(3.0, 0) == 0.0, "tail at 0, n = 0", fit_chi2_tail(0.0, 1), 1.0);
    check(fabs(fit_chi2_tail(2.0, 2) - exp(-1.0)) <= 1e-16, "chi^2_2 tail is e^-x/2", fit_chi2_tail(2.0, 2), exp(-1.0));
}

// the kernel's combination: lane s takes terms s, s + 8, ... in order; three butterfly steps
static FitMS lanes8(const std::vector<double>& e, const std::vector<double> (&v)[4], bool* symmetric, MargMS* plain)
{
    FitMS p[8];
    MargMS m[8];
    for (int s = 0; s < 8; ++s) {
        p[s] = FitMS{0.0, 0.0, 0.0, 0.0, 0.0, 0.0}; m[s] = MargMS{0.0, 0.0};
        for (size_t q = s; q < e.size(); q += 8) { fit_ms_add(p[s], e[q], v[0][q], v[1][q], v[2][q], v[3][q]); marg_ms_add(m[s], e[q]); }
    }
    for (int k = 1; k < 8; k <<= 1) {
        FitMS n[8]; MargMS nm[8];
        for (int s = 0; s < 8; ++s) {
            n[s] = fit_ms_merge(p[s], p[s ^ k]); nm[s] = marg_ms_merge(m[s], m[s ^ k]);
            const FitMS r = fit_ms_merge(p[s ^ k], p[s]);
            if (memcmp(&r, &n[s], sizeof(FitMS)) != 0) *symmetric = false;
        }
        for (int s = 0; s < 8; ++s) { p[s] = n[s]; m[s] = nm[s]; }
    }
    for (int s = 1; s < 8; ++s) if (memcmp(&p[s], &p[0], sizeof(FitMS)) != 0) *symmetric = false;
    *plain = m[0];
    return p[0];
}

static void run_merge(std::mt19937_64& g)
{
    std::uniform_real_distribution<double> ud(0.0, 1.0);
    for (int rep = 0; rep < 200; ++rep) {
        const int Q = 1 + (int)(ud(g) * 130);
        std::vector<double> e(Q), v[4];
        for (auto& x : v) x.resize(Q);
        for (int q = 0; q < Q; ++q) {
            e[q] = -1400.0 * ud(g) * (rep % 3 == 0 ? 1.0 : 0.01);
            v[0][q] = -4.0 + 8.0 * ud(g); v[1][q] = ud(g); v[2][q] = -3.0 + 9.0 * ud(g); v[3][q] = ud(g);
        }
        if (rep % 5 == 0) e[(size_t)(ud(g) * Q)] = 0.0;
        ld mx = -INFINITY, s = 0.0L, sv[4] = {0, 0, 0, 0}, av[4] = {0, 0, 0, 0};
        for (double x : e) if (x > mx) mx = x;
        for (int q = 0; q < Q; ++q) { const ld p = expl((ld)e[q] - mx); s += p; for (int c = 0; c < 4; ++c) { sv[c] += p * v[c][q]; av[c] += p * fabsl((ld)v[c][q]); } }
        bool sym = true;
        MargMS plain;
        const FitMS got = lanes8(e, v, &sym, &plain);
        const double gv[4] = {got.LZ, got.PY, got.LTZ, got.PT};
        check(sym, "the merge is symmetric bit for bit and every lane holds the same six", 0, 0);
        check(got.M == plain.M && got.S == plain.S, "M and S are MargMS's bit for bit", got.S, plain.S);
        check(got.M == (double)mx && fabsl((ld)got.S - s) <= 1e-14L * s, "S", got.S, (double)s);
        for (int c = 0; c < 4; ++c) check(fabsl((ld)gv[c] - sv[c]) <= 1e-14L * av[c], "a weighted sum", gv[c], (double)sv[c]);
        const FitRow r = fit_row(got);
        for (int c = 0; c < 4; ++c) check(fabsl((ld)r.v[c] - sv[c] / s) <= 2e-14L * av[c] / s, "a row mean", r.v[c], (double)(sv[c] / s));
        check(fabsl((ld)r.l - (mx + logl(s))) <= 1e-13L, "l", r.l, (double)(mx + logl(s)));
    }
}

static void acc_against_two_pass(const std::vector<FitRow>& r, bool weighted, const char* what)
{
    FitAcc a{0, 0, 0, {0, 0, 0, 0}};
    for (auto& x : r) fit_acc_add(a, x, weighted);
    double out[FIT_COLS];
    fit_finish(a, true, 5, out);
    ld mx = -INFINITY, W = 0, W2 = 0, sv[4] = {0, 0, 0, 0};
    for (auto& x : r) if (x.l > mx) mx = x.l;
    for (auto& x : r) { const ld om = weighted ? expl((ld)x.l - mx) : 1.0L; W += om; W2 += om * om; for (int c = 0; c < 4; ++c) sv[c] += om * x.v[c]; }
    for (int c = 0; c < 4; ++c) check(fabsl((ld)out[c] - sv[c] / W) <= 1e-13L * fmaxl(1.0L, fabsl(sv[c] / W)), what, out[c], (double)(sv[c] / W));
    check(fabsl((ld)out[FIT_ROW_ESS] - W * W / W2) <= 1e-13L * (W * W / W2) && std::isfinite(out[FIT_ROW_ESS]), what, out[FIT_ROW_ESS], (double)(W * W / W2));
}

static void run_acc(std::mt19937_64& g)
{
    std::normal_distribution<double> nd(0.0, 1.0);
    std::uniform_real_distribution<double> ud(0.0, 1.0);
    auto row = [&](double l) { return FitRow{{-0.5 + nd(g), ud(g), 0.3 + nd(g), ud(g)}, l}; };
    for (int rep = 0; rep < 100; ++rep) {
        const int n = 1 + (int)(ud(g) * 60);
        std::vector<FitRow> r;
        for (int k = 0; k < n; ++k) r.push_back(row(-300.0 - 1400.0 * ud(g) * (rep % 3 == 0 ? 1.0 : rep % 3 == 1 ? 0.01 : 0.001)));
        if (rep % 4 == 0) r[(size_t)(ud(g) * n)].l = -300.0;      // weights down to e^-1400 beside a weight of 1
        acc_against_two_pass(r, true, "weighted rows");
        acc_against_two_pass(r, false, "equal rows");
    }
    std::vector<FitRow> up, down;
    for (int k = 0; k < 40; ++k) { up.push_back(row(-1400.0 + 35.0 * k)); down.push_back(row(-35.0 * k)); }
    acc_against_two_pass(up, true, "rising maximum");
    acc_against_two_pass(down, true, "falling weights");
    for (bool weighted : {false, true}) {
        const FitRow x = row(-812.5);
        FitAcc a{0, 0, 0, {0, 0, 0, 0}};
        fit_acc_add(a, x, weighted);
        double out[FIT_COLS];
        fit_finish(a, true, 3, out);
        check(out[FIT_LZ] == x.v[0] && out[FIT_P_RESP] == x.v[1] && out[FIT_LTZ] == x.v[2] && out[FIT_P_TIME] == x.v[3] && out[FIT_ROW_ESS] == 1.0, "one row", out[FIT_LZ], x.v[0]);
        fit_finish(a, false, 3, out);
        check(out[FIT_LZ] == x.v[0] && out[FIT_P_RESP] == x.v[1] && std::isnan(out[FIT_LTZ]) && std::isnan(out[FIT_P_TIME]), "no response times: NaN", out[FIT_LTZ], NAN);
        fit_finish(a, true, 0, out);
        check(std::isnan(out[FIT_LZ]) && std::isnan(out[FIT_P_RESP]) && std::isnan(out[FIT_LTZ]) && std::isnan(out[FIT_P_TIME]) && out[FIT_ROW_ESS] == 1.0, "no observed cell: NaN", out[FIT_LZ], NAN);
        for (int k = 0; k < 6; ++k) fit_acc_add(a, x, weighted);
        fit_finish(a, true, 3, out);
        check(out[FIT_ROW_ESS] == 7.0 && out[FIT_LZ] == x.v[0], "identical rows", out[FIT_ROW_ESS], 7.0);
    }
}

int main(int argc, char** argv)
{
    if (argc >= 2 && !strcmp(argv[1], "tail")) {
        for (int k = 2; k + 1 < argc; k += 2) printf("%.17g\n", fit_chi2_tail(atof(argv[k]), atoi(argv[k + 1])));
        return 0;
    }
    if (argc >= 7 && !strcmp(argv[1], "quad")) {
        const int J = atoi(argv[2]);
        const double theta = atof(argv[3]);
        const MargLaw w{0.0, 1.0, atof(argv[4]), atof(argv[5]), atof(argv[6])};
        if (argc != 7 + 4 * J) return 2;
        MargSums ms{0, 0, 0, 0, 0, 0, 0};
        for (int j = 0; j < J; ++j) {
            const double sg = atof(argv[7 + 4 * j]), lam = atof(argv[8 + 4 * j]), t = atof(argv[9 + 4 * j]), rho = atof(argv[10 + 4 * j]);
            marg_sums_add(ms, 1.0 / sg, log(sg), lam - t, rho);
        }
        const double qf = fit_rt_quad(ms, w, theta);
        // exactly -2 (marg_T - its constants)
        const double back = -2.0 * (marg_T(ms, J, w, theta) + 0.5 * (double)J * MARG_LOG_2PI + 0.5 * ms.L + 0.5 * log1p(w.v * ms.P));
        printf("%.17g\n%.17g\n", qf, back);
        return 0;
    }
    std::mt19937_64 g(20250314);
    run_cells(g);
    run_wh_and_chunks(g);
    run_merge(g);
    run_acc(g);
    printf("failures %d\n", failures);
    return failures ? 1 : 0;
}

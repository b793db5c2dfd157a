// score_check.cpp -- the closed forms behind the scores of respondents (extendedrtirtmodeling.jl_amd/csrc/erm_score.hpp) on the CPU, built with
// UndefinedBehaviorSanitizer by tests/test_score_host.py.  The header the kernel includes against independent arithmetic in long double:
//   - score_zeta's (c0, c1, u) against a brute-force zeta grid of the product of the J normal densities and zeta's prior: the grid's mean at two values of theta gives
//     c0 and c1, its variance u (at v = 0: zeta = m0 + m1 theta exactly, u = 0); four models, J in {1, 7, 65}, v = 0 included, rho != 0 for Cross: 1e-11 relative;
//   - the (M, S, S1, S2) merge, the terms dealt to eight lanes and joined by the butterfly the kernel uses, against one-pass long-double sums over terms spanning
//     -1400 ... 0; M and S equal to MargMS's bit for bit; fewer terms than lanes;
//   - the weighted row accumulator against a two-pass long-double computation: weights spanning e^-1400 ... 1, equal weights, one row, all rows identical (equal
//     weights then give row_ess = n exactly and a between-row variance of exactly 0).
// Prints "failures N".
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>
#include "erm_score.hpp"

using namespace erm;
typedef long double ld;

static int failures = 0;
static void check(bool ok, const char* what, double got, double want)
{
    if (!ok) { ++failures; printf("FAIL %s: got %.17g want %.17g\n", what, got, want); }
}
static bool close_rel(double got, ld want, double tol) { return fabs((double)((ld)got - want)) <= tol * fmax(fabs((double)want), 1e-300); }

// mean and variance of zeta given theta and t by the trapezoid rule on prod_j N(t_j; lambda_j - zeta - rho_j theta, sig2t_j) N(zeta; m, v)
static void brute_zeta(int J, const double* t, const double* lam, const double* sg, const double* rho, ld theta, ld m, ld v, ld* mean, ld* var)
{
    ld P = 0.0L, R = 0.0L;
    for (int j = 0; j < J; ++j) { const ld g = 1.0L / (ld)sg[j]; P += g; R += g * ((ld)lam[j] - (ld)t[j] - (ld)rho[j] * theta); }
    const ld pv = 1.0L / (P + 1.0L / v), pm = pv * (R + m / v), psd = sqrtl(pv);      // used to PLACE the grid only
    const int n = 8001;
    const ld lo = pm - 16.0L * psd, h = 32.0L * psd / (n - 1);
    std::vector<ld> e(n);
    ld mx = -INFINITY;
    for (int k = 0; k < n; ++k) {
        const ld z = lo + k * h;
        ld s = -0.5L * (z - m) * (z - m) / v;
        for (int j = 0; j < J; ++j) { const ld d = (ld)t[j] - ((ld)lam[j] - z - (ld)rho[j] * theta); s -= 0.5L * d * d / (ld)sg[j]; }
        e[k] = s;
        if (s > mx) mx = s;
    }
    ld s0 = 0.0L, s1 = 0.0L, s2 = 0.0L;
    for (int k = 0; k < n; ++k) { const ld p = expl(e[k] - mx), dz = lo + k * h - pm; s0 += p; s1 += p * dz; s2 += p * dz * dz; }      // moments about pm: no cancellation
    const ld d1 = s1 / s0;
    *mean = pm + d1;
    *var = s2 / s0 - d1 * d1;
}

static void run_zeta(std::mt19937_64& g, int model, int J, bool v0, int reps)
{
    std::normal_distribution<double> nd(0.0, 1.0);
    std::uniform_real_distribution<double> ud(0.0, 1.0);
    for (int rep = 0; rep < reps; ++rep) {
        std::vector<double> t(J), lam(J), sg(J), rho(J, 0.0);
        for (int j = 0; j < J; ++j) { lam[j] = 4.0 + 0.5 * nd(g); sg[j] = 0.1 + ud(g); t[j] = 4.0 + nd(g); if (model == CROSS) rho[j] = 0.3 * nd(g); }
        const double s1 = 0.5 + ud(g), s2 = 0.25 + ud(g), r = 1.6 * ud(g) - 0.8;
        double S[4] = {s1 * s1, r * s1 * s2, r * s1 * s2, s2 * s2};
        if (v0 && model != LATENT) { S[0] = 4.0; S[1] = S[2] = 2.0; S[3] = 1.0; }
        if (v0 && model == LATENT) S[3] = 0.0;
        const MargLaw w = marg_law(model, 0.3 * nd(g), 0.3 * nd(g), 0.4 * nd(g), S);
        if (v0) check(w.v == 0.0, "v exactly 0", w.v, 0.0);
        MargSums ms{0, 0, 0, 0, 0, 0, 0};
        for (int j = 0; j < J; ++j) marg_sums_add(ms, 1.0 / sg[j], log(sg[j]), lam[j] - t[j], rho[j]);
        const ScoreZeta k = score_zeta(ms, w);
        const ld th0 = -1.25L, th1 = 2.5L;
        ld e0, e1, u0, u1;
        if (w.v == 0.0) { e0 = (ld)w.m0 + (ld)w.m1 * th0; e1 = (ld)w.m0 + (ld)w.m1 * th1; u0 = u1 = 0.0L; }
        else {
            brute_zeta(J, t.data(), lam.data(), sg.data(), rho.data(), th0, (ld)w.m0 + (ld)w.m1 * th0, (ld)w.v, &e0, &u0);
            brute_zeta(J, t.data(), lam.data(), sg.data(), rho.data(), th1, (ld)w.m0 + (ld)w.m1 * th1, (ld)w.v, &e1, &u1);
        }
        const ld c1 = (e1 - e0) / (th1 - th0), c0 = e0 - c1 * th0;
        check(close_rel(k.c0, c0, 1e-11), "c0", k.c0, (double)c0);
        check(close_rel(k.c1, c1, 1e-11), "c1", k.c1, (double)c1);
        check(w.v == 0.0 ? k.u == 0.0 : (close_rel(k.u, u0, 1e-11) && close_rel(k.u, u1, 1e-11)), "u", k.u, (double)u0);
    }
}

// the kernel's combination: lane s takes terms s, s + 8, ... in order; three butterfly steps
static ScoreMS lanes8(const std::vector<double>& e, const std::vector<double>& z, bool* symmetric, MargMS* plain)
{
    ScoreMS p[8];
    MargMS m[8];
    for (int s = 0; s < 8; ++s) {
        p[s] = ScoreMS{0.0, 0.0, 0.0, 0.0}; m[s] = MargMS{0.0, 0.0};
        for (size_t q = s; q < e.size(); q += 8) { score_ms_add(p[s], e[q], z[q]); marg_ms_add(m[s], e[q]); }
    }
    for (int k = 1; k < 8; k <<= 1) {
        ScoreMS n[8]; MargMS nm[8];
        for (int s = 0; s < 8; ++s) { n[s] = score_ms_merge(p[s], p[s ^ k]); nm[s] = marg_ms_merge(m[s], m[s ^ k]); }
        for (int s = 0; s < 8; ++s) { p[s] = n[s]; m[s] = nm[s]; }
    }
    for (int s = 1; s < 8; ++s) if (memcmp(&p[s], &p[0], sizeof(ScoreMS)) != 0) *symmetric = false;
    *plain = m[0];
    return p[0];
}

static void run_merge(std::mt19937_64& g)
{
    std::uniform_real_distribution<double> ud(0.0, 1.0);
    for (int rep = 0; rep < 200; ++rep) {
        const int Q = 1 + (int)(ud(g) * 130);
        std::vector<double> e(Q), z(Q);
        for (int q = 0; q < Q; ++q) { e[q] = -1400.0 * ud(g) * (rep % 3 == 0 ? 1.0 : 0.01); z[q] = -6.0 + 12.0 * ud(g); }
        if (rep % 5 == 0) e[(size_t)(ud(g) * Q)] = 0.0;
        ld mx = -INFINITY, s = 0.0L, s1 = 0.0L, s2 = 0.0L, a1 = 0.0L;
        for (double v : e) if (v > mx) mx = v;
        for (int q = 0; q < Q; ++q) { const ld p = expl((ld)e[q] - mx); s += p; s1 += p * z[q]; s2 += p * (ld)z[q] * z[q]; a1 += p * fabsl((ld)z[q]); }
        bool sym = true;
        MargMS plain;
        const ScoreMS got = lanes8(e, z, &sym, &plain);
        check(sym, "butterfly leaves every lane with the same four", 0, 0);
        check(got.M == plain.M && got.S == plain.S, "M and S are MargMS's bit for bit", got.S, plain.S);
        check(got.M == (double)mx && close_rel(got.S, s, 1e-14), "S", got.S, (double)s);
        check(fabs((double)((ld)got.S1 - s1)) <= 1e-14 * (double)a1, "S1", got.S1, (double)s1);      // S1's terms change sign: relative to sum |terms|
        check(close_rel(got.S2, s2, 1e-14), "S2", got.S2, (double)s2);
    }
    {   // fewer terms than lanes: empty partial sums
        bool sym = true;
        MargMS plain;
        const ScoreMS got = lanes8({-3.0, -1400.0, -2.0}, {1.0, 5.0, -2.0}, &sym, &plain);
        const double f = exp(-1.0);
        check(sym && got.M == -2.0 && fabs(got.S - (1.0 + f)) <= 1e-15 && fabs(got.S1 - (-2.0 + f)) <= 1e-15 && fabs(got.S2 - (4.0 + f)) <= 1e-15, "three terms", got.S1, -2.0 + f);
    }
}

struct Two { ld th, var_t, ze, var_z, cov, ess; };
static Two two_pass(const std::vector<ScoreRow>& r, bool weighted)
{
    ld mx = -INFINITY;
    for (auto& x : r) if (x.l > mx) mx = x.l;
    ld W = 0, W2 = 0, sE = 0, sZ = 0, sV = 0, sVz = 0, sC = 0;
    for (auto& x : r) { const ld om = weighted ? expl((ld)x.l - mx) : 1.0L; W += om; W2 += om * om; sE += om * x.E; sZ += om * x.Ez; sV += om * x.V; sVz += om * x.Vz; sC += om * x.C; }
    const ld mE = sE / W, mZ = sZ / W;
    ld bE = 0, bZ = 0, bC = 0;
    for (auto& x : r) { const ld om = weighted ? expl((ld)x.l - mx) : 1.0L; bE += om * (x.E - mE) * (x.E - mE); bZ += om * (x.Ez - mZ) * (x.Ez - mZ); bC += om * (x.E - mE) * (x.Ez - mZ); }
    return {mE, sV / W + bE / W, mZ, sVz / W + bZ / W, sC / W + bC / W, W * W / W2};
}
static void acc_against_two_pass(const std::vector<ScoreRow>& r, bool weighted, const char* what)
{
    ScoreAcc a{0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (auto& x : r) score_acc_add(a, x, weighted);
    double out[SCORE_COLS];
    score_finish(a, true, out);
    const Two w = two_pass(r, weighted);
    const double tol = 1e-13;
    check(fabs((double)((ld)out[SCORE_THETA] - w.th)) <= tol * fmax(1.0, fabs((double)w.th)), what, out[SCORE_THETA], (double)w.th);
    check(fabs((double)((ld)out[SCORE_ZETA] - w.ze)) <= tol * fmax(1.0, fabs((double)w.ze)), what, out[SCORE_ZETA], (double)w.ze);
    check(close_rel(out[SCORE_THETA_SD], sqrtl(w.var_t), tol), what, out[SCORE_THETA_SD], (double)sqrtl(w.var_t));
    check(close_rel(out[SCORE_ZETA_SD], sqrtl(w.var_z), tol), what, out[SCORE_ZETA_SD], (double)sqrtl(w.var_z));
    check(fabs((double)((ld)out[SCORE_COV] - w.cov)) <= tol * (double)sqrtl(w.var_t * w.var_z), what, out[SCORE_COV], (double)w.cov);
    check(close_rel(out[SCORE_ROW_ESS], w.ess, tol) && std::isfinite(out[SCORE_ROW_ESS]), what, out[SCORE_ROW_ESS], (double)w.ess);
}

static void run_acc(std::mt19937_64& g)
{
    std::normal_distribution<double> nd(0.0, 1.0);
    std::uniform_real_distribution<double> ud(0.0, 1.0);
    auto row = [&](double l) { const double E = 0.7 + 0.3 * nd(g), V = 0.05 + 0.2 * ud(g), c1 = 0.5 * nd(g); return ScoreRow{E, V, -0.2 + c1 * E + 0.1 * nd(g), 0.02 + c1 * c1 * V, c1 * V, l}; };
    for (int rep = 0; rep < 100; ++rep) {
        const int n = 1 + (int)(ud(g) * 60);
        std::vector<ScoreRow> r;
        for (int k = 0; k < n; ++k) r.push_back(row(-300.0 - 1400.0 * ud(g) * (rep % 3 == 0 ? 1.0 : rep % 3 == 1 ? 0.01 : 0.001)));
        if (rep % 4 == 0) r[(size_t)(ud(g) * n)].l = -300.0;      // weights down to e^-1400 beside a weight of 1
        acc_against_two_pass(r, true, "weighted rows");
        acc_against_two_pass(r, false, "equal rows");
    }
    {   // ascending and descending l: the maximum rises at every row / never
        std::vector<ScoreRow> up, down;
        for (int k = 0; k < 40; ++k) { up.push_back(row(-1400.0 + 35.0 * k)); down.push_back(row(-35.0 * k)); }
        acc_against_two_pass(up, true, "rising maximum");
        acc_against_two_pass(down, true, "falling weights");
    }
    for (bool weighted : {false, true}) {      // one row: its own moments, row_ess 1
        const ScoreRow x = row(-812.5);
        ScoreAcc a{0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
        score_acc_add(a, x, weighted);
        double out[SCORE_COLS];
        score_finish(a, true, out);
        check(out[SCORE_THETA] == x.E && out[SCORE_THETA_SD] == sqrt(x.V) && out[SCORE_ZETA] == x.Ez && out[SCORE_ZETA_SD] == sqrt(x.Vz) && out[SCORE_COV] == x.C &&
              out[SCORE_ROW_ESS] == 1.0, "one row", out[SCORE_THETA_SD], sqrt(x.V));
        score_finish(a, false, out);
        check(out[SCORE_THETA] == x.E && std::isnan(out[SCORE_ZETA]) && std::isnan(out[SCORE_ZETA_SD]) && std::isnan(out[SCORE_COV]), "no zeta: NaN", out[SCORE_ZETA], NAN);
    }
    for (int n : {2, 7, 100}) for (bool weighted : {false, true}) {      // all rows identical: no between-row variance, row_ess = n
        const ScoreRow x = row(-77.0);
        ScoreAcc a{0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
        for (int k = 0; k < n; ++k) score_acc_add(a, x, weighted);
        double out[SCORE_COLS];
        score_finish(a, true, out);
        check(a.M2E == 0.0 && a.M2Z == 0.0 && a.CEZ == 0.0 && out[SCORE_ROW_ESS] == (double)n, "identical rows", out[SCORE_ROW_ESS], (double)n);
        check(out[SCORE_THETA] == x.E && fabs(out[SCORE_THETA_SD] - sqrt(x.V)) <= 4e-16 * sqrt(x.V) && fabs(out[SCORE_COV] - x.C) <= 4e-16 * fabs(x.C), "identical rows: the row's moments",
              out[SCORE_THETA_SD], sqrt(x.V));
    }
}

static void run_row()
{
    // a rule of three nodes with weights 1/4, 1/2, 1/4 at z = -1, 0, 1: Z1 = 0, Z2 = 1/2
    ScoreMS p{0.0, 0.0, 0.0, 0.0};
    score_ms_add(p, log(0.25), -1.0); score_ms_add(p, log(0.5), 0.0); score_ms_add(p, log(0.25), 1.0);
    const MargLaw w{0.5, 2.0, 0.1, 0.3, 0.0};
    const ScoreRow r = score_row(p, w, ScoreZeta{0.1, 0.3, 0.04});
    check(fabs(r.E - 0.5) <= 1e-16 && fabs(r.V - 2.0) <= 1e-15 && fabs(r.Ez - 0.25) <= 1e-16 && fabs(r.Vz - (0.04 + 0.09 * 2.0)) <= 1e-15 && fabs(r.C - 0.6) <= 1e-15 && fabs(r.l) <= 1e-15,
          "row moments", r.V, 2.0);
    check(score_weighting_ok(SCORE_EQUAL) && score_weighting_ok(SCORE_LIKELIHOOD) && !score_weighting_ok(2) && !score_weighting_ok(-1), "weightings", 0, 0);
}

int main()
{
    std::mt19937_64 g(20240917);
    const int models[4] = {RTIRT, NULLM, CROSS, LATENT};
    for (int m : models) for (int J : {1, 7, 65}) for (int v0 = 0; v0 < 2; ++v0) run_zeta(g, m, J, v0 == 1, 6);
    run_merge(g);
    run_acc(g);
    run_row();
    printf("failures %d\n", failures);
    return failures ? 1 : 0;
}

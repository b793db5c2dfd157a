// marginal_check.cpp -- the marginal WAIC's closed forms (extendedrtirtmodeling.jl_amd/csrc/erm_marginal.hpp) on the CPU, built with UndefinedBehaviorSanitizer by
// tests/test_marginal_host.py.  The header the kernel includes against independent arithmetic in long double:
//   - marg_T(theta), zeta integrated out in closed form, against a brute-force zeta grid of the product of the J normal densities and zeta's conditional law
//     (at v = 0: the product evaluated at zeta = m), for the five models, J in {1, 7, 65}, rho != 0 for Cross, random rows and subjects: 1e-11 relative;
//   - marg_law_row against the table written out per model;
//   - the (M, S) merge, in every split of the terms over eight lanes joined by the butterfly the kernel uses, against a one-pass log-sum in long double over terms
//     spanning -1400 ... 0; an empty partial sum; a degenerate rule (all e_q equal: S = Q exactly);
//   - the node rule: z_0 = -6, z_(Q-1) = 6, the middle node 0, and sum_q exp(log weight) = 1 to the trapezoid rule's accuracy.
// Prints "failures N"; `marginal_check T ...` prints single values for the Python side.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>
#include "erm_marginal.hpp"

using namespace erm;
typedef long double ld;

static int failures = 0;
static void check(bool ok, const char* what, double got, double want)
{
    if (!ok) { ++failures; printf("FAIL %s: got %.17g want %.17g\n", what, got, want); }
}

static const ld PI_L = 3.141592653589793238462643383279502884L;
static ld norm_logpdf(ld x, ld mu, ld var) { return -0.5L * logl(2.0L * PI_L * var) - 0.5L * (x - mu) * (x - mu) / var; }

// log of the integral over zeta of prod_j N(t_j; lambda_j - zeta - rho_j theta, sig2t_j) N(zeta; m, v), by the trapezoid rule around the integrand's mode
static ld brute_T(int J, const double* t, const double* lam, const double* sg, const double* rho, ld theta, ld m, ld v)
{
    auto loglik = [&](ld zeta) { ld s = 0.0L; for (int j = 0; j < J; ++j) s += norm_logpdf((ld)t[j], (ld)lam[j] - zeta - (ld)rho[j] * theta, (ld)sg[j]); return s; };
    if (v == 0.0L) return loglik(m);
    ld P = 0.0L, R = 0.0L;
    for (int j = 0; j < J; ++j) { const ld g = 1.0L / (ld)sg[j]; P += g; R += g * ((ld)lam[j] - (ld)t[j] - (ld)rho[j] * theta); }
    const ld pv = 1.0L / (P + 1.0L / v), pm = pv * (R + m / v), psd = sqrtl(pv);      // zeta's conditional law given t: used to PLACE the grid only
    const int n = 4001;
    const ld lo = pm - 14.0L * psd, h = 28.0L * psd / (n - 1);
    std::vector<ld> e(n);
    ld mx = -INFINITY;
    for (int k = 0; k < n; ++k) { const ld z = lo + k * h; e[k] = loglik(z) + norm_logpdf(z, m, v); if (e[k] > mx) mx = e[k]; }
    ld s = 0.0L;
    for (int k = 0; k < n; ++k) s += expl(e[k] - mx);
    return mx + logl(s * h);
}

struct Case { int model, J, F; bool v0; };

static void run_T(std::mt19937_64& g, const Case& c, int reps)
{
    std::normal_distribution<double> nd(0.0, 1.0);
    std::uniform_real_distribution<double> ud(0.0, 1.0);
    const int J = c.J, F = kernel_feat(c.model, c.F);
    const int64_t wi = item_trace_width(c.model, J, F);
    for (int rep = 0; rep < reps; ++rep) {
        std::vector<double> row((size_t)wi), t(J), x(F > 0 ? F : 1, 0.0), rho(J, 0.0);
        for (int j = 0; j < J; ++j) { row[j] = 0.5 + 1.5 * ud(g); row[J + j] = nd(g); row[2 * J + j] = 4.0 + 0.5 * nd(g); row[3 * J + j] = 0.1 + ud(g); t[j] = 4.0 + nd(g); }
        double* q = row.data() + 4 * J;
        for (int k = 0; k < qr_sigp_off(c.model, J, F); ++k) q[k] = model_traits(c.model).beta == BETA_ZERO_PAIR ? 0.0 : 0.4 * nd(g);
        if (model_traits(c.model).rho) for (int j = 0; j < J; ++j) rho[j] = q[j];
        for (int f = 0; f < F; ++f) x[f] = nd(g);
        double* S = q + qr_sigp_off(c.model, J, F);
        const double s1 = 0.5 + ud(g), s2 = 0.25 + ud(g), r = c.v0 ? 1.0 : 1.6 * ud(g) - 0.8;
        if (c.v0 && c.model != LATENT) { S[0] = 4.0; S[1] = S[2] = 2.0; S[3] = 1.0; }      // correlation exactly 1 in exact arithmetic: v = 1 - 4 / 4
        else { S[0] = s1 * s1; S[1] = S[2] = r * s1 * s2; S[3] = (c.v0 && c.model == LATENT) ? 0.0 : s2 * s2; }
        const MargLaw w = marg_law_row(c.model, q, J, F, x.data());
        // the table, written out
        ld xb0 = 0.0L, xb1 = 0.0L;
        if (c.model == RTIRT || c.model == LATENT) { xb0 = q[0]; for (int f = 0; f < F; ++f) xb0 += (ld)x[f] * q[1 + f]; }
        if (c.model == RTIRT) { xb1 = q[F + 1]; for (int f = 0; f < F; ++f) xb1 += (ld)x[f] * q[F + 2 + f]; }
        const ld s11 = S[0], s12 = 0.5L * ((ld)S[1] + S[2]), s22 = S[3];
        ld mu, m0, m1, v;
        if (c.model == LATENT) { mu = 0; m0 = xb0; m1 = q[F + 1]; v = s22; }
        else { mu = c.model == RTIRT ? xb0 : 0.0L; m1 = s12 / s11; m0 = c.model == RTIRT ? xb1 - m1 * xb0 : 0.0L; v = s22 - s12 * s12 / s11; }
        check(fabs((double)(w.mu - mu)) <= 1e-14 * (1 + fabsl(mu)) && fabs((double)(w.m0 - m0)) <= 1e-14 * (1 + fabsl(m0)) && fabs((double)(w.m1 - m1)) <= 1e-14 * (1 + fabsl(m1)) &&
              fabs((double)(w.v - v)) <= 1e-14 * (1 + fabsl(v)) && fabs((double)(w.sd - sqrtl(s11))) <= 1e-15 * (double)sqrtl(s11), "law", w.v, (double)v);
        if (c.v0) check(w.v == 0.0, "v exactly 0", w.v, 0.0);
        MargSums ms{0, 0, 0, 0, 0, 0, 0};
        for (int j = 0; j < J; ++j) marg_sums_add(ms, 1.0 / row[3 * J + j], log(row[3 * J + j]), row[2 * J + j] - t[j], rho[j]);
        for (int k = 0; k < 5; ++k) {
            const double theta = w.mu + w.sd * (-6.0 + 3.0 * k);
            const double got = marg_T(ms, J, w, theta);
            const ld want = brute_T(J, t.data(), row.data() + 2 * J, row.data() + 3 * J, rho.data(), (ld)theta, (ld)w.m0 + (ld)w.m1 * theta, (ld)w.v);
            check(fabs((double)(got - want)) <= 1e-11 * fabs((double)want), "T", got, (double)want);
        }
    }
}

// the kernel's combination: lane s takes terms s, s + 8, ... in order; three butterfly steps of marg_ms_merge
static MargMS lanes8(const std::vector<double>& e, bool* symmetric)
{
    MargMS p[8];
    for (int s = 0; s < 8; ++s) { p[s] = MargMS{0.0, 0.0}; for (size_t q = s; q < e.size(); q += 8) marg_ms_add(p[s], e[q]); }
    for (int m = 1; m < 8; m <<= 1) {
        MargMS n[8];
        for (int s = 0; s < 8; ++s) n[s] = marg_ms_merge(p[s], p[s ^ m]);
        for (int s = 0; s < 8; ++s) p[s] = n[s];
    }
    for (int s = 1; s < 8; ++s) if (memcmp(&p[s], &p[0], sizeof(MargMS)) != 0) *symmetric = false;
    return p[0];
}

static void run_merge(std::mt19937_64& g)
{
    std::uniform_real_distribution<double> ud(0.0, 1.0);
    for (int rep = 0; rep < 200; ++rep) {
        const int Q = 1 + (int)(ud(g) * 130);
        std::vector<double> e(Q);
        for (int q = 0; q < Q; ++q) e[q] = -1400.0 * ud(g) * (rep % 3 == 0 ? 1.0 : 0.01);
        if (rep % 5 == 0) e[(size_t)(ud(g) * Q)] = 0.0;
        ld mx = -INFINITY, s = 0.0L;
        for (double v : e) if (v > mx) mx = v;
        for (double v : e) s += expl((ld)v - mx);
        const ld want = mx + logl(s);
        bool sym = true;
        const MargMS got = lanes8(e, &sym);
        check(sym, "butterfly leaves every lane with the same pair", 0, 0);
        check(fabs((double)(marg_ms_log(got) - want)) <= 1e-14 * fmax(1.0, fabs((double)want)), "merge", marg_ms_log(got), (double)want);
    }
    {   // fewer terms than lanes: empty partial sums
        bool sym = true;
        const MargMS got = lanes8({-3.0, -1400.0, -2.0}, &sym);
        check(sym && fabs(marg_ms_log(got) - log(exp(-3.0) + exp(-2.0))) <= 1e-15, "three terms", marg_ms_log(got), log(exp(-3.0) + exp(-2.0)));
    }
    for (int Q : {3, 61, 127}) {      // a degenerate rule: all e_q equal
        bool sym = true;
        const MargMS got = lanes8(std::vector<double>((size_t)Q, -7.25), &sym);
        check(sym && got.M == -7.25 && got.S == (double)Q, "degenerate rule", got.S, (double)Q);
    }
}

static void run_rule()
{
    for (int Q : {3, 21, 41, 61, 127, 1025}) {
        const double h = marg_step(Q);
        check(marg_nodes_ok(Q) && marg_node(0, h) == -6.0 && fabs(marg_node(Q - 1, h) - 6.0) <= 1e-14 && fabs(marg_node(Q / 2, h)) <= 1e-14, "nodes", marg_node(Q - 1, h), 6.0);
        if (Q >= 21) {
            double s = 0.0;
            for (int q = 0; q < Q; ++q) s += exp(marg_log_weight(marg_node(q, h), log(h)));
            check(fabs(s - 1.0) <= (Q >= 41 ? 1e-8 : 1e-3), "weights", s, 1.0);      // (the mass beyond +-6 is 2e-9)
        }
    }
    check(!marg_nodes_ok(2) && !marg_nodes_ok(60) && !marg_nodes_ok(1027) && !marg_nodes_ok(1) && !marg_nodes_ok(-3), "node counts refused", 0, 0);
    check(marg_served(MLIRT) && marg_served(RTIRT) && marg_served(NULLM) && marg_served(CROSS) && marg_served(LATENT) && !marg_served(CROSSQR) && !marg_served(LATENTQR), "served", 0, 0);
}

int main(int argc, char** argv)
{
    if (argc >= 2 && strcmp(argv[1], "T") == 0) {      // T P R0 R1 D0 D1 D2 L J m0 m1 v theta
        if (argc != 14) return 2;
        double a[12];
        for (int k = 0; k < 12; ++k) a[k] = atof(argv[2 + k]);
        const MargSums ms{a[0], a[1], a[2], a[3], a[4], a[5], a[6]};
        printf("T=%.17g\n", marg_T(ms, (int)a[7], MargLaw{0.0, 1.0, a[8], a[9], a[10]}, a[11]));
        return 0;
    }
    std::mt19937_64 g(20240611);
    const int models[4] = {RTIRT, NULLM, CROSS, LATENT};
    for (int m : models) for (int J : {1, 7, 65}) for (int v0 = 0; v0 < 2; ++v0) run_T(g, Case{m, J, m == RTIRT || m == LATENT ? 3 : 0, v0 == 1}, 6);
    run_T(g, Case{RTIRT, 7, 0, false}, 3);
    {   // MlIrt: the law only (no response times: T = 0 by definition)
        const double q[4] = {0.3, -0.2, 0.5, 0.1}, x[3] = {1.0, -2.0, 0.5};
        const MargLaw w = marg_law_row(MLIRT, q, 7, 3, x);
        check(fabs(w.mu - (0.3 - 0.2 - 1.0 + 0.05)) <= 1e-15 && w.sd == 1.0 && w.v == 0.0 && w.m0 == 0.0 && w.m1 == 0.0, "MlIrt law", w.mu, -0.85);
    }
    run_merge(g);
    run_rule();
    printf("failures %d\n", failures);
    return failures ? 1 : 0;
}

// ifit_check.cpp -- the pieces of the item fit (extendedrtirtmodeling.jl_amd/csrc/erm_ifit.hpp) on the CPU, built with UndefinedBehaviorSanitizer and -ftrapv by
// tests/test_ifit_host.py.  usage: ifit_check self
//   the four response values of a cell against long-double direct forms (the cell's two probabilities from expl, r = |y - p| the one of them, c their product, z^2 = r^2 / c) at
//   |eta| in {0, 1e-300, 30, 699, 701, 1e4} and on a grid, both signs, both responses; the response-time residual against the dense conditional Gaussian in long
//   double (Gauss elimination on diag(sig2t) + v 1 1' without row j) with v = 0, n_i = 1 (P - g = 0), sig2t = 1e-8 and rho != 0; ifit_finish and its NaN rules;
//   ifit_chunk; the reduction as a partition: every subject once for N in {1, 255, 256, 257, 600, 100 000} at several caps, the result the same bits at every cap.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>
#include "erm_ifit.hpp"

using namespace erm;
typedef long double ld;

static int failures = 0;
static double worst_resp = 0.0, worst_d = 0.0;
static void expect(bool ok, const char* what, double a = 0.0, double b = 0.0)
{
    if (!ok) { ++failures; printf("FAIL %s (%.17g against %.17g)\n", what, a, b); }
}
static double rel(double got, ld ref) { const ld s = fabsl(ref) > 1.0L ? fabsl(ref) : 1.0L; return (double)(fabsl((ld)got - ref) / s); }

static void check_resp(double eta, bool y)
{
    double e, r2, c, z2;
    ifit_resp(eta, y, e, r2, c, z2);
    const ld x = (ld)eta;
    const ld q = 1.0L / (1.0L + expl(fabsl(x))), big = 1.0L / (1.0L + expl(-fabsl(x)));      // the two probabilities of the cell, neither by a difference
    const ld r = y == (eta >= 0.0) ? q : big;                                               // |y - p|
    const ld cc = q * big;
    const ld ae = fabsl(x) < 700.0L ? fabsl(x) : 700.0L;
    const bool agree = y == (eta >= 0.0);
    const ld zz = fabs(eta) <= 700.0 ? r * r / cc : (agree ? expl(-fabsl(x)) : expl(ae));      // past the clamp: the definition's own value
    const double errs[4] = {rel(e, y ? r : -r), rel(r2, r * r), rel(c, cc), rel(z2, zz)};
    for (int k = 0; k < 4; ++k) {
        if (errs[k] > worst_resp) worst_resp = errs[k];
        expect(errs[k] <= 4e-15, "ifit_resp against the long-double direct form", eta, errs[k]);
    }
    expect(std::isfinite(z2) && std::isfinite(e) && r2 >= 0.0 && c >= 0.0 && c <= 0.25, "ifit_resp: finite, c in [0, 1/4]", eta, z2);
}

// d of item j among n items by the dense conditional Gaussian: u ~ N(m 1, diag(sig) + v 1 1')
static ld dense_d(int n, int j, const ld* sig, const ld* u, ld m, ld v)
{
    const int k = n - 1;
    if (k == 0) return -(u[j] - m) / sqrtl(sig[j] + v);
    std::vector<ld> A((size_t)k * (k + 2));      // [S_oo | S_oj | u_o - m]
    std::vector<int> o;
    for (int a = 0; a < n; ++a) if (a != j) o.push_back(a);
    const int W = k + 2;
    for (int a = 0; a < k; ++a) {
        for (int b = 0; b < k; ++b) A[(size_t)a * W + b] = v + (a == b ? sig[o[a]] : 0.0L);
        A[(size_t)a * W + k] = v;
        A[(size_t)a * W + k + 1] = u[o[a]] - m;
    }
    for (int p = 0; p < k; ++p) {                // elimination with partial pivoting
        int best = p;
        for (int a = p + 1; a < k; ++a) if (fabsl(A[(size_t)a * W + p]) > fabsl(A[(size_t)best * W + p])) best = a;
        if (best != p) for (int b = 0; b < W; ++b) { const ld t = A[(size_t)p * W + b]; A[(size_t)p * W + b] = A[(size_t)best * W + b]; A[(size_t)best * W + b] = t; }
        for (int a = p + 1; a < k; ++a) {
            const ld f = A[(size_t)a * W + p] / A[(size_t)p * W + p];
            for (int b = p; b < W; ++b) A[(size_t)a * W + b] -= f * A[(size_t)p * W + b];
        }
    }
    std::vector<ld> x1(k), x2(k);                // S_oo^-1 S_oj and S_oo^-1 (u_o - m)
    for (int a = k - 1; a >= 0; --a) {
        ld s1 = A[(size_t)a * W + k], s2 = A[(size_t)a * W + k + 1];
        for (int b = a + 1; b < k; ++b) { s1 -= A[(size_t)a * W + b] * x1[b]; s2 -= A[(size_t)a * W + b] * x2[b]; }
        x1[a] = s1 / A[(size_t)a * W + a]; x2[a] = s2 / A[(size_t)a * W + a];
    }
    ld mean = m, var = sig[j] + v;
    for (int a = 0; a < k; ++a) { mean += v * x2[a]; var -= v * x1[a]; }
    return -(u[j] - mean) / sqrtl(var);
}

static void check_rt(int n, double v, double sig0, bool with_rho, unsigned seed)
{
    std::vector<double> sig(n), lam(n), t(n), rho(n);
    unsigned s = seed;
    auto rnd = [&]() { s = s * 1664525u + 1013904223u; return (double)(s >> 8) / 16777216.0; };
    for (int j = 0; j < n; ++j) { sig[j] = j == 0 ? sig0 : 0.1 + 0.5 * rnd(); lam[j] = 4.0 + 0.3 * (rnd() - 0.5); t[j] = 4.0 + 1.4 * (rnd() - 0.5); rho[j] = with_rho ? 0.6 * (rnd() - 0.5) : 0.0; }
    const double theta = 0.8, m0 = 0.2, m1 = -0.4, m = m0 + m1 * theta;
    MargSums ms{0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int j = 0; j < n; ++j) marg_sums_add(ms, 1.0 / sig[j], log(sig[j]), lam[j] - t[j], rho[j]);
    std::vector<ld> sl(n), ul(n);
    for (int j = 0; j < n; ++j) { sl[j] = (ld)sig[j]; ul[j] = (ld)lam[j] - (ld)rho[j] * (ld)theta - (ld)t[j]; }
    for (int j = 0; j < n; ++j) {
        const IfitRt cell = ifit_rt_prep(1.0 / sig[j], sig[j], lam[j] - t[j], rho[j], ms.P, v);
        const double d = ifit_rt_d(cell, v, ms.R0 - theta * ms.R1, m, theta);
        const ld ref = dense_d(n, j, sl.data(), ul.data(), (ld)m, (ld)v);
        // A forward bound: d = (m_ - u) / sd with m_ = (m + v (R - g u)) / Pi, and R is a sum that CONTAINS g u.  Every term carries a few ulp of its own size,
        // so the error is relative to (|m| + v sum_k g_k |u_k|) / (Pi sd) + |u| / sd -- with the definition's form an item of sig2t = 1e-8 (g = 1e8) pays for the
        // cancellation of its own g u -- or to |d| or 1 where those are larger.
        ld gu = 0.0L;
        for (int k = 0; k < n; ++k) gu += fabsl(ul[k]) / sl[k];
        const ld scale = fmaxl(fmaxl(fabsl(ref), 1.0L), ((fabsl((ld)m) + (ld)v * gu) * (ld)cell.ipi + fabsl(ul[j])) * (ld)cell.isd);
        const double err = (double)(fabsl((ld)d - ref) / scale);
        if (err > worst_d) worst_d = err;
        expect(err <= 2e-13 && std::isfinite(d), "ifit_rt_d against the dense conditional Gaussian", d, (double)ref);
    }
}

static void check_finish()
{
    double s[IFIT_SUMS] = {-3.0, 5.0, 4.0, 18.0, 6.0, 20.0, 16.0}, out[IFIT_COLS];
    ifit_finish(s, true, out);
    expect(out[IFIT_INFIT] == 1.25 && out[IFIT_OUTFIT] == 1.125 && out[IFIT_RESP_Z] == -1.5 && out[IFIT_RT_MSQ] == 1.25 && out[IFIT_RT_Z] == 1.5 && out[IFIT_N_OBS] == 16.0, "ifit_finish");
    ifit_finish(s, false, out);
    expect(out[IFIT_INFIT] == 1.25 && std::isnan(out[IFIT_RT_MSQ]) && std::isnan(out[IFIT_RT_Z]) && out[IFIT_N_OBS] == 16.0, "ifit_finish without times");
    double z[IFIT_SUMS] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    ifit_finish(z, true, out);
    bool all = true;
    for (int c = 0; c < IFIT_N_OBS; ++c) all = all && std::isnan(out[c]);
    expect(all && out[IFIT_N_OBS] == 0.0, "ifit_finish with n_j = 0");
}

static void check_reduce()
{
    expect(ifit_chunk(92949, 0) == 92928 && ifit_chunk(100, 0) == 256 && ifit_chunk(92949, 1) == 256 && ifit_chunk(92949, 256) == 256 && ifit_chunk(92949, 257) == 512 &&
           ifit_chunk(300, 100000) == 256 && ifit_blocks(1) == 1 && ifit_blocks(256) == 1 && ifit_blocks(257) == 2, "ifit_chunk / ifit_blocks");
    const long long Ns[6] = {1, 255, 256, 257, 600, 100000};
    const long long caps[6] = {0, 1, 256, 257, 1000, 65536};
    for (long long N : Ns) {
        std::vector<double> val((size_t)N);
        unsigned s = 12345u + (unsigned)N;
        for (auto& x : val) { s = s * 1664525u + 1013904223u; x = ((double)(s >> 8) / 16777216.0 - 0.3) * (1.0 + (double)(s & 1023u)); }
        ld exact = 0.0L;
        for (double x : val) exact += (ld)x;
        double first = 0.0;
        for (int c = 0; c < 6; ++c) {
            const int64_t chunk = ifit_chunk((int64_t)1 << 20, caps[c]);
            std::vector<int> seen((size_t)N, 0);
            const double got = ifit_reduce(N, chunk, [&](int64_t i) { return val[(size_t)i]; }, seen.data());
            bool once = true;
            for (int x : seen) once = once && x == 1;
            expect(once, "ifit_reduce: every subject once", (double)N, (double)caps[c]);
            if (c == 0) first = got;
            expect(memcmp(&got, &first, sizeof(double)) == 0, "ifit_reduce: the same bits at every cap", got, first);
            expect(rel(got, exact) <= 1e-12, "ifit_reduce against the long-double sum", got, (double)exact);
        }
    }
}

int main(int argc, char** argv)
{
    if (argc < 2 || strcmp(argv[1], "self") != 0) { printf("usage: ifit_check self\n"); return 2; }
    const double etas[6] = {0.0, 1e-300, 30.0, 699.0, 701.0, 1e4};
    for (double e : etas) for (int sgn = 0; sgn < 2; ++sgn) for (int y = 0; y < 2; ++y) check_resp(sgn ? -e : e, y != 0);
    for (int k = -4000; k <= 4000; ++k) for (int y = 0; y < 2; ++y) check_resp(0.01 * k + 0.003, y != 0);
    const int ns[4] = {1, 2, 7, 12};
    for (int n : ns) for (int rho = 0; rho < 2; ++rho) {
        check_rt(n, 0.35, 0.3, rho != 0, 7u + n);
        check_rt(n, 0.0, 0.3, rho != 0, 11u + n);                     // v = 0
        check_rt(n, 0.35, 1e-8, rho != 0, 13u + n);                   // sig2t = 1e-8
        check_rt(n, 4.0, 1e-8, rho != 0, 17u + n);
    }
    check_finish();
    check_reduce();
    printf("worst resp %.3g, worst d %.3g\n", worst_resp, worst_d);
    printf("failures %d\n", failures);
    return failures ? 1 : 0;
}

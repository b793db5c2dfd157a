// psis_check -- csrc/erm_psis.hpp on the CPU, compiled by tests/test_psis_host.py with -fsanitize=undefined.  The host walks a unit exactly as psis_kernel does
// (log ratios, the (key, position) order, the exceedances, psis_fit, psis_smooth), with plain in-order sums where the kernel has its lane-strided ones.
//   psis_check tail                      prints "S M G xstar" for every S in 25 .. 8192
//   psis_check unit  < values            reads S and then S values l_s; prints "M G khat sigma elpd" and then the S normalised smoothed log-weights in trace order
//   psis_check smooth M expc k sigma     prints psis_smooth(i, M, expc, k, sigma) for i = 1 .. M
// Numbers are printed as C99 hex floats: nothing is lost on the way to the test.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "erm_rankdiag.hpp"
#include "erm_psis.hpp"

using namespace erm;

static double lse(const std::vector<double>& v)
{
    double m = v[0];
    for (double x : v) if (x > m) m = x;
    double s = 0.0;
    for (double x : v) s += exp(x - m);
    return m + log(s);
}

static int unit()
{
    int S = 0;
    if (scanf("%d", &S) != 1 || S < PSIS_MIN_ROWS || S > PSIS_MAX_ROWS) { fprintf(stderr, "bad S\n"); return 2; }
    std::vector<double> l(S);
    for (int s = 0; s < S; ++s) if (scanf("%la", &l[s]) != 1) { fprintf(stderr, "bad value %d\n", s); return 2; }
    double mx = -l[0];
    for (int s = 1; s < S; ++s) if (-l[s] > mx) mx = -l[s];
    std::vector<uint64_t> key(S);
    std::vector<int> pos(S);
    for (int s = 0; s < S; ++s) { key[s] = rk_key(-l[s] - mx); pos[s] = s; }
    std::sort(pos.begin(), pos.end(), [&](int a, int b) { return key[a] < key[b] || (key[a] == key[b] && a < b); });
    const int M = psis_tail_len(S), G = psis_grid(M), T0 = S - M;
    const double c = psis_unkey(key[pos[T0 - 1]]), expc = exp(c);
    std::vector<double> x(M), L(PSIS_MAX_GRID, 0.0), b(PSIS_MAX_GRID, 0.0), lw(S), both(S);
    for (int i = 0; i < M; ++i) x[i] = exp(psis_unkey(key[pos[T0 + i]])) - expc;
    const PsisFit fit = psis_fit(x.data(), M, L.data(), b.data());
    for (int p = 0; p < S; ++p) lw[pos[p]] = (p < T0 || !fit.ok) ? psis_unkey(key[pos[p]]) : psis_smooth(p - T0 + 1, M, expc, fit.khat, fit.sigma);
    for (int s = 0; s < S; ++s) both[s] = lw[s] + l[s];
    const double norm = lse(lw);
    printf("%d %d %a %a %a\n", M, G, fit.khat, fit.ok ? fit.sigma : (double)NAN, lse(both) - norm);
    for (int s = 0; s < S; ++s) printf("%a\n", lw[s] - norm);
    return 0;
}

int main(int argc, char** argv)
{
    if (argc >= 2 && !strcmp(argv[1], "tail")) {
        for (int S = PSIS_MIN_ROWS; S <= PSIS_MAX_ROWS; ++S) { const int M = psis_tail_len(S); printf("%d %d %d %d\n", S, M, psis_grid(M), psis_xstar(M) + 1); }
        return 0;
    }
    if (argc >= 2 && !strcmp(argv[1], "unit")) return unit();
    if (argc >= 6 && !strcmp(argv[1], "smooth")) {
        const int M = atoi(argv[2]);
        const double expc = strtod(argv[3], nullptr), k = strtod(argv[4], nullptr), sigma = strtod(argv[5], nullptr);
        for (int i = 1; i <= M; ++i) printf("%a\n", psis_smooth(i, M, expc, k, sigma));
        return 0;
    }
    fprintf(stderr, "usage: psis_check tail | unit | smooth M expc k sigma\n");
    return 2;
}

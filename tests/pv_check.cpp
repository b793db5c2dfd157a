// pv_check -- csrc/erm_pv.hpp on the CPU, compiled by tests/test_pv_host.py with -fsanitize=undefined.
//   pv_check row K n_rows      prints pv_row(k, K, n_rows) for k = 0 .. K - 1
//   pv_check key w ...         prints pv_gumbel(w) for every 32-bit word given
//   pv_check merge < pairs     reads lines "keyA qA keyB qB" (q < 0: the empty pair); prints "key q key q": pv_best_merge(A, B) and pv_best_merge(B, A)
//   pv_check pick < keys       reads Q and then Q keys; deals the nodes to eight lanes as pv_kernel does (lane s takes s, s + 8, ... through pv_best_add), joins the
//                              lanes by the kernel's butterfly (partner = lane ^ 1, ^ 2, ^ 4) and prints the q every lane ends with (eight numbers)
//   pv_check finish < draws    reads lines "E V mu sd c0 c1 u q Q has_zeta w0 w1 w2"; prints "theta zeta" of pv_finish
// Doubles are read and printed as C99 hex floats: nothing is lost on the way to the test.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "erm_pv.hpp"

using namespace erm;

static int merge()
{
    double ka, kb;
    int qa, qb;
    while (scanf("%la %d %la %d", &ka, &qa, &kb, &qb) == 4) {
        const PvBest a{ka, qa}, b{kb, qb}, ab = pv_best_merge(a, b), ba = pv_best_merge(b, a);
        printf("%a %d %a %d\n", ab.key, ab.q, ba.key, ba.q);
    }
    return 0;
}

static int pick()
{
    int Q = 0;
    if (scanf("%d", &Q) != 1 || Q < 1) { fprintf(stderr, "bad Q\n"); return 2; }
    std::vector<double> key(Q);
    for (int q = 0; q < Q; ++q) if (scanf("%la", &key[q]) != 1) { fprintf(stderr, "bad key %d\n", q); return 2; }
    PvBest lane[8];
    for (int s = 0; s < 8; ++s) {
        lane[s] = PvBest{0.0, -1};
        for (int q = s; q < Q; q += 8) pv_best_add(lane[s], key[q], q);
    }
    for (int m = 1; m < 8; m <<= 1) {
        PvBest next[8];
        for (int s = 0; s < 8; ++s) next[s] = pv_best_merge(lane[s], lane[s ^ m]);
        for (int s = 0; s < 8; ++s) lane[s] = next[s];
    }
    for (int s = 0; s < 8; ++s) printf("%d%c", lane[s].q, s == 7 ? '\n' : ' ');
    return 0;
}

static int finish()
{
    double E, V, mu, sd, c0, c1, u;
    int q, Q, has_zeta;
    unsigned long w0, w1, w2;
    while (scanf("%la %la %la %la %la %la %la %d %d %d %lu %lu %lu", &E, &V, &mu, &sd, &c0, &c1, &u, &q, &Q, &has_zeta, &w0, &w1, &w2) == 13) {
        const ScoreRow r{E, V, 0.0, 0.0, 0.0, 0.0};
        const MargLaw w{mu, sd, 0.0, 0.0, 0.0};
        const PvDraw d = pv_finish(r, w, ScoreZeta{c0, c1, u}, q, marg_step(Q), has_zeta != 0, (uint32_t)w0, (uint32_t)w1, (uint32_t)w2);
        printf("%a %a\n", d.theta, d.zeta);
    }
    return 0;
}

int main(int argc, char** argv)
{
    if (argc == 4 && !strcmp(argv[1], "row")) {
        const long long K = atoll(argv[2]), n_rows = atoll(argv[3]);
        if (!pv_draws_ok(K) || n_rows < 1) { fprintf(stderr, "bad K / n_rows\n"); return 2; }
        for (long long k = 0; k < K; ++k) printf("%lld\n", pv_row(k, K, n_rows));
        return 0;
    }
    if (argc >= 3 && !strcmp(argv[1], "key")) {
        for (int a = 2; a < argc; ++a) printf("%a\n", pv_gumbel((uint32_t)strtoul(argv[a], nullptr, 10)));
        return 0;
    }
    if (argc == 2 && !strcmp(argv[1], "merge")) return merge();
    if (argc == 2 && !strcmp(argv[1], "pick")) return pick();
    if (argc == 2 && !strcmp(argv[1], "finish")) return finish();
    fprintf(stderr, "usage: pv_check row K n_rows | key w ... | merge | pick | finish\n");
    return 2;
}

// rankdiag_check -- the pure parts of the rank-normalised diagnostics (extendedrtirtmodeling.jl_amd/csrc/erm_rankdiag.hpp) on the CPU, built with
// g++ -fsanitize=undefined by tests/test_rankdiag_host.py.
//   rankdiag_check              self-checks: the key's order over special values and random pairs, the tie-run rank, the probability map, k and the padding
//   rankdiag_check rank v ...   prints the average rank of every value, found as the device finds it: sort (key, position), walk the tie runs
//   rankdiag_check key v        prints the key of v in hex
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <random>
#include <string>
#include <utility>
#include <vector>
#include "erm_rankdiag.hpp"

using namespace erm;

static int failures = 0;
#define EXPECT(cond, ...) do { if (!(cond)) { ++failures; if (failures <= 20) { printf("FAIL %s:%d: %s  ", __FILE__, __LINE__, #cond); printf(__VA_ARGS__); printf("\n"); } } } while (0)

static std::vector<double> avg_ranks(const std::vector<double>& x)
{
    const int S = (int)x.size();
    std::vector<std::pair<uint64_t, int>> kp(S);
    for (int i = 0; i < S; ++i) kp[i] = { rk_key(x[i]), i };
    std::sort(kp.begin(), kp.end());
    std::vector<double> r(S);
    for (int first = 0; first < S;) {
        int last = first;
        while (last + 1 < S && kp[last + 1].first == kp[first].first) ++last;
        for (int p = first; p <= last; ++p) r[kp[p].second] = rk_avg_rank(first, last);
        first = last + 1;
    }
    return r;
}

int main(int argc, char** argv)
{
    if (argc >= 3 && std::string(argv[1]) == "rank") {
        std::vector<double> x;
        for (int a = 2; a < argc; ++a) x.push_back(strtod(argv[a], nullptr));
        for (double r : avg_ranks(x)) printf("%.17g\n", r);
        return 0;
    }
    if (argc == 3 && std::string(argv[1]) == "key") { printf("%016llx\n", (unsigned long long)rk_key(strtod(argv[2], nullptr))); return 0; }

    // the key over the special values, in order
    const double inf = std::numeric_limits<double>::infinity(), dmin = std::numeric_limits<double>::denorm_min();
    const double ladder[] = { -inf, -DBL_MAX, -1e300, -2.0, -1.0 - DBL_EPSILON, -1.0, -DBL_MIN, -dmin, 0.0, dmin, DBL_MIN, 1.0, 1.0 + DBL_EPSILON, 2.0, 1e300, DBL_MAX, inf };
    const int nl = (int)(sizeof(ladder) / sizeof(ladder[0]));
    for (int i = 0; i + 1 < nl; ++i) EXPECT(rk_key(ladder[i]) < rk_key(ladder[i + 1]), "ladder %d: %g %g", i, ladder[i], ladder[i + 1]);
    EXPECT(rk_key(-0.0) == rk_key(0.0), "the zeros must tie");
    EXPECT(rk_key(-dmin) < rk_key(-0.0) && rk_key(-0.0) < rk_key(dmin), "zero between the smallest subnormals");
    EXPECT(rk_key(inf) < ~0ull, "the padding key must stay above +inf");
    // ... and over random pairs of every magnitude and sign, neighbours included
    std::mt19937_64 gen(20240607);
    for (int it = 0; it < 2000000; ++it) {
        uint64_t ba = gen(), bb = (it & 3) == 0 ? ba + (gen() % 5) - 2 : gen();
        double a, b;
        memcpy(&a, &ba, 8); memcpy(&b, &bb, 8);
        if (a != a || b != b) continue;
        EXPECT((a < b) == (rk_key(a) < rk_key(b)) && (a == b) == (rk_key(a) == rk_key(b)), "pair %a %a", a, b);
    }
    // the average rank of a tie run is the mean of its 1-based positions
    for (long long first = 0; first < 300; ++first) for (long long last = first; last < first + 300; last += 7) {
        long double s = 0;
        for (long long p = first; p <= last; ++p) s += (long double)(p + 1);
        EXPECT((long double)rk_avg_rank(first, last) == s / (long double)(last - first + 1), "run %lld %lld", first, last);
    }
    EXPECT(rk_avg_rank(0, 8191) == 4096.5 && rk_avg_rank(8191, 8191) == 8192.0, "ends of the longest column");
    // rank -> probability: inside (0, 1), increasing, symmetric about 1/2, the stated three operations
    for (long long S = 2; S <= 8192; S += (S < 64 ? 1 : 61)) {
        double prev = 0.0;
        for (long long r2 = 2; r2 <= 2 * S; ++r2) {                 // half-integer ranks
            const double r = 0.5 * (double)r2, p = rk_prob(r, S);
            EXPECT(p > prev && p < 1.0, "S %lld r %g p %g", S, r, p);
            EXPECT(p == (r - 0.375) / ((double)S + 0.25), "S %lld r %g", S, r);
            EXPECT(fabs(p + rk_prob((double)S + 1.0 - r, S) - 1.0) <= 4 * DBL_EPSILON, "symmetry S %lld r %g", S, r);
            prev = p;
        }
    }
    // k = ceil(S / 20) and the padding
    for (long long S = 1; S <= 100000; ++S) {
        const long long k = rk_tail_k(S);
        EXPECT(20 * k >= S && 20 * (k - 1) < S, "k of %lld", S);
    }
    EXPECT(rk_tail_k(8) == 1 && rk_tail_k(20) == 1 && rk_tail_k(21) == 2 && rk_tail_k(8192) == 410, "known k");
    for (int S = 1; S <= RK_MAX_DRAWS; ++S) { const int P = rk_pad(S); EXPECT(P >= S && (P & (P - 1)) == 0 && (P == 1 || P / 2 < S), "pad of %d", S); }
    EXPECT(RK_MAX_DRAWS >= 8192, "the cap");
    // ranks of a column with every kind of tie
    {
        const std::vector<double> x = { 3.0, -0.0, 1.0, 0.0, 3.0, -inf, 3.0, inf };
        const double want[] = { 6.0, 2.5, 4.0, 2.5, 6.0, 1.0, 6.0, 8.0 };
        const std::vector<double> r = avg_ranks(x);
        for (size_t i = 0; i < x.size(); ++i) EXPECT(r[i] == want[i], "rank %zu: %g", i, r[i]);
    }
    printf("failures %d\n", failures);
    return failures ? 1 : 0;
}

// csrc/erm_obs.hpp on the CPU, driven by tests/test_obs_host.py (built with g++ -fsanitize=undefined -ftrapv):
//   obs_check FILE    FILE holds int64 N, int64 J, int64 rt, then obs [J][N] uint8, Y [J][N] uint8 (both column-major [N][J]) and, if rt, logT [J][N] double.
//                     Prints "status bad" of obs_offsets; if that passed, "status bad" of obs_compact; if that passed too, the lines "off ...", "idx ...", "y ..."
//                     and "t ..." (the log-times as hex floats: every bit).
// The unobserved cells of Y and logT in FILE are the caller's poison: the header must not read them.
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "erm_obs.hpp"

using namespace erm;

int main(int argc, char** argv)
{
    if (argc != 2) { fprintf(stderr, "usage: obs_check FILE\n"); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    int64_t head[3];
    if (fread(head, sizeof(int64_t), 3, f) != 3) return 2;
    const int64_t N = head[0]; const int J = (int)head[1]; const bool rt = head[2] != 0;
    if (N <= 0 || J <= 0 || J > OBS_MAX_ITEMS) return 2;
    const size_t NJ = (size_t)N * (size_t)J;
    std::vector<uint8_t> obs(NJ), Y(NJ);
    std::vector<double> logT(rt ? NJ : 0);
    if (fread(obs.data(), 1, NJ, f) != NJ || fread(Y.data(), 1, NJ, f) != NJ) return 2;
    if (rt && fread(logT.data(), sizeof(double), NJ, f) != NJ) return 2;
    fclose(f);

    std::vector<int64_t> off((size_t)N + 1), cur((size_t)N);
    int64_t bad = -1;
    int st = obs_offsets(obs.data(), N, J, off.data(), &bad);
    printf("%d %lld\n", st, (long long)bad);
    if (st != OBS_OK) return 0;
    const size_t total = (size_t)off[(size_t)N];
    std::vector<uint16_t> idx(total);
    std::vector<uint8_t> y(total);
    std::vector<double> t(rt ? total : 0);
    bad = -1;
    st = obs_compact(Y.data(), rt ? logT.data() : nullptr, obs.data(), N, J, off.data(), cur.data(), idx.data(), y.data(), rt ? t.data() : nullptr, &bad);
    printf("%d %lld\n", st, (long long)bad);
    if (st != OBS_OK) return 0;
    printf("off"); for (int64_t v : off) printf(" %lld", (long long)v); printf("\n");
    printf("idx"); for (uint16_t v : idx) printf(" %u", (unsigned)v); printf("\n");
    printf("y"); for (uint8_t v : y) printf(" %u", (unsigned)v); printf("\n");
    printf("t"); for (double v : t) printf(" %a", v); printf("\n");
    return 0;
}

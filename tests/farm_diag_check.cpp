// farm_diag_check -- the chunk arithmetic of the chain farm's joint diagnostics (extendedrtirtmodeling.jl_amd/csrc/erm_farm_diag.hpp) on the CPU, built with
// g++ -fsanitize=undefined by tests/test_farm_diag_host.py.
//   farm_diag_check                              self-checks over the sweep below: the chunks cover every column exactly once and in order, none exceeds the
//                                                budget unless a single column does, none exceeds the cap, and the byte counts do not overflow
//   farm_diag_check ncol Tn L elem budget cap    prints "chunk count" and then every chunk "c0 nc" (at most the first and last 1000 of a long list)
#include <cstdio>
#include <cstdlib>
#include "erm_farm_diag.hpp"

using namespace erm;

static int failures = 0;
#define EXPECT(cond, ...) do { if (!(cond)) { ++failures; if (failures <= 20) { printf("FAIL %s:%d: %s  ", __FILE__, __LINE__, #cond); printf(__VA_ARGS__); printf("\n"); } } } while (0)

static void check_plan(int64_t ncol, int64_t Tn, int64_t L, int64_t elem, int64_t budget, int64_t cap)
{
    const FarmDiagChunks P = farm_diag_chunks(ncol, Tn, L, elem, budget, cap);
    const int64_t n = P.count(), one = farm_diag_bytes(1, Tn, L, elem);
#define CASE "ncol %lld Tn %lld L %lld elem %lld budget %lld cap %lld", (long long)ncol, (long long)Tn, (long long)L, (long long)elem, (long long)budget, (long long)cap
    EXPECT(P.chunk >= 1 && P.chunk <= ncol, CASE);
    EXPECT(cap <= 0 || P.chunk <= cap, CASE);
    EXPECT(one == Tn * L * elem, CASE);
    EXPECT(farm_diag_bytes(P.chunk, Tn, L, elem) <= budget || (P.chunk == 1 && one > budget), CASE);
    EXPECT(P.chunk < 4 || P.chunk % 4 == 0 || P.chunk == ncol, CASE);      // rounded to a multiple of four only where more chunks follow
    // the longest chunk the budget and the cap allow, up to the rounding to a multiple of four
    const int64_t more = P.chunk + (P.chunk >= 4 ? 4 : 1);      // (a block of ncol columns that fits whole is taken whole: the first disjunct below)
    EXPECT(P.chunk == ncol || (cap > 0 && more > cap) || farm_diag_bytes(more, Tn, L, elem) > budget || more > ncol, CASE);
    EXPECT(n >= 1 && (n - 1) * P.chunk < ncol && ncol <= n * P.chunk, CASE);
    // coverage: chunk i starts where chunk i - 1 ended, the first at column 0, the last ends at ncol; every chunk but the last has the full length.  A list of more
    // than two million chunks is walked at both ends and at a stride in between (the chunks are an arithmetic progression: at() is one multiplication).
    const int64_t stride = n > 2000000 ? n / 100003 : 1;
    int64_t next = 0, walked = 0;
    auto after = [&](int64_t i) { return (i < 1000 || i + 1000 >= n) ? i + 1 : (i + stride + 1000 >= n ? n - 1000 : i + stride); };
    for (int64_t i = 0; i < n; i = after(i)) {
        const FarmDiagChunk c = P.at(i);
        if (stride == 1 || i == 0) EXPECT(c.c0 == next, CASE);
        EXPECT(c.c0 == i * P.chunk && c.nc >= 1 && c.c0 + c.nc <= ncol, CASE);
        EXPECT(i == n - 1 ? c.c0 + c.nc == ncol : c.nc == P.chunk, CASE);
        EXPECT(farm_diag_bytes(c.nc, Tn, L, elem) <= budget || c.nc == 1, CASE);
        next = c.c0 + c.nc;
        ++walked;
    }
    EXPECT(next == ncol && walked >= 1, CASE);
#undef CASE
}

int main(int argc, char** argv)
{
    if (argc == 7) {
        const int64_t a[6] = { atoll(argv[1]), atoll(argv[2]), atoll(argv[3]), atoll(argv[4]), atoll(argv[5]), atoll(argv[6]) };
        const FarmDiagChunks P = farm_diag_chunks(a[0], a[1], a[2], a[3], a[4], a[5]);
        printf("%lld %lld\n", (long long)P.chunk, (long long)P.count());
        for (int64_t i = 0; i < P.count(); ++i) {
            if (i >= 1000 && i + 1000 < P.count()) { i = P.count() - 1001; continue; }
            printf("%lld %lld\n", (long long)P.at(i).c0, (long long)P.at(i).nc);
        }
        return 0;
    }
    const int64_t ncols[] = { 1, 31, 32, 33, 316, 100000000 }, Ls[] = { 1, 2, 16 }, Tns[] = { 8, 9, 8192 / 2 }, elems[] = { 4, 8 }, caps[] = { 0, 1, 100 };
    // the library's budget, one that a few columns fill, one that not even one column fits, and the largest int64
    const int64_t budgets[] = { FARM_DIAG_BUDGET, 4096, 16, FARM_DIAG_I64_MAX };
    long long plans = 0;
    for (int64_t ncol : ncols) for (int64_t L : Ls) for (int64_t Tn : Tns) for (int64_t elem : elems) for (int64_t cap : caps) for (int64_t budget : budgets) {
        check_plan(ncol, Tn, L, elem, budget, cap);
        ++plans;
    }
    // saturation instead of overflow
    EXPECT(farm_diag_bytes(FARM_DIAG_I64_MAX, 4096, 16, 8) == FARM_DIAG_I64_MAX, "saturated product");
    EXPECT(farm_diag_bytes(100000000, 4096, 16, 8) == 52428800000000ll, "1e8 columns of 16 chains: 5.2e13 bytes");
    EXPECT(farm_diag_bytes(0, 8, 1, 4) == 0, "no columns");
    // known plans: 316 float columns of 3 chains x 20 rows under a cap of 100 -> 100, 100, 100, 16;  1e8 double columns of 16 chains x 4096 rows -> 512 columns a chunk
    {
        const FarmDiagChunks P = farm_diag_chunks(316, 20, 3, 4, FARM_DIAG_BUDGET, 100);
        EXPECT(P.chunk == 100 && P.count() == 4 && P.at(3).c0 == 300 && P.at(3).nc == 16, "316 under a cap of 100");
        const FarmDiagChunks Q = farm_diag_chunks(100000000, 4096, 16, 8, FARM_DIAG_BUDGET, 0);
        EXPECT(Q.chunk == 512 && Q.count() == 195313 && Q.at(195312).nc == 100000000 - 195312ll * 512, "1e8 columns");
        const FarmDiagChunks R = farm_diag_chunks(33, 9, 2, 8, 16, 0);
        EXPECT(R.chunk == 1 && R.count() == 33, "a budget below one column: one column a chunk");
        const FarmDiagChunks W = farm_diag_chunks(100001, 50, 4, 8, FARM_DIAG_BUDGET, 0);
        EXPECT(W.chunk == 100001 && W.count() == 1 && W.at(0).nc == 100001, "a block that fits is one chunk, whatever its width");
        const FarmDiagChunks V = farm_diag_chunks(302, 20, 3, 4, FARM_DIAG_BUDGET, 301);
        EXPECT(V.chunk == 300 && V.count() == 2 && V.at(1).c0 == 300 && V.at(1).nc == 2, "more chunks follow: a multiple of four");
    }
    printf("plans %lld failures %d\n", plans, failures);
    return failures ? 1 : 0;
}

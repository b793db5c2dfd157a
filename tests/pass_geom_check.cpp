// tests/pass_geom_check.cpp -- CPU sweep of pass_geom (extendedrtirtmodeling.jl_amd/csrc/erm_geometry.hpp): the launch geometry of the passes behind a sweep
// (pointwise_kernel, predictive_kernel, predictive_items_kernel) and of DIC's loglik_kernel.  Built by tests/test_pass_geometry_host.py with
// g++ -fsanitize=undefined -fno-sanitize-recover -ftrapv.  For every plan it REPLAYS the kernels' index loops on the host -- the loops are restated here from the
// kernels, with the plan's numbers as the only input -- and requires: every subject (every cell) visited exactly once, idle slots inside the data set, W * R == T
// with T a multiple of 64, an LDS request of at most 160 KB that holds every index the kernel forms, a slab of nb rows written and read, every workgroup range of
// loglik_kernel inside [0, N], and the 16 parts of the item kernel a partition of [0, nb).
//   (no arguments)                  the sweep: N in 1 ... 10 000 and a few large values, J in 1 ... 896, compute units 1 / 64 / 256 / 304
//   case <model> <N> <J> <cus>      one plan as key=value pairs
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <utility>
#include <vector>
#include "erm_geometry.hpp"

using namespace erm;

static long long fails = 0, n_plans = 0, n_replays = 0;
#define REQUIRE(cond, ...) do { if (!(cond)) { if (fails++ < 20) { fprintf(stderr, "FAIL %s: ", #cond); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); } } } while (0)

// ---- O(1) properties of a plan
static void check_plan(int model, long long N, int J, int cu, const PassGeom& g)
{
    ++n_plans;
    const int W = 1 << g.logW;
    REQUIRE(g.logW >= 0 && g.logW <= 6 && (W >= J || 4 * W >= J || W == 64) && (g.logW == 0 || 4 * (W / 2) < J), "J %d: logW %d", J, g.logW);
    REQUIRE(g.T % 64 == 0 && g.T >= 64 && g.T <= PASS_THREADS && W * g.R == g.T && g.R >= 1, "model %d J %d: T %d W %d R %d", model, J, g.T, W, g.R);
    REQUIRE(W * g.R_pw == PASS_THREADS, "J %d: W %d R_pw %d", J, W, g.R_pw);
    REQUIRE(g.nq == (model == MLIRT ? 3 : 5), "model %d nq %d", model, g.nq);
    REQUIRE(g.lds_pred <= LDS_LIMIT && g.lds_pred == ((size_t)6 * J + (size_t)g.R * g.nq * J) * 8, "model %d J %d: lds_pred %zu", model, J, g.lds_pred);
    REQUIRE(g.T == PASS_THREADS || pred_lds_bytes(model, J, 2 * g.T, g.logW) > LDS_LIMIT, "model %d J %d: T %d halved without need", model, J, g.T);
    REQUIRE(g.lds_pw == (size_t)7 * J * 8 && g.lds_pw <= 64 * 1024 && g.lds_loglik <= 64 * 1024, "J %d: lds_pw %zu lds_loglik %zu", J, g.lds_pw, g.lds_loglik);
    REQUIRE(g.nb_pred >= 1 && g.nb_pred <= PRED_MAX_BLOCKS && ((long long)g.nb_pred - 1) * g.R < N, "N %lld J %d: nb_pred %d R %d", N, J, g.nb_pred, g.R);
    REQUIRE(g.nb_pred == PRED_MAX_BLOCKS || (long long)g.nb_pred * g.R >= N, "N %lld J %d: nb_pred %d below its cap does not cover N", N, J, g.nb_pred);
    REQUIRE(g.nb_pw_subject >= 1 && g.nb_pw_subject <= 8LL * cu && ((long long)g.nb_pw_subject - 1) * g.R_pw < N, "N %lld J %d cu %d: nb_pw_subject %d", N, J, cu, g.nb_pw_subject);
    REQUIRE(g.nb_pw_subject == 8LL * cu || (long long)g.nb_pw_subject * g.R_pw >= N, "N %lld J %d cu %d: nb_pw_subject %d below its cap does not cover N", N, J, cu, g.nb_pw_subject);
    REQUIRE(g.nb_pw_cell >= 1 && g.nb_pw_cell <= 16LL * cu && ((long long)g.nb_pw_cell - 1) * PASS_THREADS < N * J, "N %lld J %d cu %d: nb_pw_cell %d", N, J, cu, g.nb_pw_cell);
    REQUIRE(g.nb_pw_cell == 16LL * cu || (long long)g.nb_pw_cell * PASS_THREADS >= N * J, "N %lld J %d cu %d: nb_pw_cell %d below its cap does not cover the cells", N, J, cu, g.nb_pw_cell);
    REQUIRE(g.nb_loglik >= 1 && g.nb_loglik <= LOGLIK_MAX_BLOCKS && g.rows_per_block >= 1 && g.rows_per_block * g.nb_loglik >= N, "N %lld: nb_loglik %d rows_per_block %lld", N, g.nb_loglik, g.rows_per_block);
}

// ---- predictive_kernel / pointwise_kernel<PW_SUBJECT>: `for (i0 = blockIdx.x * R; i0 < N; i0 += gridDim.x * R)`, slot r takes subject i0 + r when that is < N
// and repeats subject N - 1 otherwise.  By chunks of R subjects: every chunk taken once, by one workgroup; the idle slots of the last chunk stay inside [0, N).
static void replay_subject_chunks(const char* what, long long N, int R, int nb, std::vector<unsigned char>& seen)
{
    ++n_replays;
    const long long nchunk = (N + R - 1) / R;
    seen.assign((size_t)nchunk, 0);
    long long subjects = 0;
    for (int b = 0; b < nb; ++b)
        for (long long i0 = (long long)b * R; i0 < N; i0 += (long long)nb * R) {
            REQUIRE(i0 % R == 0 && i0 / R < nchunk && !seen[(size_t)(i0 / R)], "%s N %lld R %d nb %d: chunk at %lld taken twice", what, N, R, nb, i0);
            seen[(size_t)(i0 / R)] = 1;
            for (int r : {0, R - 1}) {                          // the first and the last slot of the chunk (the slots between them lie between their subjects)
                const bool ok = i0 + r < N;
                const long long i = ok ? i0 + r : N - 1;
                REQUIRE(i >= 0 && i < N, "%s N %lld R %d: slot %d reads subject %lld", what, N, R, r, i);
            }
            subjects += (i0 + R <= N) ? R : N - i0;
        }
    REQUIRE(subjects == N, "%s N %lld R %d nb %d: %lld subjects updated", what, N, R, nb, subjects);
    for (long long c = 0; c < nchunk; ++c) REQUIRE(seen[(size_t)c], "%s N %lld R %d nb %d: chunk %lld never taken", what, N, R, nb, c);
}

// ---- the same loops thread by thread, at small sizes: every (subject, item) added once by an `ok` lane, every LDS index inside the request, the butterfly's
// partners inside the subject's lanes.  T threads, dynamic LDS of lds_doubles doubles of which the first 6 J are the item parameters (replicate pass only).
static void replay_lanes(const char* what, long long N, int J, int logW, int T, int nb, int nq, size_t lds_doubles, std::vector<unsigned char>& cell)
{
    ++n_replays;
    const int W = 1 << logW, R = T >> logW;
    cell.assign((size_t)(N * J), 0);
    std::vector<int> updates((size_t)N, 0);
    for (int b = 0; b < nb; ++b)
        for (long long i0 = (long long)b * R; i0 < N; i0 += (long long)nb * R)
            for (int tid = 0; tid < T; ++tid) {
                const int s = tid & (W - 1), r = tid >> logW;
                const bool ok = i0 + r < N;
                const long long i = ok ? i0 + r : N - 1;
                REQUIRE(i >= 0 && i < N && r < R, "%s N %lld J %d: thread %d reads subject %lld (slot %d of %d)", what, N, J, tid, i, r, R);
                for (int j = s; j < J; j += W) {
                    if (nq) REQUIRE((size_t)6 * J + (size_t)r * nq * J + (size_t)(nq - 1) * J + j < lds_doubles, "%s N %lld J %d: LDS index of slot %d item %d beyond %zu doubles", what, N, J, r, j, lds_doubles);
                    if (ok) { REQUIRE(!cell[(size_t)(i * J + j)], "%s N %lld J %d: cell (%lld, %d) added twice", what, N, J, i, j); cell[(size_t)(i * J + j)] = 1; }
                }
                for (int m = 1; m < W; m <<= 1) REQUIRE(((tid ^ m) >> logW) == r && (tid ^ m) < T && ((tid ^ m) >> 6) == (tid >> 6), "%s J %d: butterfly partner of thread %d at %d leaves the subject", what, J, tid, m);
                if (ok && s == 0) ++updates[(size_t)i];
            }
    for (long long e = 0; e < N * J; ++e) REQUIRE(cell[(size_t)e], "%s N %lld J %d: cell %lld never added", what, N, J, e);
    for (long long i = 0; i < N; ++i) REQUIRE(updates[(size_t)i] == 1, "%s N %lld J %d: subject %lld updated %d times", what, N, J, i, updates[(size_t)i]);
}

// ---- pointwise_kernel<PW_CELL>: `for (e = blockIdx.x * 256 + tid; e < N J; e += gridDim.x * 256)`, i = e / J, j = e - i J.  By chunks of 256 cells.
static void replay_cell_chunks(long long N, int J, int nb, std::vector<unsigned char>& seen)
{
    ++n_replays;
    const long long NJ = N * J, nchunk = (NJ + PASS_THREADS - 1) / PASS_THREADS;
    seen.assign((size_t)nchunk, 0);
    long long cells = 0;
    for (int b = 0; b < nb; ++b)
        for (long long e0 = (long long)b * PASS_THREADS; e0 < NJ; e0 += (long long)nb * PASS_THREADS) {
            REQUIRE(!seen[(size_t)(e0 / PASS_THREADS)], "cell unit N %lld J %d nb %d: chunk at %lld taken twice", N, J, nb, e0);
            seen[(size_t)(e0 / PASS_THREADS)] = 1;
            const long long last = (e0 + PASS_THREADS <= NJ ? e0 + PASS_THREADS : NJ) - 1;
            for (long long e : {e0, last}) {
                const long long i = e / J; const int j = (int)(e - i * J);
                REQUIRE(i >= 0 && i < N && j >= 0 && j < J && i * J + j == e, "cell unit N %lld J %d: cell %lld -> (%lld, %d)", N, J, e, i, j);
            }
            cells += last - e0 + 1;
        }
    REQUIRE(cells == NJ, "cell unit N %lld J %d nb %d: %lld cells updated", N, J, nb, cells);
    for (long long c = 0; c < nchunk; ++c) REQUIRE(seen[(size_t)c], "cell unit N %lld J %d nb %d: chunk %lld never taken", N, J, nb, c);
}

// ---- loglik_kernel: workgroup b owns subjects [r0, r1), r0 = b rows_per_block, r1 = min(r0 + rows_per_block, N); a workgroup past the end owns none.
// Cell c of its range is (r0 + c / J, c % J); with `cells` the (subject, item) pairs are replayed one by one.
static void replay_loglik(long long N, int J, int nb, long long rpb, bool cells)
{
    ++n_replays;
    long long next = 0;
    for (int b = 0; b < nb; ++b) {
        const long long r0 = (long long)b * rpb, r1 = (r0 + rpb < N) ? r0 + rpb : N;
        const long long rows = r1 > r0 ? r1 - r0 : 0;
        if (rows == 0) { REQUIRE(next == N, "loglik N %lld nb %d: workgroup %d is empty before the end", N, nb, b); continue; }
        REQUIRE(r0 == next && r0 >= 0 && r1 <= N, "loglik N %lld nb %d rows_per_block %lld: workgroup %d owns [%lld, %lld), expected to start at %lld", N, nb, rpb, b, r0, r1, next);
        next = r1;
        if (cells) {
            long long want_i = r0; int want_j = 0;
            for (long long c = 0; c < rows * J; ++c) {
                const long long i = r0 + c / J; const int j = (int)(c % J);
                REQUIRE(i == want_i && j == want_j && i < r1, "loglik N %lld J %d: cell %lld of workgroup %d -> (%lld, %d)", N, J, c, b, i, j);
                if (++want_j == J) { want_j = 0; ++want_i; }
            }
        }
    }
    REQUIRE(next == N, "loglik N %lld nb %d rows_per_block %lld: subjects up to %lld owned", N, nb, rpb, next);
}

// ---- predictive_items_kernel: part p (of 16) adds slab rows [p per, min(nb, p per + per)), per = ceil(nb / 16); lane l of the trip at j0 takes item j0 + l
static void replay_items(int nb, int J)
{
    ++n_replays;
    const int per = (nb + PRED_IT_PARTS - 1) / PRED_IT_PARTS;
    int next = 0;
    for (int part = 0; part < PRED_IT_PARTS; ++part) {
        const int b0 = part * per, b1 = std::min(nb, b0 + per);
        for (int b = b0; b < b1; ++b) { REQUIRE(b == next && b < nb, "item step nb %d: part %d reads row %d, expected %d", nb, part, b, next); ++next; }
    }
    REQUIRE(next == nb, "item step nb %d: %d rows read", nb, next);
    int items = 0;
    for (int j0 = 0; j0 < J; j0 += 64) for (int lane = 0; lane < 64; ++lane) { const int j = j0 + lane; if (j < J) { REQUIRE(j == items, "item step J %d: item %d out of order", J, j); ++items; } }
    REQUIRE(items == J, "item step J %d: %d items updated", J, items);
}

int main(int argc, char** argv)
{
    if (argc == 6 && !strcmp(argv[1], "case")) {
        const int model = atoi(argv[2]); const long long N = atoll(argv[3]); const int J = atoi(argv[4]), cu = atoi(argv[5]);
        if (model < MLIRT || model > LATENT || N < 1 || J < 1 || J > MAX_ITEMS || cu < 1) { printf("error=bad case\n"); return 0; }
        const PassGeom g = pass_geom(model, N, J, cu);
        check_plan(model, N, J, cu, g);
        printf("logW=%d T=%d R=%d nq=%d nb_pred=%d lds_pred=%zu R_pw=%d nb_pw_subject=%d nb_pw_cell=%d lds_pw=%zu nb_loglik=%d rows_per_block=%lld lds_loglik=%zu\n", g.logW, g.T, g.R, g.nq, g.nb_pred,
               g.lds_pred, g.R_pw, g.nb_pw_subject, g.nb_pw_cell, g.lds_pw, g.nb_loglik, g.rows_per_block, g.lds_loglik);
        return fails ? 1 : 0;
    }
    std::vector<long long> Ns;
    for (long long N = 1; N <= 10000; ++N) Ns.push_back(N);
    for (long long N : {16383LL, 16384LL, 16385LL, 65535LL, 65536LL, 65537LL, 100000LL, 262143LL, 262145LL, 1000003LL, 4194304LL}) Ns.push_back(N);
    static const int CUs[] = {1, 64, 256, 304};
    static const int MODELS2[] = {MLIRT, RTIRT};                // the two slab widths; the other five models plan as RTIRT does (checked below)
    std::vector<unsigned char> seen;
    // 1. every plan's own properties; the distinct (R, nb) of the subject loops and the distinct loglik plans are collected per N and replayed once each
    for (long long N : Ns) {
        std::set<std::pair<int, int>> pred, pws;
        std::set<std::pair<int, long long>> lls;
        for (int model : MODELS2)
            for (int cu : CUs) {
                PassGeom last;
                last.R = 0;
                for (int J = 1; J <= MAX_ITEMS; ++J) {
                    const PassGeom g = pass_geom(model, N, J, cu);
                    check_plan(model, N, J, cu, g);
                    if (g.R == last.R && g.nb_pred == last.nb_pred && g.R_pw == last.R_pw && g.nb_pw_subject == last.nb_pw_subject) continue;      // (neighbouring J mostly share their loops)
                    pred.insert({g.R, g.nb_pred}); pws.insert({g.R_pw, g.nb_pw_subject}); lls.insert({g.nb_loglik, g.rows_per_block});
                    last = g;
                }
            }
        for (auto& p : pred) replay_subject_chunks("replicate pass", N, p.first, p.second, seen);
        for (auto& p : pws) replay_subject_chunks("WAIC subject unit", N, p.first, p.second, seen);
        for (auto& p : lls) replay_loglik(N, 1, p.first, p.second, false);
    }
    for (int model = MLIRT; model <= LATENT; ++model)
        for (int J : {1, 5, 129, 787, 788, 896}) {
            const PassGeom a = pass_geom(model, 1000, J, 256), b = pass_geom(model == MLIRT ? MLIRT : RTIRT, 1000, J, 256);
            REQUIRE(a.T == b.T && a.nq == b.nq && a.lds_pred == b.lds_pred && a.nb_pred == b.nb_pred, "model %d J %d plans unlike its slab-width class", model, J);
        }
    // 2. the cell unit by chunks: every J at small and marked N, every N at marked J
    static const int Jmark[] = {1, 3, 50, 129};
    for (long long N : Ns) {
        const bool markedN = N <= 64 || N == 4096 || N == 4101 || N == 8197 || N == 9733 || N == 10000;
        if (N > 300000) continue;
        for (int cu : CUs) {
            if (markedN) for (int J = 1; J <= MAX_ITEMS; ++J) replay_cell_chunks(N, J, pass_geom(RTIRT, N, J, cu).nb_pw_cell, seen);
            else for (int J : Jmark) replay_cell_chunks(N, J, pass_geom(RTIRT, N, J, cu).nb_pw_cell, seen);
        }
    }
    // 3. thread by thread at small sizes: the lane widths and their switches, the LDS edge of the replicate pass, one compute unit (every cap exceeded early)
    static const int Jlanes[] = {1, 2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 64, 65, 128, 129, 257, 787, 788, 896};
    for (int J : Jlanes)
        for (int model : MODELS2) {
            const int R0 = pass_geom(model, 1, J, 1).R, Rp = pass_geom(model, 1, J, 1).R_pw;
            std::set<long long> small = {1, 2, 3, R0 - 1, R0, R0 + 1, 2LL * R0 + 1, Rp - 1, Rp, Rp + 1, 8LL * Rp + 5, 67};
            if (J <= 129) small.insert({1024LL * R0 + 5, 4101});
            for (long long N : small) {
                if (N < 1) continue;
                const PassGeom g = pass_geom(model, N, J, 1);
                replay_lanes("replicate pass", N, J, g.logW, g.T, g.nb_pred, g.nq, g.lds_pred / 8, seen);
                replay_lanes("WAIC subject unit", N, J, g.logW, PASS_THREADS, g.nb_pw_subject, 0, 0, seen);
                if (N * J <= 200000) replay_loglik(N, J, g.nb_loglik, g.rows_per_block, true);
            }
        }
    // 4. the item step: every slab height, every item count
    for (int nb = 1; nb <= PRED_MAX_BLOCKS; ++nb) replay_items(nb, nb <= MAX_ITEMS ? nb : MAX_ITEMS);
    for (int J = 1; J <= MAX_ITEMS; ++J) replay_items(17, J);
    printf("plans %lld, replays %lld, invariant failures %lld\n", n_plans, n_replays, fails);
    return fails ? 1 : 0;
}

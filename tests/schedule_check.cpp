// tests/schedule_check.cpp -- CPU sweep of the erm_run planner and its executor loop (extendedrtirtmodeling.jl_amd/csrc/erm_schedule.hpp).
// Built by tests/test_run_schedule.py with g++ -fsanitize=undefined -fno-sanitize-recover -ftrapv.  Every plan of every input Engine::run_checked can
// produce is checked against the rules in the header's first comment and driven through run_steps() -- the loop the engine runs -- on an executor of
// counters, once with no graph built and once with all of them; the timed-sweep count (erm_timing.pass_launches) must equal a closed form read off the
// schedule code this planner replaced (the `was:` notes quote it).  With `case <nsweeps> <cq> <fused> <persist> <shard> <no_graph> <profile>
// <stats_valid> <calibrate> [graph_sweeps]` it prints one plan and its counts.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include "erm_schedule.hpp"

using namespace erm;

static int fails = 0;
static long long n_plans = 0, n_executed = 0;
#define REQUIRE(cond, ...) do { if (!(cond)) { if (fails++ < 20) { fprintf(stderr, "FAIL %s: ", #cond); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); } } } while (0)

static std::string describe(const RunIn& in)
{
    char b[200];
    snprintf(b, sizeof b, "nsweeps=%lld cq=%d fused=%d persist=%d shard=%d no_graph=%d profile=%d stats_valid=%d calibrate=%d gs=%d", (long long)in.nsweeps, in.cq, in.fused, in.persist,
             in.shard, in.no_graph, in.profile, in.stats_valid, in.calibrate, in.graph_sweeps);
    return b;
}

// erm_timing.pass_launches of the call, from the schedule as it was written out in Engine::run_checked / run_model before the planner existed
static int64_t expected_pass_launches(const RunIn& in)
{
    const int64_t n = in.nsweeps;
    const int GS = in.graph_sweeps;
    const int per = in.cq ? 2 : 1;      // was: enqueue_sweep -> launch_pass<MODEL, 0> and (Cross family) launch_pass<MODEL, 1>, each `++n_pass_timed`; launch_fused: one
    // was: `const bool persistent_run = persist && !sharded() && nsweeps > 0 && !m_cq();` and launch_persist: `ev = cfg.profile && ...; n_pass_timed += nsweeps`
    if (in.persist && in.shard == SHARD_NONE && n > 0 && !in.cq) return in.profile ? n : 0;
    const bool graph_timing = in.profile && !in.cq && in.fused && in.shard == SHARD_NONE;      // was: `cfg.profile && !fam_cq(MODEL) && fused() && !sharded()`
    const bool single_timing = in.profile && !graph_timing;                                    // was: `cfg.profile && !graph_timing`
    const bool use_graph = in.shard != SHARD_CALLBACK && !in.no_graph;                         // was: `exch == nullptr && (cfg.flags & ERM_FLAG_NO_GRAPH) == 0`
    // was: `if (exch == nullptr && !NO_GRAPH && !sharded() && !persistent_run && stats_valid && !calibrate && nsweeps >= 1 && !(cfg.profile && !graph_timing)) whole = ...`;
    // whole == 1: `n_pass_timed += nsweeps` when graph_timing; whole == 2: replay(): `launches += nsw`, close(): `n_pass_timed += launches`, over all nsweeps
    if (use_graph && in.shard == SHARD_NONE && in.stats_valid && !in.calibrate && n >= 1 && !single_timing) return graph_timing ? n : 0;
    // was: `if (use_graph && !single_timing)`: every replayed sweep in `launches` when graph_timing, the at most one sweep left `enqueue_sweep(graph_timing || ...)`
    if (use_graph && !single_timing) return graph_timing ? n : 0;
    if (!in.profile) return 0;
    if (graph_timing) return n;         // was: (no graphs) `for (...; k < nsweeps; ...) enqueue_sweep(graph_timing || ...)`: every fused sweep, one kernel each
    int64_t timed = 0, k = 0;
    // was: `else if (use_graph && nsweeps >= 2 * (GRAPH_SWEEPS + 2)) for (; nsweeps - k >= GRAPH_SWEEPS + 2; k += GRAPH_SWEEPS + 2) { enqueue_sweep(true); enqueue_sweep(false); graph }`
    if (use_graph && n >= 2 * (GS + 2)) { timed = n / (GS + 2); k = timed * (GS + 2); }
    // was: `short_run = nsweeps < 2 * (GRAPH_SWEEPS + 2); for (r = 0; k < nsweeps; ++k, ++r) enqueue_sweep(... single_timing && (short_run || (r % PROFILE_STRIDE) == 0))`
    timed += n < 2 * (GS + 2) ? n - k : (n - k + 7) / 8;
    return timed * per;
}

// run_steps' executor with the HIP calls replaced by counters
struct Fake {
    const RunIn& in;
    const Plan& P;
    std::string d;
    bool capturing = false;
    std::map<int, bool> graphs;
    bool open = false;
    int in_bracket = 0, cur = 0, builds = 0;
    int64_t begins = 0, prologues = 0, sweeps = 0, closes = 0, ends = 0, timed = 0, brackets = 0, persist_launches = 0, graph_launches = 0;
    unsigned long long hash = 1469598103934665603ull;
    Fake(const RunIn& i, const Plan& p) : in(i), P(p), d(describe(i)) {}
    static int key(const Step& s) { return s.kind * 100000 + (s.kind == STEP_BLOCK ? s.gi : s.n); }
    void mix(unsigned long long v) { hash = (hash ^ v) * 1099511628211ull; }
    // the kernels of a call in stream order
    void emit(int kind, int64_t count) {
        switch (kind) {
        case STEP_RUN_BEGIN: REQUIRE(begins + prologues + sweeps + closes + ends == 0, "%s: run-begin is not first", d.c_str()); ++begins; break;
        case STEP_PROLOGUE: REQUIRE(begins == 1 && sweeps + closes + ends == 0, "%s: prologue out of place", d.c_str()); ++prologues; break;
        case STEP_TINY_CLOSE: REQUIRE(begins == 1 && closes + ends == 0, "%s: closing tiny step out of place", d.c_str()); ++closes; break;
        case STEP_RUN_END: REQUIRE(begins == 1 && closes == 1 && ends == 0, "%s: run-end out of place", d.c_str()); ++ends; break;
        default: REQUIRE(begins == 1 && closes + ends == 0, "%s: a sweep outside run-begin ... closing step", d.c_str()); sweeps += count;
        }
    }
    bool built(const Step& s) const { return graphs.count(key(s)) != 0; }
    int build(const Step& s) {
        REQUIRE(!open, "%s: graph %d:%d built inside an open bracket", d.c_str(), s.kind, s.n);
        REQUIRE(!capturing, "%s: a graph built inside a capture", d.c_str());
        REQUIRE(!P.flips || cur == 0, "%s: graph %d:%d captured at parity 1", d.c_str(), s.kind, s.n);
        const Plan body = graph_body(P, s);
        Fake sub(in, body);
        sub.capturing = true; sub.begins = s.kind == STEP_FULL ? 0 : 1;
        run_steps(body, 0, body.n, sub);
        REQUIRE(sub.sweeps == s.n && sub.timed == 0 && sub.brackets == 0, "%s: graph %d:%d captures %lld sweeps", d.c_str(), s.kind, s.n, (long long)sub.sweeps);
        REQUIRE((sub.closes == 1 && sub.ends == 1) == (s.kind != STEP_BLOCK) && sub.closes == sub.ends, "%s: graph %d:%d closing steps", d.c_str(), s.kind, s.n);
        graphs[key(s)] = true; ++builds;
        return 0;
    }
    int bracket(bool close, int64_t n) {
        if (close ? !open : (open || !in.profile)) return 0;      // Engine::bracket without the capacity check
        REQUIRE(!capturing, "%s: an event record inside a capture", d.c_str());
        open = !close;
        if (close) { ++brackets; timed += n; in_bracket = 0; }
        return 0;
    }
    void flip(int64_t n) { cur = (int)((cur + n) & 1); }
    int launch(const Step& s, bool t) {
        if (!capturing) { mix((unsigned long long)s.kind); mix((unsigned long long)s.n); mix(is_graph(s.kind) ? (unsigned long long)s.gi : (unsigned long long)t); }
        if (is_graph(s.kind)) {
            REQUIRE(built(s), "%s: graph %d:%d replayed before it was built", d.c_str(), s.kind, s.n);
            REQUIRE(!P.flips || (cur == 0 && sweeps % 2 == 0), "%s: graph %d:%d replayed at parity 1 (%lld sweeps ahead)", d.c_str(), s.kind, s.n, (long long)sweeps);
            REQUIRE(!P.flips || s.kind != STEP_BLOCK || s.n % 2 == 0, "%s: block graph of %d sweeps", d.c_str(), s.n);
            REQUIRE(t == open || !in.profile, "%s: graph %d:%d timed %d, bracket open %d", d.c_str(), s.kind, s.n, (int)t, (int)open);
            if (open) { ++in_bracket; REQUIRE(in_bracket <= 4, "%s: %d replays in one bracket", d.c_str(), in_bracket); }
            ++graph_launches;
            if (s.kind == STEP_FULL) emit(STEP_RUN_BEGIN, 0);
            emit(STEP_SINGLE, s.n);
            if (s.kind != STEP_BLOCK) { emit(STEP_TINY_CLOSE, 0); emit(STEP_RUN_END, 0); }
            return 0;
        }
        REQUIRE(!open, "%s: step %d inside a graph bracket", d.c_str(), s.kind);
        emit(s.kind, s.n);
        if (s.kind == STEP_PERSIST) { ++persist_launches; REQUIRE(s.n >= 1 && s.n <= (1 << 20), "%s: persistent launch of %d sweeps", d.c_str(), s.n); }
        // Engine::launch_persist brackets the launch (n sweeps), enqueue_sweep each of its row-pass kernels
        if (t && in.profile && (s.kind == STEP_PERSIST || s.kind == STEP_SINGLE)) { const int k = s.kind == STEP_PERSIST ? 1 : in.cq ? 2 : 1; brackets += k; timed += s.kind == STEP_PERSIST ? s.n : k; }
        return 0;
    }
};

// sweeps and timed sweep-kernel launches of steps [i, i + count) read off the plan (for calls too long to execute launch by launch)
static void tally(const RunIn& in, const Plan& P, int i, int count, int64_t mult, int64_t& sweeps, int64_t& timed)
{
    for (int e = i + count; i < e; ++i) {
        const Step& s = P.step[i];
        if (s.kind == STEP_REPEAT) { tally(in, P, i + 1, s.n, mult * s.reps, sweeps, timed); i += s.n; continue; }
        if (!has_sweeps(s.kind)) continue;
        sweeps += mult * s.reps * s.n;
        if (s.stride > 0 && in.profile) timed += mult * (s.kind == STEP_SINGLE ? (s.reps + s.stride - 1) / s.stride * (in.cq ? 2 : 1) : s.reps * s.n);
    }
}

static void print_plan(const Plan& P)
{
    static const char* names[] = {"begin", "prologue", "persist", "full", "tail", "block", "single", "close", "end", "repeat"};
    printf("plan=");
    for (int i = 0; i < P.n; ++i) {
        const Step& s = P.step[i];
        printf("%s%s", i ? "," : "", names[s.kind]);
        if (has_sweeps(s.kind) || s.kind == STEP_REPEAT) printf(":%d", s.n);
        if (s.reps != 1) printf("x%lld", (long long)s.reps);
        if (s.stride) printf("/t%d", s.stride);
    }
}

static void check(const RunIn& in, bool print = false)
{
    const std::string ds = describe(in);
    const char* d = ds.c_str();
    const Plan P = plan_run(in);
    ++n_plans;
    REQUIRE(P.n >= 1 && P.n <= 9, "%s: %d steps", d, P.n);
    REQUIRE(P.flips == (!in.cq && in.fused), "%s: flips %d", d, (int)P.flips);
    const int64_t want = expected_pass_launches(in);
    int64_t sweeps = 0, timed = 0;
    tally(in, P, 0, P.n, 1, sweeps, timed);
    REQUIRE(sweeps == in.nsweeps, "%s: the plan holds %lld sweeps", d, (long long)sweeps);
    REQUIRE(timed == want, "%s: the plan times %lld sweep kernels, the schedule it replaces %lld", d, (long long)timed, (long long)want);
    int64_t persist_launches = 0;
    for (int i = 0; i < P.n; ++i) {
        const Step& s = P.step[i];
        REQUIRE(s.reps >= 1 && s.stride >= 0 && (in.profile || s.stride == 0), "%s: step %d reps %lld stride %d", d, i, (long long)s.reps, s.stride);
        if (s.kind == STEP_REPEAT) REQUIRE(s.n >= 1 && i + s.n < P.n, "%s: repeat group runs off the plan", d);
        if (s.kind == STEP_PERSIST) { persist_launches += s.reps; REQUIRE(P.persistent && s.n >= 1 && s.n <= (1 << 20), "%s: persistent step of %d", d, s.n); }
        if (is_graph(s.kind)) {
            REQUIRE(!P.persistent && in.shard != SHARD_CALLBACK && !in.no_graph, "%s: a graph step where none may be", d);
            REQUIRE(s.n >= 1 && s.n <= in.graph_sweeps && (s.kind != STEP_BLOCK || (s.gi >= 0 && s.gi < NBLOCK && s.n == block_sweeps(in.graph_sweeps, s.gi))), "%s: graph step %d:%d", d, s.kind, s.n);
            // a profiled Cross-family, two-kernel or sharded call times single sweeps only
            if (in.cq || !in.fused || in.shard != SHARD_NONE) REQUIRE(s.stride == 0, "%s: a timed graph of sweeps that hold more than the sweep kernel", d);
            if (s.kind != STEP_BLOCK) REQUIRE(in.stats_valid && !in.calibrate, "%s: a whole-call graph without resident statistics / in the calibrating call", d);
        }
    }
    if (P.persistent) REQUIRE(persist_launches == (in.nsweeps + (1 << 20) - 1) / (1 << 20), "%s: %lld persistent launches", d, (long long)persist_launches);
    int64_t brackets = 0;
    if (in.nsweeps <= (1 << 20) + 1) {      // launch by launch: first every graph unbuilt, then with all of them built
        ++n_executed;
        Fake a(in, P), b(in, P);
        REQUIRE(run_steps(P, 0, P.n, a) == 0, "%s: run_steps failed", d);
        b.graphs = a.graphs;
        REQUIRE(run_steps(P, 0, P.n, b) == 0, "%s: run_steps failed", d);
        for (const Fake* f : {&a, &b}) {
            REQUIRE(f->begins == 1 && f->closes == 1 && f->ends == 1 && f->prologues == (in.stats_valid ? 0 : 1), "%s: begin %lld prologue %lld close %lld end %lld", d, (long long)f->begins,
                    (long long)f->prologues, (long long)f->closes, (long long)f->ends);
            REQUIRE(f->sweeps == in.nsweeps && !f->open, "%s: %lld sweeps enqueued", d, (long long)f->sweeps);
            REQUIRE(f->timed == want, "%s: %lld sweep kernels timed, the schedule it replaces %lld", d, (long long)f->timed, (long long)want);
            REQUIRE(!P.flips || f->cur == (int)(in.nsweeps & 1), "%s: parity %d after the call", d, f->cur);
            REQUIRE(P.flips || f->cur == 0, "%s: a two-kernel schedule moved the parity", d);
        }
        REQUIRE(a.hash == b.hash && a.graph_launches == b.graph_launches, "%s: building graphs changed what the call enqueues", d);
        REQUIRE(b.builds == 0, "%s: a built graph was built again", d);
        brackets = b.brackets;
    }
    if (print) { print_plan(P); printf(" steps=%d flips=%d persistent=%d pass_launches=%lld brackets=%lld\n", P.n, (int)P.flips, (int)P.persistent, (long long)timed, (long long)brackets); }
}

int main(int argc, char** argv)
{
    if (argc >= 11 && !strcmp(argv[1], "case")) {
        RunIn in;
        in.nsweeps = atoll(argv[2]); in.cq = atoi(argv[3]); in.fused = atoi(argv[4]); in.persist = atoi(argv[5]); in.shard = atoi(argv[6]); in.no_graph = atoi(argv[7]);
        in.profile = atoi(argv[8]); in.stats_valid = atoi(argv[9]); in.calibrate = atoi(argv[10]);
        if (argc > 11) in.graph_sweeps = atoi(argv[11]);
        check(in, true);
        return fails ? 1 : 0;
    }
    // every input Engine::run_checked can produce: the Cross family is never fused; the persistent schedule exists for fused, unsharded single-pass engines only;
    // a sharded engine's statistics are never resident; only a profiling engine calibrates
    const int64_t large[] = {(1 << 20) - 1, 1 << 20, (1 << 20) + 1, 2147483647LL};
    for (int gs : {32, 16})
    for (int fam = 0; fam < 3; ++fam) for (int persist = 0; persist < 2; ++persist) for (int shard = 0; shard < 3; ++shard)
    for (int no_graph = 0; no_graph < 2; ++no_graph) for (int profile = 0; profile < 2; ++profile) for (int sv = 0; sv < 2; ++sv) for (int cal = 0; cal < 2; ++cal) {
        RunIn in;
        in.cq = fam == 2; in.fused = fam == 0; in.persist = persist; in.shard = shard; in.no_graph = no_graph; in.profile = profile; in.stats_valid = sv; in.calibrate = cal; in.graph_sweeps = gs;
        if (persist && (fam != 0 || shard != SHARD_NONE)) continue;
        if (sv && shard != SHARD_NONE) continue;
        if (cal && !profile) continue;
        for (int64_t n = 0; n <= 200; ++n) { in.nsweeps = n; check(in); }
        if (gs == 32) for (int64_t n : large) { in.nsweeps = n; check(in); }
    }
    printf("plans %lld (executed launch by launch: %lld), invariant failures %d\n", n_plans, n_executed, fails);
    return fails ? 1 : 0;
}

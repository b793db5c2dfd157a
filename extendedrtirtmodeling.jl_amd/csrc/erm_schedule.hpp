// erm_schedule.hpp -- what ONE erm_run enqueues, as a PURE host function, and the loop that executes it.
//
// Engine::run_checked (ertirt.hip) calls plan_run() and nothing else decides which launches, graph replays and event brackets a call consists of;
// run_steps() is the one loop that enqueues them.  The same header is compiled by g++ with -fsanitize=undefined -ftrapv into tests/schedule_check
// and driven through an executor of counters (tests/test_run_schedule.py).  No HIP, no allocation, no environment.
//
// The rules a plan keeps (asserted there for every input the engine can produce):
//   - every sweep of the call is enqueued exactly once; run-begin comes first, the closing tiny step after the last sweep, run-end last -- each exactly
//     once, on the stream or inside the call's one FULL / TAIL graph;
//   - a graph is replayed only at buffer parity 0 (the parity it was captured with): when sweeps flip the double buffers, the count ahead of every
//     replay is even and so is every BLOCK graph;
//   - a graph is never built inside an open event bracket, and a bracket holds at most BRACKET_REPLAYS replays.
#pragma once
#include <cstdint>

namespace erm {

enum StepKind {
    STEP_RUN_BEGIN,     // run_begin_kernel: counters, tickets, the persistent launch's wait bound
    STEP_PROLOGUE,      // the row pass(es) in mode 0: omega_{t+1} (nu_{t+1}) and the statistics of the current state, when they are not resident
    STEP_PERSIST,       // n sweeps in ONE persistent launch
    STEP_FULL,          // graph full[n]  = run-begin, n sweeps, closing tiny step, run-end: the whole call
    STEP_TAIL,          // graph tail[n]  = n sweeps, closing tiny step, run-end: the end of a call behind its blocks
    STEP_BLOCK,         // graph block[gi] = n sweeps
    STEP_SINGLE,        // one sweep enqueued on the stream
    STEP_TINY_CLOSE,    // the closing tiny step: the log-likelihood of the last sweep
    STEP_RUN_END,       // run_end_kernel: counters and time-out word into pinned host memory
    STEP_REPEAT         // the next n steps, as a group, reps times
};
enum ShardKind { SHARD_NONE, SHARD_CALLBACK, SHARD_RCCL };

struct Step {
    int kind = STEP_SINGLE;
    int n = 0;              // sweeps per launch (REPEAT: steps in the group)
    int gi = 0;             // BLOCK: which of the block graphs
    int64_t reps = 1;       // launches of this step
    int stride = 0;         // event brackets: 0 = none; s = launches 0, s, 2 s, ... of the step are timed (a graph replay shares its bracket with up to
};                          // BRACKET_REPLAYS - 1 timed replays that follow it directly; a sweep of the Cross family is two timed kernels)

struct RunIn {
    int64_t nsweeps = 0;
    bool cq = false;            // Cross family: two row passes per sweep
    bool fused = true;          // Engine::fused(): the tiny step runs inside the row-pass kernel
    bool persist = false;       // small data sets: the persistent schedule is available
    int shard = SHARD_NONE;     // a callback exchange synchronises with the host once per pass and cannot be captured; RCCL's all-gather is a stream operation
    bool no_graph = false;      // ERM_FLAG_NO_GRAPH
    bool profile = false;       // erm_config.profile
    bool stats_valid = false;   // omega_{t+1} and the statistics of the current state are resident
    bool calibrate = false;     // this call also measures the empty event pair (the first call of a profiling engine)
    int graph_sweeps = 32;
};

constexpr int MAX_STEPS = 12;               // the longest plan has nine
constexpr int NBLOCK = 4;
constexpr int BRACKET_REPLAYS = 4;
constexpr int PROFILE_STRIDE = 8;
constexpr int PERSIST_MAX_SWEEPS = 1 << 20; // per launch: packet tags are 32 bits and only grow

struct Plan {
    Step step[MAX_STEPS];
    int n = 0;
    bool flips = false;         // a sweep of this plan flips the double buffers (the fused kernel reads [cur], writes [1 - cur])
    bool persistent = false;    // the sweeps run in persistent launches
    void add(int kind, int n_ = 0, int64_t reps = 1, int stride = 0, int gi = 0) {
        if (reps <= 0) return;
        Step& s = step[n < MAX_STEPS ? n++ : MAX_STEPS - 1];
        s.kind = kind; s.n = n_; s.reps = reps; s.stride = stride; s.gi = gi;
    }
};
inline bool is_graph(int kind) { return kind == STEP_FULL || kind == STEP_TAIL || kind == STEP_BLOCK; }
inline bool has_sweeps(int kind) { return kind == STEP_PERSIST || kind == STEP_SINGLE || is_graph(kind); }
inline int block_sweeps(int graph_sweeps, int gi) { const int s[NBLOCK] = {graph_sweeps, 16, 4, 2}; return s[gi]; }

inline Plan plan_run(const RunIn& in)
{
    Plan P;
    const int64_t n = in.nsweeps;
    const int GS = in.graph_sweeps;
    P.flips = !in.cq && in.fused;
    P.persistent = in.persist && in.shard == SHARD_NONE && n > 0 && !in.cq;
    const bool use_graph = in.shard != SHARD_CALLBACK && !in.no_graph;
    // profile mode (erm_get_timing: the live kernel time of bench.py's roofline).  Fused single-pass sweeps: every replayed graph holds launches of the sweep
    // kernel and little else, so the event pairs go around graph replays and every sweep of the call is inside a bracket while it proceeds at replay speed.
    // The Cross family's sweeps hold tiny kernels too, a sharded sweep its pack kernel and all-gather: those are bracketed kernel by kernel on singly
    // enqueued sweeps.
    const bool graph_timing = in.profile && P.flips && in.shard == SHARD_NONE;
    const bool single_timing = in.profile && !graph_timing;
    // The whole call inside graphs: per-sweep schedule, statistics resident, nothing that has to be bracketed kernel by kernel.  Between a graph and an
    // ordinary launch the device idles 10-14 us, inside a graph 0.
    if (use_graph && in.shard == SHARD_NONE && !P.persistent && in.stats_valid && !in.calibrate && n >= 1 && !single_timing) {
        if (n <= GS) { P.add(STEP_FULL, (int)n, 1, graph_timing); return P; }      // (its bracket also holds the three small kernels: ~12 us per call)
        const int r = n % GS == 0 ? GS : (int)(n % GS);
        P.add(STEP_RUN_BEGIN);
        P.add(STEP_BLOCK, GS, (n - r) / GS, graph_timing, 0);
        P.add(STEP_TAIL, r, 1, graph_timing);
        return P;
    }
    P.add(STEP_RUN_BEGIN);
    if (!in.stats_valid) P.add(STEP_PROLOGUE);      // a call that CONTINUES the previous one finds both in place and skips it
    int64_t left = n;
    if (P.persistent) {
        P.add(STEP_PERSIST, PERSIST_MAX_SWEEPS, n / PERSIST_MAX_SWEEPS, in.profile);
        P.add(STEP_PERSIST, (int)(n % PERSIST_MAX_SWEEPS), n % PERSIST_MAX_SWEEPS ? 1 : 0, in.profile);
        left = 0;
    } else if (use_graph && !single_timing) {       // block graphs, largest first, then at most one sweep
        for (int gi = 0; gi < NBLOCK; ++gi) { const int b = block_sweeps(GS, gi); P.add(STEP_BLOCK, b, left / b, graph_timing, gi); left %= b; }
    } else if (use_graph && n >= 2 * (GS + 2)) {    // a long profiled run: a timed sweep, an untimed one (two keep the buffer parity), a block graph
        P.add(STEP_REPEAT, 2, n / (GS + 2));
        P.add(STEP_SINGLE, 1, 2, 2);
        P.add(STEP_BLOCK, GS, 1, 0, 0);
        left = n % (GS + 2);
    }
    // the sweeps no graph took: all timed beside timed graphs and in a short profiled run, every PROFILE_STRIDE-th in a long one
    P.add(STEP_SINGLE, 1, left, graph_timing ? 1 : !single_timing ? 0 : n < 2 * (GS + 2) ? 1 : PROFILE_STRIDE);
    P.add(STEP_TINY_CLOSE);     // (a call without sweeps: nothing to reduce, the step returns at once)
    P.add(STEP_RUN_END);
    return P;
}

// What building the graph of step `g` captures.
inline Plan graph_body(const Plan& of, const Step& g)
{
    Plan B;
    B.flips = of.flips;
    if (g.kind == STEP_FULL) B.add(STEP_RUN_BEGIN);
    B.add(STEP_SINGLE, 1, g.n);
    if (g.kind != STEP_BLOCK) { B.add(STEP_TINY_CLOSE); B.add(STEP_RUN_END); }
    return B;
}

// Enqueues steps [from, to) of a plan on executor `x`:
//   x.launch(step, timed)  one launch of the step (a timed sweep or persistent launch brackets its own kernels)
//   x.built(step) / x.build(step)  a graph step's executable graph
//   x.bracket(close, sweeps)  opens an event bracket / closes the open one, which held `sweeps` timed sweeps (no-ops without profile mode or event pairs left)
//   x.flip(sweeps)  the double buffers after `sweeps` flipping sweeps
template <typename X> int run_steps(const Plan& P, int from, int to, X& x)
{
    int replays = 0;
    int64_t held = 0;       // timed graph replays / their sweeps since the bracket was opened
    auto close = [&]() -> int { const int rc = replays ? x.bracket(true, held) : 0; replays = 0; held = 0; return rc; };
    auto one = [&](const Step& s) -> int {
        for (int64_t r = 0; r < s.reps; ++r) {
            const bool timed = s.stride > 0 && r % s.stride == 0;
            if (!is_graph(s.kind) || !timed || replays >= BRACKET_REPLAYS) { if (int rc = close()) return rc; }
            if (is_graph(s.kind) && !x.built(s)) {      // built by the first call that needs it (a benchmark's warm-up), never inside an event bracket
                if (int rc = close()) return rc;
                if (int rc = x.build(s)) return rc;
            }
            if (is_graph(s.kind) && timed) {
                if (!replays) { if (int rc = x.bracket(false, 0)) return rc; }
                ++replays; held += s.n;
            }
            if (int rc = x.launch(s, timed)) return rc;
            if (P.flips && has_sweeps(s.kind)) x.flip(s.n);
        }
        return 0;
    };
    for (int i = from; i < to; ++i) {
        const Step& s = P.step[i];
        if (s.kind != STEP_REPEAT) { if (int rc = one(s)) return rc; continue; }
        for (int64_t r = 0; r < s.reps; ++r) for (int j = 1; j <= s.n; ++j) { if (int rc = one(P.step[i + j])) return rc; }
        i += s.n;
    }
    return close();
}

}  // namespace erm

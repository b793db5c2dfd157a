// diag_walk_check -- the convergence diagnostics' walk over a trace's blocks, its two kinds of source and its limits (the plain-C++ half of
// extendedrtirtmodeling.jl_amd/csrc/erm_diagnostics.hpp) on the CPU, built with g++ -fsanitize=undefined -ftrapv by tests/test_diag_walk_host.py.
// An executor of counters stands where the device is: it records which columns an estimate or a NaN fill wrote and in which order the operations came.
//   diag_walk_check                         self-checks over the sweep in main(); prints "walks W refusals R limits G failures F"
//   diag_walk_check limits rank Tn chains   prints the refusal of diag_limits ("ok" for none)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "erm_diagnostics.hpp"

using namespace erm;

static int failures = 0;
#define EXPECT(cond, ...) do { if (!(cond)) { ++failures; if (failures <= 20) { printf("FAIL %s:%d: %s  ", __FILE__, __LINE__, #cond); printf(__VA_ARGS__); printf("\n"); } } } while (0)

// what the walk reads of an engine: the config, the rows recorded and where a block's draws are (Engine::block_src restated: a subject-level block in the
// engine's trace type with its own width as the stride, an item-level block in double inside the item trace's rows, nothing for constant columns)
static char g_draws[4];      // addresses only: nothing is read
struct StubEngine {
    struct BlockSrc { const void* p; int64_t ld; size_t elem; };
    erm_config cfg{};
    int64_t rows_done = 0;
    bool nu_resident = true;
    int64_t trace_width(int which) const { return erm::trace_width(cfg.model, which, cfg.n_subj, cfg.n_item, cfg.n_feat); }
    TraceBlocks trace_blocks(int which) const { return erm::trace_blocks(cfg.model, which, cfg.n_subj, cfg.n_item, cfg.n_feat); }
    BlockSrc block_src(const TraceBlock& b) const {
        const size_t real = cfg.precision == ERM_PREC_F32 ? 4 : 8;
        if (b.kind == BLK_SUBJECT || b.kind == BLK_CELL) return { b.src == SUBJ_NU && !nu_resident ? nullptr : g_draws + b.src, b.ncol, real };
        if (b.kind == BLK_ITEM) return { g_draws + 3, item_trace_width(cfg.model, cfg.n_item, cfg.n_feat), 8 };
        return { nullptr, 0, 0 };
    }
};

struct Counters {
    bool rank; int64_t cap; int64_t wd = -1;
    std::vector<int> est, nan;               // writes per column
    std::vector<DiagView> views;             // of every estimate
    int code = 0; std::string msg;
    int drains = 0, allocs = 0, fills = 0, estimates = 0, begins = 0, gathers = 0, ends = 0, finishes = 0, out_of_order = 0;
    bool open = false; int64_t open_chunk = 0; size_t open_elem = 0; const void* gathered = nullptr;
    int device_ops() const { return drains + allocs + fills + estimates + begins + gathers + ends + finishes; }
    int fail(int c, const std::string& m) { code = c; msg = m; return c; }
    int drain() { out_of_order += device_ops() != 0; ++drains; return 0; }
    int alloc(int64_t w) { out_of_order += drains != 1 || allocs != 0; ++allocs; wd = w; est.assign((size_t)w, 0); nan.assign((size_t)w, 0); return 0; }
    int fill_nan(int64_t c0, int64_t nc) { out_of_order += allocs != 1 || open || finishes; ++fills; for (int64_t c = c0; c < c0 + nc; ++c) ++nan.at((size_t)c); return 0; }
    int estimate(const DiagView& v, int64_t c0, int64_t nc) {
        out_of_order += allocs != 1 || finishes || (open && v.p != gathered);
        ++estimates; views.push_back(v);
        for (int64_t c = c0; c < c0 + nc; ++c) ++est.at((size_t)c);
        return 0;
    }
    int finish() { out_of_order += open || allocs != 1; ++finishes; return 0; }
    int64_t chunk_cap() const { return cap; }
    int gather_begin(int64_t chunk, int, size_t elem) { out_of_order += open || allocs != 1; open = true; open_chunk = chunk; open_elem = elem; ++begins; return 0; }
    int gather(const TraceBlock&, const FarmDiagChunk& ch, DiagView& v) {
        out_of_order += !open || ch.nc > open_chunk || ch.nc < 1 || v.elem != open_elem;
        ++gathers; v.p = gathered = g_draws + (gathers & 1);
        return 0;
    }
    int gather_end() { out_of_order += !open; open = false; ++ends; return 0; }
};

struct Case { int model; int which; bool rank; int L; bool farm; int64_t cap; int64_t N; int J, F; int prec; };
#define CASE "model %d which %d rank %d L %d farm %d cap %lld N %lld J %d F %d prec %d", c.model, c.which, (int)c.rank, c.L, (int)c.farm, (long long)c.cap, (long long)c.N, c.J, c.F, c.prec

// L engines: a farm's chains (n_chain = 1 each) or one engine of L interleaved chains
static std::vector<StubEngine> engines(const Case& c, int n_iter, int n_burnin)
{
    std::vector<StubEngine> e((size_t)(c.farm ? c.L : 1));
    for (StubEngine& s : e) {
        s.cfg.model = c.model; s.cfg.n_subj = c.N; s.cfg.n_item = c.J; s.cfg.n_feat = c.F; s.cfg.precision = c.prec; s.cfg.trace_mode = ERM_TRACE_FULL;
        s.cfg.n_iter = n_iter; s.cfg.n_burnin = n_burnin; s.cfg.n_chain = c.farm ? 1 : c.L;
        s.rows_done = (int64_t)n_iter * s.cfg.n_chain;
    }
    return e;
}
static int walk(std::vector<StubEngine>& e, const Case& c, Counters& x)
{
    std::vector<StubEngine*> p;
    for (StubEngine& s : e) p.push_back(&s);
    return diag_walk(DiagSource<StubEngine>{p.data(), (int)p.size(), c.farm}, c.which, c.rank, x);
}

static void check_walk(const Case& c)
{
    const int n_iter = 30, n_burnin = 13, Tn = n_iter - n_burnin;
    std::vector<StubEngine> e = engines(c, n_iter, n_burnin);
    Counters x{c.rank, c.cap};
    const int rc = walk(e, c, x);
    const TraceBlocks blocks = e[0].trace_blocks(c.which);
    if (blocks.width() <= 0) {      // GibbsMlIrt has no rt trace
        EXPECT(rc == ERM_ERR_ARG && x.device_ops() == 0, CASE);
        return;
    }
    EXPECT(rc == 0 && x.code == 0 && x.out_of_order == 0, CASE);
    EXPECT(x.drains == 1 && x.allocs == 1 && x.finishes == 1 && !x.open && x.wd == blocks.width(), CASE);
    int64_t want_est = 0, want_fill = 0, want_begin = 0;
    for (const TraceBlock& b : blocks) {
        for (int64_t k = b.col0; k < b.col0 + b.ncol; ++k) {      // every column once: by one estimate, or (constant columns only) by one NaN fill
            EXPECT(x.est[(size_t)k] + x.nan[(size_t)k] == 1 && x.nan[(size_t)k] == (b.kind == BLK_ZERO), CASE);
        }
        if (b.kind == BLK_ZERO) { ++want_fill; continue; }
        const size_t elem = b.kind == BLK_ITEM ? 8 : (c.prec == ERM_PREC_F32 ? 4 : 8);
        want_est += c.farm ? farm_diag_chunks(b.ncol, Tn, c.L, (int64_t)elem, FARM_DIAG_BUDGET, c.cap).count() : 1;
        want_begin += c.farm;
    }
    EXPECT(x.fills == want_fill && x.estimates == want_est && x.begins == want_begin && x.ends == want_begin, CASE);
    EXPECT(x.gathers == (c.farm ? want_est : 0), CASE);      // one gather per chunk; an engine is read in place
    for (const DiagView& v : x.views) {
        if (c.farm) EXPECT(v.n_iter == Tn && v.n_chain == c.L && v.n_burnin == 0 && v.p != nullptr && v.ld >= 1 && (c.cap <= 0 || v.ld <= c.cap), CASE);
        else EXPECT(v.n_iter == n_iter && v.n_chain == c.L && v.n_burnin == n_burnin && v.p != nullptr, CASE);
    }
    if (!c.farm) {      // the views are the engine's blocks as they stand
        size_t i = 0;
        for (const TraceBlock& b : blocks) if (b.kind != BLK_ZERO) {
            const StubEngine::BlockSrc s = e[0].block_src(b);
            EXPECT(i < x.views.size() && x.views[i].p == s.p && x.views[i].ld == s.ld && x.views[i].elem == s.elem, CASE);
            ++i;
        }
    }
}

// one broken precondition (or two: the first named is the one reported), the code, a fragment of the message -- and no device work at all
static int refusals = 0;
static void refused(const Case& c, std::vector<StubEngine>& e, int which, int code, const char* text)
{
    Case cc = c; cc.which = which;
    Counters x{c.rank, c.cap};
    const int rc = walk(e, cc, x);
    EXPECT(rc == code && x.code == code && x.device_ops() == 0 && strstr(x.msg.c_str(), text), CASE);
    if (!(rc == code && strstr(x.msg.c_str(), text)) && failures <= 20) printf("   got %d \"%s\", want %d \"%s\"\n", rc, x.msg.c_str(), code, text);
    ++refusals;
}
static void check_refusals(const Case& c)
{
    const int last = c.farm ? c.L - 1 : 0;
    { auto e = engines(c, 30, 13); refused(c, e, ERM_TRACE_LOGLIKE, ERM_ERR_ARG, "ra / rt / qr"); }
    { auto e = engines(c, 30, 13); e[(size_t)last].rows_done -= 1; refused(c, e, ERM_TRACE_RA, ERM_ERR_STATE, c.farm ? ("chain " + std::to_string(last) + ": trace incomplete").c_str() : "trace incomplete");
      e[0].rows_done = 0; refused(c, e, ERM_TRACE_QR, ERM_ERR_STATE, c.farm ? "chain 0: " : "trace incomplete");
      for (auto& s : e) s.cfg.trace_mode = ERM_TRACE_SUMMARY;
      refused(c, e, ERM_TRACE_RA, ERM_ERR_STATE, "trace incomplete"); }                       // rows still to run come before the trace mode
    { auto e = engines(c, 26, 20); for (auto& s : e) s.cfg.trace_mode = ERM_TRACE_SUMMARY;
      refused(c, e, ERM_TRACE_RA, ERM_ERR_NOTRACE, "ERM_TRACE_FULL"); }                       // ... the trace mode before the limits
    { auto e = engines(c, 26, 20); for (auto& s : e) s.nu_resident = false;
      refused(c, e, ERM_TRACE_QR, ERM_ERR_ARG, "too few post-burn-in"); }                     // ... the limits before a block that is not resident
    if (c.rank) { auto e = engines(c, 2 * (RK_MAX_DRAWS / (2 * c.L)) + 2, 0); refused(c, e, ERM_TRACE_RA, ERM_ERR_ARG, "8192"); }
    if (model_traits(c.model).nu != NU_NONE) {
        auto e = engines(c, 30, 13); e[(size_t)last].nu_resident = false;
        refused(c, e, ERM_TRACE_QR, ERM_ERR_NOTRACE, c.model == CROSSQR ? "nu trace" : "not recorded");
        if (c.farm) refused(c, e, ERM_TRACE_QR, ERM_ERR_NOTRACE, ("chain " + std::to_string(last) + ": ").c_str());
        Counters x{c.rank, c.cap};
        Case ra = c; ra.which = ERM_TRACE_RA;
        EXPECT(walk(e, ra, x) == 0 && x.estimates > 0, CASE);                                   // ra does not need the nu trace
    }
}

// The rule of the code this walk replaced, restated: the rank entries refused fewer than 8 rows after burn-in, then fewer than 1 or more than 16 chains (32 split
// sequences), then more than 8192 used draws S = 2 * chains * floor(Tn / 2); the basic entries the first two.  0 = accepted, 1 .. 3 = which refusal.
static int parent_verdict(bool rank, long long Tn, long long chains)
{
    if (Tn / 2 < 4) return 1;
    if (chains < 1 || 2 * chains > 32) return 2;
    if (rank && 2 * chains * (Tn / 2) > 8192) return 3;
    return 0;
}
static int verdict(bool rank, int64_t Tn, int64_t chains)
{
    const std::string m = diag_limits(rank, Tn, chains);
    if (m.empty()) return 0;
    const bool few = m.find("too few post-burn-in") != std::string::npos, many = m.find("too many chains") != std::string::npos, cap = m.find("8192") != std::string::npos;
    return few + many + cap != 1 ? -1 : few ? 1 : many ? 2 : 3;
}

int main(int argc, char** argv)
{
    if (argc == 5 && !strcmp(argv[1], "limits")) {
        const std::string m = diag_limits(atoi(argv[2]) != 0, atoll(argv[3]), atoll(argv[4]));
        printf("%s\n", m.empty() ? "ok" : m.c_str());
        return 0;
    }
    long long walks = 0, grid = 0;
    // N = 37, J = 5: CrossQr's nu block has 185 columns, no multiple of four and of no cap; N = 1 and J = 1: the narrowest blocks; 1000 x 9: several chunks of 100
    const struct { int64_t N; int J, F; } shapes[] = { {37, 5, 3}, {1, 1, 0}, {1000, 9, 2} };
    const struct { int L; bool farm; } sources[] = { {3, false}, {1, false}, {1, true}, {3, true}, {16, true} };
    for (int model = 0; model < 7; ++model) for (int which : {ERM_TRACE_RA, ERM_TRACE_RT, ERM_TRACE_QR}) for (bool rank : {false, true}) for (const auto& s : sources)
        for (int64_t cap : {0, 1, 100}) for (const auto& sh : shapes) for (int prec : {ERM_PREC_F32, ERM_PREC_F64}) {
            const Case c{model, which, rank, s.L, s.farm, cap, sh.N, sh.J, sh.F, prec};
            check_walk(c);
            ++walks;
            if (which == ERM_TRACE_RA && cap == 0 && sh.N == 37 && prec == ERM_PREC_F64) check_refusals(c);
        }
    {   // 17 chains, interleaved or farmed: refused by name, whatever the estimator
        for (bool farm : {false, true}) for (bool rank : {false, true}) {
            const Case c{RTIRT, ERM_TRACE_RA, rank, 17, farm, 0, 64, 5, 3, ERM_PREC_F64};
            auto e = engines(c, 30, 14);
            refused(c, e, ERM_TRACE_RA, ERM_ERR_ARG, "too many chains");
        }
    }
    for (bool rank : {false, true}) {
        for (long long Tn = 0; Tn <= 20; ++Tn) for (long long ch = 0; ch <= 20; ++ch, ++grid)
            EXPECT(verdict(rank, Tn, ch) == parent_verdict(rank, Tn, ch), "rank %d Tn %lld chains %lld", (int)rank, Tn, ch);
        // the cap of 8192 used draws from either side: one chain and sixteen, an odd row count (the odd row is not used)
        for (long long ch : {1, 2, 3, 16}) for (long long Tn = 2 * (8192 / (2 * ch)) - 3; Tn <= 2 * (8192 / (2 * ch)) + 4; ++Tn, ++grid)
            EXPECT(verdict(rank, Tn, ch) == parent_verdict(rank, Tn, ch), "rank %d Tn %lld chains %lld", (int)rank, Tn, ch);
        EXPECT(verdict(rank, -5, 1) == 1 && verdict(rank, 0x7fffffff, 255) == 2 && verdict(rank, 0x7fffffff, 16) == (rank ? 3 : 0), "the ends of the range");
    }
    EXPECT(verdict(true, 8192, 1) == 0 && verdict(true, 8193, 1) == 0 && verdict(true, 8194, 1) == 3 && verdict(true, 512, 16) == 0 && verdict(true, 514, 16) == 3, "the cap");
    EXPECT(verdict(false, 8194, 1) == 0 && verdict(false, 514, 16) == 0, "the basic estimator has no cap");
    printf("walks %lld refusals %d limits %lld failures %d\n", walks, refusals, grid, failures);
    return failures ? 1 : 0;
}

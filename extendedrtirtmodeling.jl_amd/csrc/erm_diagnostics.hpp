// erm_diagnostics.hpp -- the host path of the convergence diagnostics: erm_get_diagnostics / _convergence / _rank_diagnostics / _rank_convergence,
// their four erm_farm_* siblings and erm_debug_diagnostics / erm_debug_rank_diagnostics are argument checks plus ONE call of diag_query below.
//
// The first half is plain C++: what a column view is, the limits of the estimators, the two ways a source yields views and the walk over a trace's blocks.  The walk
// reaches the device only through the operations of an executor `x`, as plan_run / run_steps do (erm_schedule.hpp); g++ compiles this half with
// -fsanitize=undefined -ftrapv into tests/diag_walk_check and drives it with an executor of counters (tests/test_diag_walk_host.py).
// The second half (hipcc only) is that executor on the device, the one caller of the estimator kernels, the fetch and the counts.  ertirt.hip includes this header
// where its DevBuf, fail / HIPCHK, count_converged, rank_diag_run, EngineBase and debug_upload are in scope.
#pragma once
#include <cstdint>
#include <string>
#include "ertirt.h"
#include "erm_model.hpp"
#include "erm_farm_diag.hpp"
#include "erm_rankdiag.hpp"

namespace erm {

// Columns an estimator reads as they stand: rows laid out as [row = m * n_chain + l][ld], iteration m of chain l, of which the first n_burnin iterations are skipped
struct DiagView {
    const void* p;          // column 0 of row 0
    int64_t ld;             // row stride in elements
    size_t elem;            // sizeof(float) or sizeof(double): the element type
    int n_iter, n_chain, n_burnin;
};

// What the estimators take, for every entry: Tn rows after burn-in of `chains` chains.  "" or the refusal (ERM_ERR_ARG).
constexpr int DIAG_MAX_CHAINS = 16;      // 2 * 16 split sequences = DIAG_MAXSEQ (erm_service_kernels.hpp)
inline std::string diag_limits(bool rank, int64_t Tn, int64_t chains)
{
    if (Tn / 2 < 4) return "too few post-burn-in iterations for split-chain diagnostics (need >= 8)";
    if (chains < 1 || chains > DIAG_MAX_CHAINS) return "too many chains for the diagnostics kernel (at most " + std::to_string(DIAG_MAX_CHAINS) + ")";
    const int64_t S = 2 * chains * (Tn / 2);
    if (rank && S > RK_MAX_DRAWS) return "rank diagnostics take at most " + std::to_string(RK_MAX_DRAWS) + " used draws per column (2 * n_chain * floor((n_iter - n_burnin) / 2) = " +
                                         std::to_string(S) + ")";
    return "";
}

// Where the draws are: L engines of type E (EngineBase; the debug entries' UploadedDraws; the CPU test's stand-in), read through block_src, trace_blocks,
// trace_width, rows_done and cfg.
//   in place   ONE engine: a resident block is one view with the engine's n_iter, n_chain and n_burnin, and nothing is copied;
//   gathered   a chain farm, engine l = chain l (n_chain = 1 each, a farm of one chain included): the post-burn-in rows of a chunk of columns of every chain are
//              gathered into one interleaved scratch (x.gather; chunks: erm_farm_diag.hpp), a view of L chains without burn-in.
template <typename E> struct DiagSource {
    E* const* eng; int L; bool gathered;
    const erm_config& cfg() const { return eng[0]->cfg; }
    int chains() const { return gathered ? L : cfg().n_chain; }
    int Tn() const { return cfg().n_iter - cfg().n_burnin; }
    std::string chain(int l) const { return gathered ? "chain " + std::to_string(l) + ": " : ""; }
    // f(view, c0, nc) for views that cover columns [c0, c0 + nc) of block b, every column of the block once
    template <typename X, typename F> int views(const TraceBlock& b, X& x, F&& f) const {
        const auto s = eng[0]->block_src(b);
        if (!gathered) return f(DiagView{s.p, s.ld, s.elem, cfg().n_iter, cfg().n_chain, cfg().n_burnin}, (int64_t)0, b.ncol);
        const FarmDiagChunks plan = farm_diag_chunks(b.ncol, Tn(), L, (int64_t)s.elem, FARM_DIAG_BUDGET, x.chunk_cap());
        if (int rc = x.gather_begin(plan.chunk, Tn(), s.elem)) return rc;
        for (int64_t i = 0; i < plan.count(); ++i) {
            const FarmDiagChunk ch = plan.at(i);
            DiagView v{nullptr, ch.nc, s.elem, Tn(), L, 0};
            if (int rc = x.gather(b, ch, v)) return rc;
            if (int rc = f(v, ch.c0, ch.nc)) return rc;
        }
        return x.gather_end();
    }
};

// Every column of trace `which` of the source through the basic (ess, rhat) or the rank (bulk, tail, rhat) estimator, into x's 2 or 3 output vectors of
// trace_width(which) doubles; a block in device order (TraceBlock::device_order) is diagnosed in that order.  All refusals come before any device work, in the
// order the engine, the farm and the debug entries always had: the trace asked for, rows still to run (ERM_ERR_STATE), the trace mode (ERM_ERR_NOTRACE), the
// limits (ERM_ERR_ARG), a block that is not resident (ERM_ERR_NOTRACE).
template <typename E, typename X> int diag_walk(const DiagSource<E>& src, int which, bool rank, X& x)
{
    const int64_t wd = src.eng[0]->trace_width(which);
    if (which == ERM_TRACE_LOGLIKE || wd <= 0) return x.fail(ERM_ERR_ARG, "diagnostics exist for the ra / rt / qr traces");
    for (int l = 0; l < src.L; ++l) if (src.eng[l]->rows_done != (int64_t)src.eng[l]->cfg.n_iter * src.eng[l]->cfg.n_chain)
        return x.fail(ERM_ERR_STATE, src.chain(l) + (src.gathered ? "trace incomplete: run n_iter sweeps of every chain first" : "trace incomplete: run n_iter*n_chain sweeps first"));
    if (src.cfg().trace_mode != ERM_TRACE_FULL) return x.fail(ERM_ERR_NOTRACE, "subject-level traces need trace_mode = ERM_TRACE_FULL");
    if (const std::string no = diag_limits(rank, src.Tn(), src.chains()); !no.empty()) return x.fail(ERM_ERR_ARG, no);
    const TraceBlocks blocks = src.eng[0]->trace_blocks(which);
    for (const TraceBlock& b : blocks) if (b.kind != BLK_ZERO) for (int l = 0; l < src.L; ++l) if (!src.eng[l]->block_src(b).p)
        return x.fail(ERM_ERR_NOTRACE, src.chain(l) + (b.kind == BLK_CELL ? "the per-sweep nu trace was not recorded (erm_config.nu_trace_max_gb)" : "this trace was not recorded"));
    if (int rc = x.drain()) return rc;                     // the chains' streams: the traces are complete on their devices
    if (int rc = x.alloc(wd)) return rc;
    for (const TraceBlock& b : blocks) {
        if (b.kind == BLK_ZERO) { if (int rc = x.fill_nan(b.col0, b.ncol)) return rc; continue; }      // constant columns: NaN
        if (int rc = src.views(b, x, [&](const DiagView& v, int64_t c0, int64_t nc) { return x.estimate(v, b.col0 + c0, nc); })) return rc;
    }
    return x.finish();
}

}  // namespace erm

#ifdef __HIPCC__
static_assert(2 * DIAG_MAX_CHAINS == DIAG_MAXSEQ, "diag_limits and diag_kernel disagree about the number of split sequences");

// Columns [0, nc) of a view through one estimator into out[q] + c0 (ess, rhat | bulk, tail, rhat) on `stream`: the ONE caller of diag_kernel and rank_diag_run
static int estimate(const DiagView& v, int64_t c0, int64_t nc, bool rank, hipStream_t stream, double* const* out)
{
    auto run = [&](auto* tr) -> int {
        using T = std::remove_const_t<std::remove_pointer_t<decltype(tr)>>;
        if (rank) return rank_diag_run(tr, v.ld, nc, v.n_chain, v.n_burnin, v.n_iter - v.n_burnin, stream, out[0] + c0, out[1] + c0, out[2] + c0);
        hipLaunchKernelGGL((diag_kernel<T>), dim3((unsigned)((nc + 255) / 256)), dim3(256), 0, stream, tr, (long long)nc, (long long)v.ld, v.n_iter, v.n_chain, v.n_burnin, out[0] + c0, out[1] + c0);
        HIPCHK(hipGetLastError());
        return 0;
    };
    return v.elem == sizeof(float) ? run(static_cast<const float*>(v.p)) : run(static_cast<const double*>(v.p));
}

// diag_walk's executor on the device.  The outputs, the gathered draws and every estimator launch are on chain 0's device and stream.  The gather
// (farm_gather_kernel) reads a chain that shares chain 0's device in place; a chain on another device (or every chain but chain 0, under ERM_FARM_DIAG_REMOTE=1) is
// first compacted into a slab [Tn][nc] on its own device (the same kernel with L = 1), the slab crosses with hipMemcpyPeerAsync, and is gathered from its landing
// copy.  Device memory: the scratch (at most FARM_DIAG_BUDGET), a 1 / L of it twice for the slab and the landing copy, and rank_diag_run's own 256 MB of staged
// draws.  ERM_FARM_DIAG_CHUNK caps the chunk length in columns (the tests of the chunk tails).
template <typename E> struct DiagDevice {
    E* const* eng; int L; bool rank; DevBuf* out;
    DevBuf scratch, land;
    std::vector<DevBuf> slab;       // slab[via[l]]: on the device of chain via[l], the first chain there
    std::vector<int> via;           // -1: chain l is gathered in place
    int dev(int l) const { return eng[l]->cfg.device; }
    hipStream_t s0() const { return eng[0]->work_stream(); }
    int fail(int code, const std::string& msg) const { return ::fail(code, msg); }
    int drain() {
        for (int l = 0; l < L; ++l) { HIPCHK(hipSetDevice(dev(l))); HIPCHK(hipStreamSynchronize(eng[l]->work_stream())); }
        HIPCHK(hipSetDevice(dev(0)));
        return 0;
    }
    int alloc(int64_t wd) {
        for (int q = 0; q < (rank ? 3 : 2); ++q) if (int rc = out[q].try_alloc((size_t)wd * sizeof(double), "the diagnostics")) return rc;
        return 0;
    }
    int fill_nan(int64_t c0, int64_t nc) {
        const std::vector<double> nanv((size_t)nc, std::nan(""));
        for (int q = 0; q < (rank ? 3 : 2); ++q) HIPCHK(hipMemcpyAsync(out[q].as<double>() + c0, nanv.data(), nanv.size() * sizeof(double), hipMemcpyHostToDevice, s0()));
        HIPCHK(hipStreamSynchronize(s0()));
        return 0;
    }
    int estimate(const DiagView& v, int64_t c0, int64_t nc) {
        double* const o[3] = { out[0].as<double>(), out[1].as<double>(), out[2].as<double>() };
        return ::estimate(v, c0, nc, rank, s0(), o);
    }
    int finish() { if (!rank) HIPCHK(hipStreamSynchronize(s0())); return 0; }      // the basic estimator's launches (rank_diag_run drains the stream itself)

    int64_t chunk_cap() const { const char* e = getenv("ERM_FARM_DIAG_CHUNK"); return e ? std::max<long long>(0, atoll(e)) : 0; }
    int gather_begin(int64_t chunk, int Tn, size_t elem) {
        const char* fr = getenv("ERM_FARM_DIAG_REMOTE");
        const bool force_remote = fr && atoi(fr) == 1;
        via.assign(L, -1);
        for (int l = 1; l < L; ++l) if (dev(l) != dev(0) || force_remote) { int d = 1; while (dev(d) != dev(l)) ++d; via[l] = d; }
        slab.resize(L);
        const size_t slab_bytes = (size_t)farm_diag_bytes(chunk, Tn, 1, (int64_t)elem);
        HIPCHK(hipSetDevice(dev(0)));
        if (int rc = scratch.try_alloc((size_t)farm_diag_bytes(chunk, Tn, L, (int64_t)elem), "the farm diagnostics' gathered draws")) return rc;
        for (int l = 1; l < L; ++l) if (via[l] >= 0) {
            if (!land.p) { HIPCHK(hipSetDevice(dev(0))); if (int rc = land.try_alloc(slab_bytes, "the farm diagnostics' slab")) return rc; }
            if (!slab[via[l]].p) { HIPCHK(hipSetDevice(dev(l))); if (int rc = slab[via[l]].try_alloc(slab_bytes, "the farm diagnostics' slab")) return rc; }
        }
        return 0;
    }
    template <typename T> int gather_as(const TraceBlock& b, const FarmDiagChunk& ch, int Tn) {
        const int64_t gx = std::min<int64_t>(std::max<int64_t>(1, (ch.nc / (int64_t)(16 / sizeof(T)) + 255) / 256), 2048);
        const dim3 grid((unsigned)gx, (unsigned)std::min<int64_t>(Tn, std::max<int64_t>(1, 16384 / gx)));
        // rows [nB, nB + Tn) of ch.nc columns at p become chain l of nl in dst
        auto launch = [&](hipStream_t s, const T* p, int64_t ld, int nB, int nl, int l, T* dst) -> int {
            hipLaunchKernelGGL((farm_gather_kernel<T>), grid, dim3(256), 0, s, p, (long long)ld, (long long)ch.nc, Tn, nB, nl, l, dst);
            HIPCHK(hipGetLastError());
            return 0;
        };
        for (int l = 0; l < L; ++l) {
            const auto src = eng[l]->block_src(b);
            const T* p = static_cast<const T*>(src.p) + ch.c0;
            int64_t ld = src.ld; int nB = eng[l]->cfg.n_burnin;
            if (via[l] >= 0) {      // the owner compacts the rows, its stream drains, the slab crosses, the copy completes: gathered from there like a local chain
                T* own = slab[via[l]].template as<T>();
                HIPCHK(hipSetDevice(dev(l)));
                if (int rc = launch(eng[l]->work_stream(), p, ld, nB, 1, 0, own)) return rc;
                HIPCHK(hipStreamSynchronize(eng[l]->work_stream()));
                HIPCHK(hipSetDevice(dev(0)));
                HIPCHK(hipMemcpyPeerAsync(land.p, dev(0), own, dev(l), (size_t)farm_diag_bytes(ch.nc, Tn, 1, (int64_t)sizeof(T)), s0()));
                HIPCHK(hipStreamSynchronize(s0()));
                p = land.as<T>(); ld = ch.nc; nB = 0;
            }
            HIPCHK(hipSetDevice(dev(0)));
            if (int rc = launch(s0(), p, ld, nB, L, l, scratch.as<T>())) return rc;
        }
        return 0;
    }
    int gather(const TraceBlock& b, const FarmDiagChunk& ch, DiagView& v) {
        v.p = scratch.p;
        return v.elem == sizeof(float) ? gather_as<float>(b, ch, v.n_iter) : gather_as<double>(b, ch, v.n_iter);
    }
    int gather_end() {      // the block's scratch and slabs are released once chain 0's stream has read them
        HIPCHK(hipStreamSynchronize(s0()));
        scratch = DevBuf(); land = DevBuf(); slab.clear();
        return 0;
    }
};

// One diagnostics query: the walk, then EITHER checkConvergence's counts on the device (diag_count_kernel through count_converged: 4 of (ess, rhat), or
// { bulk defined, bulk > 400, tail defined, tail > 400, rhat defined, rhat < 1.1 } of (bulk, rhat) and (tail, rhat)) OR the vectors to the caller's arrays, a NULL
// one skipped and a block in device order (CrossQr's nu, row-major N x J) reordered to Julia's vec.  The walk reads the source only; the current device is
// chain 0's after the call, also where a step failed on another chain's device (what it left in flight there is drained when its buffers are released).
template <typename E> static int diag_query(E* const* eng, int L, bool gathered, int which, bool rank, double* const* vec, int64_t* counts)
{
    DevBuf d[3];
    DiagDevice<E> x{eng, L, rank, d};
    if (const int rc = diag_walk(DiagSource<E>{eng, L, gathered}, which, rank, x)) { (void)hipSetDevice(eng[0]->cfg.device); return rc; }
    const int64_t wd = eng[0]->trace_width(which);
    if (counts) {
        int64_t a[4], b[4];
        if (int rc = count_converged(d[0], d[rank ? 2 : 1], wd, x.s0(), a)) return rc;
        if (!rank) { std::copy(a, a + 4, counts); return 0; }
        if (int rc = count_converged(d[1], d[2], wd, x.s0(), b)) return rc;
        const int64_t c6[6] = { a[0], a[1], b[0], b[1], a[2], a[3] };
        std::copy(c6, c6 + 6, counts);
        return 0;
    }
    for (int q = 0; q < (rank ? 3 : 2); ++q) if (vec[q]) {
        HIPCHK(hipMemcpy(vec[q], d[q].p, (size_t)wd * sizeof(double), hipMemcpyDeviceToHost));
        for (const TraceBlock& b : eng[0]->trace_blocks(which)) if (b.device_order()) {
            const std::vector<double> h(vec[q] + b.col0, vec[q] + b.col0 + b.ncol);
            rows_to_cols(h.data(), vec[q] + b.col0, eng[0]->cfg.n_subj, (int64_t)eng[0]->cfg.n_item);
        }
    }
    return 0;
}
static int diag_query(erm_handle h, int which, bool rank, double* const* vec, int64_t* counts)
{
    EngineBase* e = h->e.get();
    return diag_query(&e, 1, false, which, rank, vec, counts);
}
static int diag_query(erm_farm_handle f, int which, bool rank, double* const* vec, int64_t* counts)
{
    std::vector<EngineBase*> chains;
    for (auto& e : f->eng) chains.push_back(e->e.get());
    return diag_query(chains.data(), (int)chains.size(), true, which, rank, vec, counts);
}

// erm_debug_diagnostics / erm_debug_rank_diagnostics: caller-supplied draws through the same query, as an engine whose one trace is one resident subject-level
// block of n_col columns in precision T (debug_upload), on the NULL stream
struct UploadedDraws {
    erm_config cfg{}; int64_t rows_done = 0;
    const void* p = nullptr; size_t elem = 0;
    int64_t trace_width(int) const { return cfg.n_subj; }
    TraceBlocks trace_blocks(int) const { TraceBlocks t; t.add(BLK_SUBJECT, cfg.n_subj, SUBJ_THETA); return t; }
    EngineBase::BlockSrc block_src(const TraceBlock&) const { return { p, cfg.n_subj, elem }; }
    hipStream_t work_stream() const { return nullptr; }
};
static int debug_query(int device, int precision, const double* x, int64_t n_draw, int64_t n_col, int32_t n_chain, bool rank, double* const* vec)
{
    if (!x || n_draw <= 0 || n_col <= 0 || n_draw > 0x7fffffff) return fail(ERM_ERR_ARG, "bad x / n_draw / n_col");
    if (precision != ERM_PREC_F32 && precision != ERM_PREC_F64) return fail(ERM_ERR_ARG, "unknown precision");
    if (const std::string no = diag_limits(rank, n_draw, n_chain); !no.empty()) return fail(ERM_ERR_ARG, no);
    const int64_t len = n_draw * n_col * n_chain;
    for (int64_t e = 0; e < len; ++e) if (x[e] != x[e]) return fail(ERM_ERR_NONFINITE, "x holds a NaN at entry " + std::to_string(e));
    HIPCHK(hipSetDevice(device));
    DevBuf dTr;
    if (int rc = precision == ERM_PREC_F32 ? debug_upload<float>(x, n_draw, n_col, n_chain, dTr) : debug_upload<double>(x, n_draw, n_col, n_chain, dTr)) return rc;
    UploadedDraws u;
    u.cfg.device = device; u.cfg.n_subj = n_col; u.cfg.n_iter = (int32_t)n_draw; u.cfg.n_chain = n_chain; u.cfg.trace_mode = ERM_TRACE_FULL;
    u.rows_done = n_draw * n_chain; u.p = dTr.p; u.elem = precision == ERM_PREC_F32 ? sizeof(float) : sizeof(double);
    UploadedDraws* e = &u;
    return diag_query(&e, 1, false, ERM_TRACE_RA, rank, vec, nullptr);
}
#endif  // __HIPCC__

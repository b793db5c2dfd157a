// ertirt.hip -- C-ABI host implementation of libertirt.so (declared in include/ertirt.h).
// Build: hipcc --offload-arch=gfx950 -O3 -std=c++17 -shared -fPIC -I include ertirt.hip -o libertirt.so
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>      // types only: the library is bound at run time (dlopen) and only by subject-sharded chains
#include <dlfcn.h>
#include <chrono>
#include <condition_variable>
#include <functional>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <cstdlib>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <type_traits>
#include <vector>
#include "ertirt.h"
#include "erm_kernels.hpp"
#include "erm_predictive_kernels.hpp"      // posterior predictive checks: the replicate pass behind every sweep
#include "erm_rank_diag_kernels.hpp"       // rank-normalised convergence diagnostics: bulk / tail ESS, rank R-hat
#include "erm_marginal_kernels.hpp"        // marginal WAIC: theta and zeta integrated out, from the item trace
#include "erm_psis_kernels.hpp"            // marginal PSIS-LOO: Pareto-smoothed leave-one-subject-out from marginal_kernel's l
#include "erm_score_kernels.hpp"           // scores of respondents: posterior moments of theta and zeta, from the item trace
#include "erm_fit_kernels.hpp"             // person fit: lz and the response-time chi^2 of every respondent, from the item trace
#include "erm_ifit_kernels.hpp"            // item fit and drift: infit, outfit and the signed residuals of every item, from the item trace
#include "erm_pv_kernels.hpp"              // plausible values: draws of theta and zeta from each subject's posterior, from the item trace
#include "erm_farm_diag.hpp"               // the chain farm's joint diagnostics: chunk arithmetic
#include "erm_geometry.hpp"
#include "erm_model.hpp"
#include "erm_schedule.hpp"

using namespace erm;

namespace {

thread_local std::string g_err;
int fail(int code, const std::string& msg) { g_err = msg; return code; }

#define HIPCHK(expr)                                                                                     \
    do {                                                                                                 \
        hipError_t e__ = (expr);                                                                         \
        if (e__ != hipSuccess) {                                                                         \
            return fail(ERM_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e__));                \
        }                                                                                                \
    } while (0)

// RCCL, bound lazily: libertirt.so has no link-time communication dependency.  A process that already loaded RCCL (torch does)
// gets that same copy back from dlopen by soname.
struct Rccl {
    void* lib = nullptr;
    ncclResult_t (*GetUniqueId)(ncclUniqueId*) = nullptr;
    ncclResult_t (*CommInitRank)(ncclComm_t*, int, ncclUniqueId, int) = nullptr;
    ncclResult_t (*AllGather)(const void*, void*, size_t, ncclDataType_t, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*AllReduce)(const void*, void*, size_t, ncclDataType_t, ncclRedOp_t, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*CommInitAll)(ncclComm_t*, int, const int*) = nullptr;
    ncclResult_t (*GroupStart)() = nullptr;
    ncclResult_t (*GroupEnd)() = nullptr;
    ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
    ncclResult_t (*CommCount)(const ncclComm_t, int*) = nullptr;
    const char* (*GetErrorString)(ncclResult_t) = nullptr;
    std::mutex mu;
    int load() {
        std::lock_guard<std::mutex> lock(mu);      // engines of several host threads may shard at the same time
        if (lib) return 0;
        const char* env = getenv("ERM_RCCL_LIB");
        const char* names[] = {env, "librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"};
        for (const char* n : names) { if (n && (lib = dlopen(n, RTLD_NOW | RTLD_LOCAL))) break; }
        if (!lib) return fail(ERM_ERR_STATE, std::string("cannot load RCCL: ") + dlerror());
        GetUniqueId = reinterpret_cast<decltype(GetUniqueId)>(dlsym(lib, "ncclGetUniqueId"));
        CommInitRank = reinterpret_cast<decltype(CommInitRank)>(dlsym(lib, "ncclCommInitRank"));
        AllGather = reinterpret_cast<decltype(AllGather)>(dlsym(lib, "ncclAllGather"));
        AllReduce = reinterpret_cast<decltype(AllReduce)>(dlsym(lib, "ncclAllReduce"));
        CommInitAll = reinterpret_cast<decltype(CommInitAll)>(dlsym(lib, "ncclCommInitAll"));
        GroupStart = reinterpret_cast<decltype(GroupStart)>(dlsym(lib, "ncclGroupStart"));
        GroupEnd = reinterpret_cast<decltype(GroupEnd)>(dlsym(lib, "ncclGroupEnd"));
        CommDestroy = reinterpret_cast<decltype(CommDestroy)>(dlsym(lib, "ncclCommDestroy"));
        CommCount = reinterpret_cast<decltype(CommCount)>(dlsym(lib, "ncclCommCount"));
        GetErrorString = reinterpret_cast<decltype(GetErrorString)>(dlsym(lib, "ncclGetErrorString"));
        if (!GetUniqueId || !CommInitRank || !AllGather || !CommDestroy || !CommCount || !GetErrorString || !AllReduce || !CommInitAll || !GroupStart || !GroupEnd) { lib = nullptr; return fail(ERM_ERR_STATE, "RCCL library lacks an expected symbol"); }
        return 0;
    }
};
Rccl g_rccl;
#define RCCLCHK(expr)                                                                                    \
    do {                                                                                                 \
        ncclResult_t r__ = (expr);                                                                       \
        if (r__ != ncclSuccess) return fail(ERM_ERR_STATE, std::string(#expr) + ": " + g_rccl.GetErrorString(r__)); \
    } while (0)

// host -> device, complete on return for EVERY stream: the copy runs on the NULL stream, with which the engines' non-blocking streams are not ordered
#define H2D(dst, src, n) do { HIPCHK(hipMemcpy((dst), (src), (n), hipMemcpyHostToDevice)); HIPCHK(hipStreamSynchronize(nullptr)); } while (0)
struct DevBuf {
    void* p = nullptr; size_t bytes = 0;
    DevBuf() = default;
    DevBuf(DevBuf&& o) noexcept : p(o.p), bytes(o.bytes) { o.p = nullptr; o.bytes = 0; }
    DevBuf& operator=(DevBuf&& o) noexcept { std::swap(p, o.p); std::swap(bytes, o.bytes); return *this; }      // (o's destructor frees what this held)
    ~DevBuf() { if (p) (void)hipFree(p); }
    int alloc(size_t n) {
        if (p) { (void)hipFree(p); p = nullptr; }
        bytes = n;
        if (n == 0) return 0;
        HIPCHK(hipMalloc(&p, n));
        // hipMemset on device memory is asynchronous with respect to the host and runs on the NULL stream, with which the engines' non-blocking
        // streams are not ordered: a kernel enqueued next on an engine stream could write the buffer before (and be wiped by) the fill.  Seen as
        // a farm chain whose data constants were off about once in 500 runs, with three host threads in erm_set_data at once.
        HIPCHK(hipMemset(p, 0, n));
        HIPCHK(hipStreamSynchronize(nullptr));
        return 0;
    }
    // n bytes WITHOUT the zero fill, for a buffer that is staged and then moved into place: out of memory is ERM_ERR_NOMEM (the HIP error consumed), and what
    // this held is released only once the new memory exists
    int try_alloc(size_t n, const char* what) {
        void* q = nullptr;
        if (n > 0 && hipMalloc(&q, n) != hipSuccess) { (void)hipGetLastError(); return fail(ERM_ERR_NOMEM, std::string("out of device memory for ") + what + " (" + std::to_string(n) + " bytes)"); }
        if (p) (void)hipFree(p);
        p = q; bytes = n;
        return 0;
    }
    template <typename T> T* as() const { return reinterpret_cast<T*>(p); }
};

// checkConvergence's four counts (diag_count_kernel, the reference's thresholds ESS > 400 and R-hat < 1.1) of n device-resident ess / rhat values: the one place
// that launches the kernel, for the diagnostics' counts (erm_diagnostics.hpp) and for erm_debug_convergence
static int count_converged(const DevBuf& dE, const DevBuf& dR, int64_t n, hipStream_t stream, int64_t* c4)
{
    DevBuf dC;
    if (int rc = dC.alloc(4 * sizeof(unsigned long long))) return rc;
    hipLaunchKernelGGL(diag_count_kernel, dim3((unsigned)std::min<int64_t>((n + 255) / 256, 1024)), dim3(256), 0, stream, dE.as<double>(), dR.as<double>(), (long long)n, 400.0, 1.1,
                       dC.as<unsigned long long>());
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(stream));
    unsigned long long h[4];
    HIPCHK(hipMemcpy(h, dC.p, sizeof(h), hipMemcpyDeviceToHost));
    for (int k = 0; k < 4; ++k) c4[k] = (int64_t)h[k];
    return 0;
}

// Rank-normalised diagnostics (erm_rank_diag_kernels.hpp), the one place that launches the kernels (its caller and its limits: erm_diagnostics.hpp):
// columns [0, ncol) of the trace tr ([row = m nChain + l][ld]) -> bulk / tail / rhat[0 .. ncol), in chunks of columns whose staged draws fit the scratch budget
// (256 MB whatever the trace width; ERM_RANK_DIAG_CHUNK: a chunk length in columns, for the tests of the chunk tails)
template <typename T>
static int rank_diag_run(const T* tr, int64_t ld, int64_t ncol, int nChain, int nBurnin, int Tn, hipStream_t stream, double* bulk, double* tail, double* rhat)
{
    const int n = Tn / 2, M = 2 * nChain, S = M * n, P = rk_pad(S);
    int64_t chunk = std::max<int64_t>(1, ((int64_t)256 << 20) / ((int64_t)S * (int64_t)sizeof(double)));
    if (const char* e = getenv("ERM_RANK_DIAG_CHUNK")) { const long long v = atoll(e); if (v > 0) chunk = std::min<int64_t>(chunk, v); }
    chunk = std::min(chunk, ncol);
    DevBuf scratch;
    if (int rc = scratch.try_alloc((size_t)chunk * S * sizeof(double), "the rank diagnostics' staged draws")) return rc;
    const size_t lds = (size_t)P * 10 + (size_t)S * 8;
    HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(&rank_diag_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    for (int64_t c0 = 0; c0 < ncol; c0 += chunk) {
        const int64_t nc = std::min(chunk, ncol - c0);
        hipLaunchKernelGGL((rank_stage_kernel<T>), dim3((unsigned)((nc + 31) / 32), (unsigned)((S + 31) / 32)), dim3(256), 0, stream, tr + c0, (long long)ld, (long long)nc, nChain, nBurnin,
                           Tn, n, S, scratch.as<double>());
        hipLaunchKernelGGL(rank_diag_kernel, dim3((unsigned)nc), dim3(RK_THREADS), lds, stream, scratch.as<double>(), M, n, P, bulk + c0, tail + c0, rhat + c0);
        HIPCHK(hipGetLastError());
    }
    HIPCHK(hipStreamSynchronize(stream));
    return 0;
}

// WAIC's totals from per-unit accumulators (erm_pointwise.hpp) on the device: the one place that launches pointwise_finish_kernel -- for erm_get_waic /
// erm_get_pointwise (the accumulators the pass behind the sweep fills) and for the marginal WAIC (those marginal_kernel fills).
// one launch of the finish kernel; sums[0..4]: its columns added over the workgroups in order
static int pw_finish_on(const double2* acc_ms, const double2* acc_w, int64_t U, int64_t n, double center, double* lppd_out, double* p_out, hipStream_t stream, double* sums)
{
    const int nb = (int)std::min<int64_t>(1024, (U + 255) / 256);
    DevBuf dPart;
    if (int rc = dPart.alloc((size_t)nb * PW_FIN_COLS * sizeof(double))) return rc;
    PwFinArgs a{};
    a.acc_ms = acc_ms; a.acc_w = acc_w; a.U = U; a.n = n; a.center = center;
    a.lppd_out = lppd_out; a.p_out = p_out; a.part = dPart.as<double>();
    hipLaunchKernelGGL(pointwise_finish_kernel, dim3(nb), dim3(256), 0, stream, a);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(stream));
    std::vector<double> part((size_t)nb * PW_FIN_COLS);
    HIPCHK(hipMemcpy(part.data(), dPart.p, part.size() * sizeof(double), hipMemcpyDeviceToHost));
    for (int q = 0; q < PW_FIN_COLS; ++q) { double t = 0.0; for (int b = 0; b < nb; ++b) t += part[(size_t)b * PW_FIN_COLS + q]; sums[q] = t; }
    return 0;
}
// out8 of erm_get_waic: two launches (the sums, then the squared deviations of elpd_u from its mean over the units)
static int pw_totals(const double2* acc_ms, const double2* acc_w, int64_t units, int64_t n, hipStream_t stream, double* out8)
{
    const double U = (double)units;
    double s0[PW_FIN_COLS], s1[PW_FIN_COLS];
    if (int rc = pw_finish_on(acc_ms, acc_w, units, n, 0.0, nullptr, nullptr, stream, s0)) return rc;
    if (int rc = pw_finish_on(acc_ms, acc_w, units, n, s0[2] / U, nullptr, nullptr, stream, s1)) return rc;
    const double var_u = U > 1.0 ? s1[3] / (U - 1.0) : 0.0;
    out8[0] = s0[2]; out8[1] = s0[1]; out8[2] = -2.0 * s0[2]; out8[3] = 2.0 * std::sqrt(U * var_u);
    out8[4] = s0[0]; out8[5] = U; out8[6] = (double)n; out8[7] = s0[4];
    return 0;
}

// A persistent launch needs all its workgroups resident at once.  Two persistent launches of ONE process on one device (a farm's chains sharing a
// device, several engines) could each hold some compute units and wait for the other's for ever: they take turns.
std::mutex g_persist_mu[64];

struct ItemSource;      // erm_item_pass.hpp
struct EngineBase {
    erm_config cfg{};
    virtual ~EngineBase() {}
    virtual int init() = 0;
    virtual int set_data(const uint8_t*, const double*, const double*) = 0;
    virtual int set_state(const erm_state*) = 0;
    virtual int get_state(erm_state*) = 0;
    virtual int run(int64_t) = 0;
    virtual int get_trace(int, double*) = 0;
    virtual int get_item_trace(double*) = 0;
    virtual int get_mean(erm_state*) = 0;
    virtual int get_dic(double*) = 0;
    // WAIC (erm_set_pointwise / erm_get_waic / erm_pointwise_units / erm_get_pointwise)
    virtual int set_pointwise(int unit) = 0;
    virtual int get_waic(double* out8) = 0;
    virtual int64_t pointwise_units() const = 0;
    virtual int get_pointwise(double* lppd_u, double* p_u) = 0;
    // the passes over the item trace (erm_item_pass.hpp: marginal WAIC and LOO, scores, plausible values, person fit, item fit): this engine's resident data set as the source of `pass`,
    // or the refusal in the pass's words; S.rows == NULL: with its own post-burn-in rows, read in place (the farm hands chain 0 a table of the rows of all chains
    // on its device).  And the resident item trace.
    virtual int item_source(int pass, ItemSource& S) = 0;
    virtual const double* item_trace_dev() const = 0;
    // posterior predictive checks (erm_set_predictive / erm_predictive_reps / erm_get_predictive)
    virtual int set_predictive(int on, int32_t thin) = 0;
    virtual int64_t predictive_reps() const = 0;
    virtual int get_predictive(double* item, double* subj, double* total) = 0;
    virtual int set_seed(uint64_t) = 0;
    // DIC pieces for the chain farm: the log-likelihood at sum * inv (sum: a device vector in the summary layout) and the sum of the recorded logLike rows
    virtual int loglik_at(const double* dsum, double inv, double* ll) = 0;
    virtual int ll_trace_sum(double* out) = 0;
    virtual int simulate_data(const erm_state*, uint64_t, int) = 0;
    virtual int get_data(uint8_t*, double*, double*) = 0;
    virtual int get_truth(double*, double*) = 0;
    virtual int reset_trace() = 0;
    virtual int set_shard(int, int, int64_t, int64_t, erm_exchange_fn, void*, const void*) = 0;
    // Post.mean and DIC, of one engine and of a chain farm (erm_farm_*): this chain's post-burn-in SUMS [item-level trace columns | theta | zeta | nu] added into
    // `acc` (device memory of this engine's device, summary_len() doubles; only the subject-level blocks `want` names, all of them if NULL), and the inverse step
    // from the accumulated sums to the fields of an erm_state
    virtual int64_t summary_len() const = 0;
    virtual int summary_add(double* acc, const erm_state* want) = 0;
    virtual int mean_from_summary(const double* dacc, double inv, erm_state* out) = 0;
    // The convergence diagnostics (erm_diagnostics.hpp) read an engine's and every farm chain's resident trace blocks in place: the device address of row 0 of the
    // block's first column, the row stride in elements and the element size (the engine's trace type for a subject-level block, double for an item-level one);
    // p = NULL: the block is not resident (ERM_TRACE_SUMMARY, CrossQr's nu block beyond its budget, BLK_ZERO).  And the stream the chain's kernels run on.
    struct BlockSrc { const void* p; int64_t ld; size_t elem; };
    virtual BlockSrc block_src(const TraceBlock& b) const = 0;
    virtual hipStream_t work_stream() const = 0;
    int64_t rows_done = 0;
    int64_t post_rows = 0;
    erm_timing timing{};
    // the per-model facts and every width that follows from them: one table (erm_model.hpp)
    ModelTraits mt() const { return model_traits(cfg.model); }
    int64_t trace_width(int which) const { return erm::trace_width(cfg.model, which, cfg.n_subj, cfg.n_item, cfg.n_feat); }
    TraceBlocks trace_blocks(int which) const { return erm::trace_blocks(cfg.model, which, cfg.n_subj, cfg.n_item, cfg.n_feat); }
    int nq() const { return erm::nq(cfg.model, cfg.n_item, cfg.n_feat); }
    int nbeta() const { return erm::nbeta(cfg.model, cfg.n_feat); }
    int64_t nu_len() const { return erm::nu_len(cfg.model, cfg.n_subj, cfg.n_item); }
    int64_t item_trace_width() const { return erm::item_trace_width(cfg.model, cfg.n_item, cfg.n_feat); }
};

// getDic's four numbers {Dbar, Dhat, pD, DIC} from the accumulated summary `dacc` of `rows` post-burn-in rows (on eng[0]'s device, which evaluates the
// log-likelihood at the mean) and the logLike rows of the n chains
int dic_from_summary(EngineBase* const* eng, size_t n, const double* dacc, int64_t rows, double* out4)
{
    double ll_hat = 0.0;
    if (int rc = eng[0]->loglik_at(dacc, 1.0 / (double)rows, &ll_hat)) return rc;
    double ll_sum = 0.0; int64_t ll_rows = 0;
    for (size_t l = 0; l < n; ++l) { double t = 0.0; if (int rc = eng[l]->ll_trace_sum(&t)) return rc; ll_sum += t; ll_rows += eng[l]->rows_done; }
    if (ll_rows <= 0) return fail(ERM_ERR_STATE, "no sweeps recorded");
    const double Dhat = -2.0 * ll_hat, Dbar = -2.0 * ll_sum / (double)ll_rows;
    out4[0] = Dbar; out4[1] = Dhat; out4[2] = Dbar - Dhat; out4[3] = Dbar + (Dbar - Dhat);
    return 0;
}

constexpr const ParField<erm_state> (&FIELDS)[N_PAR_FIELDS] = PAR_FIELDS<erm_state>;      // the parameter block's item-level fields (erm_model.hpp)

template <typename real> struct Engine : EngineBase {
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    std::vector<hipEvent_t> pass_ev;
    int cu_count = 256;
    int64_t N = 0; int J = 0, F = 0, Fk = 0;   // Fk = covariate columns the kernels see (0 for CrossQr)
    int64_t rows_cap = 0;
    bool has_data = false;
    Geom G;                                          // launch geometry and LDS layout: decided by plan_geometry (erm_geometry.hpp) and nowhere else, read in place
    uint32_t sweeps_total = 0;

    DevBuf dY, dC, dOmega, dNu, dX, dTheta, dZeta, dCst, dSlab0, dSlab1, dGslab1, dGcnt;
    // double-buffered: a fused sweep kernel reads [cur] and writes [1 - cur] (parameter block, counters, group-reduced statistics)
    DevBuf dParB[2], dCtlB[2], dGslab0B[2];
    DevBuf dDbgTs;                                   // ERM_TIMELINE diagnostics
    DevBuf dXbuf;                                    // persistent launches: packet rows of the statistics exchange
    DevBuf dSnap;                                    // persistent launches: the state saved before an erm_run (restored if the launch times out: run())
    bool snap_stats_valid = false;
    int persist_fault_countdown = 0;                 // ERM_FLAG_TEST_PERSIST_TIMEOUT: the engine's SECOND persistent erm_run loses a statistics row (the first leaves rows and sums for the restore to keep)
    uint32_t xtag = 0;                               // last packet tag handed out (tags only grow; the buffer is cleared before they wrap)
    int cur = 0;
    // subject sharding (erm_set_shard): this device holds subjects [row_base, row_base + N) of n_total
    int shard_rank = 0, shard_count = 1;
    int64_t n_total = 0, row_base = 0;
    erm_exchange_fn exch = nullptr; void* exch_user = nullptr;     // the caller's all-gather (host-synchronous) ...
    ncclComm_t comm = nullptr;                                       // ... or RCCL enqueued on the engine's stream
    DevBuf dShardSend, dShardRecv[2];
    bool sharded() const { return exch != nullptr || comm != nullptr; }
    // small data sets: ONE launch per erm_run (pass_kernel<..., PERSIST>: the statistics rows cross between its sweeps as tagged packets).  Starts as G.persist and is
    // the one geometry fact kept outside G: it changes after planning (the occupancy check, erm_set_shard, a pass behind the sweep, a time-out)
    bool persist = false;
    bool fused() const { return !m_cq() && G.fused; }  // single-pass models run the tiny step inside the row-pass kernel (G.fused is false when its LDS layout cannot fit: very long tests)
    DevBuf dSumTheta, dSumZeta, dSumNu, dTrTheta, dTrZeta, dTrNu, dTrItem, dTrLl;
    const DevBuf& subj_trace(int64_t which) const { return which == SUBJ_THETA ? dTrTheta : which == SUBJ_ZETA ? dTrZeta : dTrNu; }      // a TraceBlock's `src`
    // WAIC (erm_set_pointwise): the unit, the accumulators {m, s}[units] and {mean, m2}[units] (erm_pointwise.hpp), GibbsRtIrtCrossQr's copy of nu_t
    // (taken ahead of pass B of every sweep, which overwrites nu_t with nu_{t+1}: N * J values of the engine's cell type)
    int pw_unit = PW_OFF;
    DevBuf dPwMs, dPwW, dNuSnap;
    // posterior predictive checks (erm_set_predictive): every pred_thin-th post-burn-in row is a replicate row (0 = off); the accumulators of the subjects
    // [N][PRED_SUBJ], of the items and the data set [J][PRED_ITEM] | [PRED_TOT] | replicate counter, and the workgroups' slab rows (erm_predictive_kernels.hpp)
    int32_t pred_thin = 0;
    DevBuf dPredSubj, dPredItem, dPredSlab;
    bool aux_pass() const { return pw_unit != PW_OFF || pred_thin > 0; }      // a pass of its own follows every sweep
    bool persist_avail = false;                       // the persistent schedule as init() / erm_set_shard / a time-out left it: an engine with a pass behind the sweep plans
                                                      // per-sweep launches at the same geometry (as ERM_FLAG_NO_PERSIST does) and returns to it when the last pass is turned off
    // the one place that decides `persist`: a persistent launch cannot interleave another kernel between its sweeps
    void set_persist_avail(bool avail) { persist_avail = avail; persist = avail && !aux_pass(); timing.persistent = persist ? 1 : 0; }

    ~Engine() override {
        drop_graphs();
        if (comm) (void)g_rccl.CommDestroy(comm);
        for (auto e : pass_ev) (void)hipEventDestroy(e);
        if (host_ctl) (void)hipHostFree(host_ctl);
        if (host_run) (void)hipHostFree(host_run);
        if (ev0) (void)hipEventDestroy(ev0);
        if (ev1) (void)hipEventDestroy(ev1);
        if (stream) (void)hipStreamDestroy(stream);
    }

    bool is_rt() const { return mt().rt; }
    bool m_cq() const { return mt().rho; }                // the cross-relation models: two row passes per sweep
    bool m_nu() const { return mt().nu != NU_NONE; }
    int p() const { return Fk + 1; }
    // calls f(std::integral_constant<int, MODEL>) for the configured model: with the range check in init() the one place that names the models (the rest
    // reads erm_model.hpp's table, which is indexed by erm::Model -- the same numbers, as is asserted here)
    static_assert(MLIRT == ERM_MODEL_MLIRT && RTIRT == ERM_MODEL_RTIRT && CROSSQR == ERM_MODEL_CROSSQR && LATENTQR == ERM_MODEL_LATENTQR && NULLM == ERM_MODEL_NULL &&
                  CROSS == ERM_MODEL_CROSS && LATENT == ERM_MODEL_LATENT, "erm::Model and ERM_MODEL_* number the models differently");
    static_assert(TRACE_RA == ERM_TRACE_RA && TRACE_RT == ERM_TRACE_RT && TRACE_QR == ERM_TRACE_QR && TRACE_LOGLIKE == ERM_TRACE_LOGLIKE, "erm::Trace and ERM_TRACE_* differ");
    template <typename Fn> int dispatch(Fn&& f) {
        switch (cfg.model) {
        case ERM_MODEL_MLIRT: return f(std::integral_constant<int, MLIRT>{});
        case ERM_MODEL_RTIRT: return f(std::integral_constant<int, RTIRT>{});
        case ERM_MODEL_CROSSQR: return f(std::integral_constant<int, CROSSQR>{});
        case ERM_MODEL_LATENTQR: return f(std::integral_constant<int, LATENTQR>{});
        case ERM_MODEL_NULL: return f(std::integral_constant<int, NULLM>{});
        case ERM_MODEL_CROSS: return f(std::integral_constant<int, CROSS>{});
        case ERM_MODEL_LATENT: return f(std::integral_constant<int, LATENT>{});
        }
        return fail(ERM_ERR_ARG, "unknown model");
    }
    // LatentQr with sigp_mode 1 also accumulates the 1/nu-weighted Gram entries of [1 X theta | u]
    int ngx() const {
        if (mt().nu != NU_SUBJECT || cfg.sigp_mode != 1) return 0;      // (one weight per subject: of the seven models that is LatentQr alone)
        const int q = p() + 1;
        return q * (q + 1) / 2 + q + 1;
    }
    DevBuf dPgTab;                                   // the Polya-Gamma proposal table [PG_NBIN][4] (erm_rng.hpp, pg_bin)

    int init() override {
        N = cfg.n_subj; J = cfg.n_item; F = cfg.n_feat;
        Fk = kernel_feat(cfg.model, F);
        if (N <= 0 || J <= 0 || F < 0) return fail(ERM_ERR_ARG, "n_subj, n_item must be positive and n_feat non-negative");
        if (N >= (1LL << 32)) return fail(ERM_ERR_ARG, "n_subj must fit 32 bits");
        if (cfg.model < 0 || cfg.model > ERM_MODEL_LATENT) return fail(ERM_ERR_ARG, "unknown model");
        if (Fk + 2 > PMAX) return fail(ERM_ERR_ARG, "n_feat too large (max " + std::to_string(PMAX - 2) + ")");
        if (J > 896) return fail(ERM_ERR_ARG, "n_item too large (max 896)");
        if (m_nu() && !(cfg.q_rt > 0.0 && cfg.q_rt < 1.0))
            return fail(ERM_ERR_ARG, "qRt must be between 0 and 1");   // @assert at src/Draw.pl.jl:476
        if (cfg.n_iter < 0 || cfg.n_chain < 1 || cfg.n_burnin < 0) return fail(ERM_ERR_ARG, "bad n_iter / n_chain / n_burnin");
        if (cfg.sigp_mode != 0 && cfg.sigp_mode != 1) return fail(ERM_ERR_ARG, "sigp_mode must be 0 or 1");
        if (cfg.chain_id < 0 || cfg.chain_id > 255) return fail(ERM_ERR_ARG, "chain_id must be in [0, 255] (the random streams carry eight bits of it: chain 256 would replay chain 0)");
        if (cfg.flags & ~(int32_t)ERM_FLAG_ALL) return fail(ERM_ERR_ARG, "unknown bits in erm_config.flags (built against another version of ertirt.h? erm_abi_version() = " + std::to_string(ERM_ABI_VERSION) + ")");
        if (!(cfg.nu_trace_max_gb >= 0.0) || !std::isfinite(cfg.nu_trace_max_gb)) return fail(ERM_ERR_ARG, "nu_trace_max_gb must be finite and non-negative (0 = the default)");
        if (cfg.precision != ERM_PREC_F32 && cfg.precision != ERM_PREC_F64) return fail(ERM_ERR_ARG, "unknown precision");
        if (cfg.trace_mode != ERM_TRACE_SUMMARY && cfg.trace_mode != ERM_TRACE_FULL) return fail(ERM_ERR_ARG, "unknown trace_mode");
        HIPCHK(hipSetDevice(cfg.device));
        hipDeviceProp_t prop;
        HIPCHK(hipGetDeviceProperties(&prop, cfg.device));
        cu_count = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
        HIPCHK(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
        HIPCHK(hipEventCreate(&ev0));
        HIPCHK(hipEventCreate(&ev1));
        HIPCHK(hipHostMalloc(reinterpret_cast<void**>(&host_ctl), 4 * sizeof(Ctl), hipHostMallocDefault));      // [1], [2]: the two device copies of the counters, [3]: a persistent launch's time-out word -- written by run_end_kernel
        HIPCHK(hipHostGetDevicePointer(reinterpret_cast<void**>(&host_ctl_dev), host_ctl, 0));
        HIPCHK(hipHostMalloc(reinterpret_cast<void**>(&host_run), sizeof(RunParams), hipHostMallocDefault));      // an erm_run's parameters, read by run_begin_kernel
        HIPCHK(hipHostGetDevicePointer(reinterpret_cast<void**>(&host_run_dev), host_run, 0));

        // ---- geometry (pure host function, CPU-tested: erm_geometry.hpp)
        {
            GeomIn gi;
            gi.model = cfg.model; gi.f64 = sizeof(real) == 8; gi.N = N; gi.J = J; gi.Fk = Fk; gi.ngx = ngx();
            gi.lanes_per_row = cfg.lanes_per_row; gi.block_threads = cfg.block_threads; gi.grid_blocks = cfg.grid_blocks;
            gi.cu_count = cu_count; gi.no_fuse = (cfg.flags & ERM_FLAG_NO_FUSE) != 0;
            std::string msg;
            // small data sets (the reference's own sizes): few, full workgroups and ONE persistent launch per erm_run -- decided by the planner
            gi.no_persist = (cfg.flags & ERM_FLAG_NO_PERSIST) != 0;
#ifdef ERM_DIAG_BUILD
            gi.no_persist = true;                       // the stage-timing early exits would strand the other workgroups polling for a row that never comes
#endif
            if (plan_geometry(gi, G, msg) != 0) return fail(ERM_ERR_ARG, msg);
            set_persist_avail(G.persist);
        }

        // ---- device memory
        rows_cap = (int64_t)cfg.n_iter * cfg.n_chain;
        const size_t NJ = (size_t)N * J;
        int rc = 0;
        rc |= dY.alloc(NJ);
        rc |= dOmega.alloc(NJ * sizeof(real));
        if (is_rt()) rc |= dC.alloc(NJ * sizeof(real));
        rc |= dNu.alloc((size_t)nu_len() * sizeof(real));
        if (Fk > 0) rc |= dX.alloc((size_t)N * Fk * sizeof(real));
        rc |= dTheta.alloc((size_t)N * sizeof(real));
        rc |= dZeta.alloc((size_t)N * sizeof(real));
        for (int k = 0; k < 2; ++k) rc |= dParB[k].alloc((size_t)par_size(J) * sizeof(double));
        rc |= dCst.alloc((size_t)cst_size(J) * sizeof(double));
        rc |= dSlab0.alloc((size_t)G.grid_blocks * G.ns[0] * sizeof(double));
        // (at least GROUP rows, zero-filled: the fused head requests its first GROUP group rows unconditionally and masks those beyond n_groups)
        for (int k = 0; k < 2; ++k) rc |= dGslab0B[k].alloc((size_t)std::max(G.n_groups, GROUP) * G.ns[0] * sizeof(double));
        rc |= dGcnt.alloc(((size_t)2 * G.n_groups + 4) * sizeof(unsigned int));       // group tickets | a persistent launch's time-out flag, wait bound (ticks), test hook, pad
        if (persist) {      // packet rows of the persistent launch's statistics exchange: [parity][workgroup][2 * ns] 64-bit packets, tags start at 1
            rc |= dXbuf.alloc((size_t)2 * G.grid_blocks * 2 * G.ns[0] * sizeof(unsigned long long));
            if (!rc) HIPCHK(hipMemset(dXbuf.p, 0, dXbuf.bytes));
        }
        if (persist) rc |= dSnap.alloc(snap_bytes());
        if (m_cq()) { rc |= dSlab1.alloc((size_t)G.grid_blocks * G.ns[1] * sizeof(double)); rc |= dGslab1.alloc((size_t)std::max(G.n_groups, GROUP) * G.ns[1] * sizeof(double)); }      // >= GROUP rows: see dGslab0B
        for (int k = 0; k < 2; ++k) rc |= dCtlB[k].alloc(sizeof(Ctl));
        rc |= dSumTheta.alloc((size_t)N * sizeof(double));
        rc |= dSumZeta.alloc((size_t)N * sizeof(double));
        rc |= dSumNu.alloc((size_t)nu_len() * sizeof(double));
        rc |= dTrItem.alloc((size_t)std::max<int64_t>(rows_cap, 1) * item_trace_width() * sizeof(double));
        rc |= dTrLl.alloc((size_t)std::max<int64_t>(rows_cap, 1) * sizeof(double));
        if (cfg.trace_mode == ERM_TRACE_FULL && rows_cap > 0) {
            rc |= dTrTheta.alloc((size_t)rows_cap * N * sizeof(real));
            if (is_rt()) rc |= dTrZeta.alloc((size_t)rows_cap * N * sizeof(real));
            if (mt().nu == NU_SUBJECT) rc |= dTrNu.alloc((size_t)rows_cap * N * sizeof(real));
            if (mt().nu == NU_CELL) {
                // Post.qr of GibbsRtIrtCrossQr carries vec(nu) (N*J values) per sweep (src/GibbsRtIrtCross.pl.jl:65,296): kept on the device
                // when it fits the budget (erm_config.nu_trace_max_gb, default 16 GiB), otherwise only nu's running mean is available
                const double cap_gb = cfg.nu_trace_max_gb > 0.0 ? cfg.nu_trace_max_gb : 16.0;
                const double need_gb = (double)rows_cap * (double)NJ * sizeof(real) / 1073741824.0;
                if (need_gb <= cap_gb) rc |= dTrNu.alloc((size_t)rows_cap * NJ * sizeof(real));
            }
        }
#ifdef ERM_TIMELINE_BUILD
        if (getenv("ERM_TIMELINE")) rc |= dDbgTs.alloc(2 * 16 * 16 * sizeof(unsigned long long));
#endif
        if (rc) return rc;
        if (cfg.profile) {
            pass_ev.resize(2 * 4096);
            for (auto& e : pass_ev) HIPCHK(hipEventCreate(&e));
        }

        // ---- default state (constructors' deterministic part: a = 1, b = 0, lambda = 0, sig2t = 1, Sigp = I)
        std::vector<double> par(par_size(J), 0.0);
        for (const auto& f : FIELDS) std::fill_n(&par[f.off(J)], J, f.init);
        par[par_off_sigp(J) + 0] = 1.0; par[par_off_sigp(J) + 3] = 1.0;
        par[par_off_derived(J)] = (double)J;
        for (int k = 0; k < 2; ++k) H2D(dParB[k].p, par.data(), par.size() * sizeof(double));
        if (dNu.p) {
            std::vector<real> ones(dNu.bytes / sizeof(real), real(1));
            H2D(dNu.p, ones.data(), dNu.bytes);
        }
        {   // the Polya-Gamma proposal table, computed here in fp64 (the oracle restates the same closed form)
            std::vector<double> tab((size_t)PG_NBIN * 4);
            for (int k = 0; k < PG_NBIN; ++k) pg_bin(k, &tab[(size_t)4 * k]);
            if (int rc2 = dPgTab.alloc(tab.size() * sizeof(double))) return rc2;
            H2D(dPgTab.p, tab.data(), tab.size() * sizeof(double));
        }
        persist_fault_countdown = (cfg.flags & ERM_FLAG_TEST_PERSIST_TIMEOUT) ? 2 : 0;
        timing.lanes_per_row = G.W; timing.block_threads = G.block_threads; timing.grid_blocks = G.grid_blocks;
        timing.lds_bytes = (int32_t)std::max(G.lds_pass[0], G.lds_pass[1]); timing.cu_count = cu_count;
        return configure_kernels();
    }

    // -------------------------------------------------------------------------------------------- kernels
    template <int MODEL, int PHASE, bool FUSED> int set_lds_attr(size_t bytes) {
        HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(&pass_kernel<MODEL, real, PHASE, FUSED>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
        return 0;
    }
    // dynamic LDS limits of every kernel this engine launches; the planner's figure for the kernels' STATIC LDS is checked against the compiler's
    template <int MODEL, int PHASE, bool FUSED> int check_static_lds() {
        hipFuncAttributes fa;
        HIPCHK(hipFuncGetAttributes(&fa, reinterpret_cast<const void*>(&pass_kernel<MODEL, real, PHASE, FUSED>)));
        if (fa.sharedSizeBytes > G.lds_static[PHASE])
            return fail(ERM_ERR_STATE, "internal: pass_kernel declares " + std::to_string(fa.sharedSizeBytes) + " B of static LDS, the planner assumes " + std::to_string(G.lds_static[PHASE]));
        return 0;
    }
    int configure_kernels() {
        const int tl = (int)G.lds_tiny;
        return dispatch([&](auto m) -> int {
            constexpr int M = decltype(m)::value;
            if (int rc = check_static_lds<M, 0, false>()) return rc;
            if (int rc = set_lds_attr<M, 0, false>(G.lds_pass[0])) return rc;
            HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(&tiny_kernel<M, 0>), hipFuncAttributeMaxDynamicSharedMemorySize, tl));
            if constexpr (!fam_cq(M)) {
                if (fused()) { if (int rc = check_static_lds<M, 0, true>()) return rc; if (int rc = set_lds_attr<M, 0, true>(G.lds_fused)) return rc; }
                if (persist) {
                    hipFuncAttributes fa;
                    HIPCHK(hipFuncGetAttributes(&fa, reinterpret_cast<const void*>(&pass_kernel<M, real, 0, true, true>)));
                    if (fa.sharedSizeBytes > G.lds_static[0]) return fail(ERM_ERR_STATE, "internal: the persistent kernel's static LDS exceeds the planner's figure");
                    HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(&pass_kernel<M, real, 0, true, true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)G.lds_fused));
                    // every workgroup of a persistent launch must be resident at once: ask the runtime how many fit a compute unit with this block size and LDS
                    int per_cu = 0;
                    HIPCHK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, reinterpret_cast<const void*>(&pass_kernel<M, real, 0, true, true>), G.block_threads, G.lds_fused));
                    if ((long long)per_cu * cu_count < G.grid_blocks) set_persist_avail(false);
                }
            }
            if constexpr (fam_cq(M)) {
                if (int rc = check_static_lds<M, 1, false>()) return rc;
                if (int rc = set_lds_attr<M, 1, false>(G.lds_pass[1])) return rc;
                HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(&tiny_kernel<M, 1>), hipFuncAttributeMaxDynamicSharedMemorySize, tl));
            }
            return 0;
        });
    }

    // stage-timing knobs: read only by a -DERM_DIAG_BUILD library (the kernels of the shipped one contain no early return at all)
    static int diag_stop(const char* name) {
#ifdef ERM_DIAG_BUILD
        const char* e = getenv(name);
        return e ? atoi(e) : 0;
#else
        (void)name;
        return 0;
#endif
    }
    // the quantile weights' constants (src/Draw.pl.jl:163-164) for the sweep, WAIC, the replicates and DIC alike; without weights nu == 1, k1 = 0, k2 = 1
    struct QuantileConsts { double k1, k2; };
    QuantileConsts quantile_consts() const {
        if (!m_nu()) return {0.0, 1.0};
        const double q = cfg.q_rt;
        return {(1.0 - 2.0 * q) / (q * (1.0 - q)),
                2.0 / (q * (1.0 - q))};
    }
    PassArgs<real> pass_args(int phase, int mode, bool fz = false) const {
        PassArgs<real> a{};
        a.Y = dY.as<uint8_t>(); a.C = dC.as<real>(); a.omega = dOmega.as<real>(); a.nu = dNu.as<real>(); a.X = dX.as<real>();
        a.theta = dTheta.as<real>(); a.zeta = dZeta.as<real>();
        a.par = dParB[cur].template as<double>(); a.cst = dCst.as<double>(); a.pgtab = dPgTab.as<double>();
        a.slab = phase == 0 ? dSlab0.as<double>() : dSlab1.as<double>();
        a.gslab = phase == 0 ? dGslab0B[fz ? 1 - cur : cur].template as<double>() : dGslab1.as<double>();
        a.gcnt = dGcnt.as<unsigned int>() + (phase == 0 ? 0 : G.n_groups);
        a.ctl = dCtlB[cur].template as<Ctl>();
        a.sum_theta = dSumTheta.as<double>(); a.sum_zeta = dSumZeta.as<double>(); a.sum_nu = dSumNu.as<double>();
        a.tr_theta = dTrTheta.as<real>(); a.tr_zeta = dTrZeta.as<real>(); a.tr_nu = dTrNu.as<real>();
        a.N = N; a.rows_per_block = G.rows_per_block; a.rows_per_wave = G.rows_per_wave; a.J = J; a.nFeat = Fk; a.W = G.W; a.logW = G.logW; a.IPL = G.IPL; a.mode = mode; a.ngx = phase == 0 ? ngx() : 0;
        a.chain = (uint32_t)cfg.chain_id; a.seed = cfg.seed;
        const QuantileConsts k = quantile_consts();
        a.k1 = k.k1; a.k2 = k.k2;
        a.dbg_stop = diag_stop("ERM_PASS_STOP"); a.dbg_sweep = (uint32_t)diag_stop("ERM_STOP_SWEEP");
        a.dbg_ts = dDbgTs.as<unsigned long long>();
        a.row_base = (uint32_t)row_base;
        a.acc_off = fz ? G.acc_off_fused : G.acc_off[phase];     // the accumulators close the launch's dynamic LDS
        for (int k = 0; k < 2; ++k) { a.parB[k] = dParB[k].template as<double>(); a.ctlB[k] = dCtlB[k].template as<Ctl>(); a.gslabB[k] = dGslab0B[k].template as<double>(); }
        a.nsweeps = 1u; a.cur0 = (uint32_t)cur;
        a.xbuf = dXbuf.as<unsigned long long>(); a.tag0 = 0u; a.tmo = dGcnt.as<unsigned int>() + 2 * G.n_groups;
        return a;
    }
    TinyArgs tiny_args(int mode, bool fz = false) const {
        TinyArgs t{};
        const int o = fz ? 1 - cur : cur;
        t.par = dParB[cur].template as<double>(); t.par_out = dParB[o].template as<double>();
        t.cst = dCst.as<double>(); t.slab0 = dGslab0B[cur].template as<double>(); t.slab1 = dGslab1.as<double>();
        t.ctl = dCtlB[cur].template as<Ctl>(); t.ctl_out = dCtlB[o].template as<Ctl>(); t.ctl_err = dCtlB[0].template as<Ctl>();
        t.tr_item = dTrItem.as<double>(); t.tr_ll = dTrLl.as<double>();
        t.N = N; t.J = J; t.nFeat = Fk; t.nb0 = G.n_groups; t.nb1 = G.n_groups; t.mode = mode;
        t.intercept = cfg.intercept; t.onepl = cfg.one_pl; t.cov2one = cfg.cov2one; t.sigp_mode = cfg.sigp_mode;
        t.chain = (uint32_t)cfg.chain_id; t.seed = cfg.seed;
        const QuantileConsts k = quantile_consts();
        t.k1 = k.k1; t.k2 = k.k2;
        t.nq = nq(); t.ngx = ngx();
        if (sharded()) {     // the statistics rows of all devices, gathered after every row pass; N = the whole data set
            t.slab0 = dShardRecv[0].as<double>(); t.slab1 = dShardRecv[1].as<double>(); t.nb0 = shard_count; t.nb1 = shard_count; t.N = n_total;
        }
        t.dbg_stop = diag_stop("ERM_TINY_STOP"); t.dbg_sweep = (uint32_t)diag_stop("ERM_STOP_SWEEP");
        return t;
    }

    int64_t n_pass_timed = 0;                        // sweep-kernel launches inside event brackets in the current run
    int64_t n_brackets = 0;                          // event pairs used
    std::vector<int> bracket_launches;               // launches inside each bracket
    bool bracket_open = false;
    // The event pair around timed launches: bracket(false) opens one (profile mode, while pairs beyond the calibration's are left), bracket(true, n) closes
    // the open one, which held n launches of the sweep kernel (n sweeps of a graph or a persistent launch).
    int bracket(bool close, int64_t launches = 0) {
        if (close ? !bracket_open : (bracket_open || !cfg.profile || (size_t)(2 * n_brackets + 1) + 64 >= pass_ev.size())) return 0;
        HIPCHK(hipEventRecord(pass_ev[2 * n_brackets + (close ? 1 : 0)], stream));
        bracket_open = !close;
        if (close) { ++n_brackets; n_pass_timed += launches; bracket_launches.push_back((int)launches); }
        return 0;
    }
    // (pw: this launch completes a sweep -- the pointwise pass of an engine with WAIC enabled follows it, inside the launch's event bracket)
    template <int MODEL, int PHASE> int launch_pass(int mode, bool timed, bool pw = false) {
        PassArgs<real> a = pass_args(PHASE, mode);
        TinyArgs t{};
        if (timed) { if (int rc = bracket(false)) return rc; }
        hipLaunchKernelGGL((pass_kernel<MODEL, real, PHASE, false>), dim3(G.grid_blocks), dim3(G.block_threads), G.lds_pass[PHASE], stream, a, t);
        if (pw) { if (int rc = launch_behind<MODEL>(cur)) return rc; }
        if (timed) { if (int rc = bracket(true, 1)) return rc; }
        if (sharded()) return shard_exchange(PHASE, a.gslab);
        return 0;
    }
    // Subject-sharded chains: this device's statistics of the pass just enqueued -> one row -> all-gather over the devices
    int shard_exchange(int phase, const double* gslab) {
        hipLaunchKernelGGL(shard_pack_kernel, dim3(1), dim3(256), 0, stream, gslab, G.n_groups, G.ns[phase], dShardSend.as<double>());
        HIPCHK(hipGetLastError());
        return gather_row(phase, (size_t)G.ns[phase]);
    }
    // all-gather of n doubles of dShardSend into dShardRecv[k]: in stream order over RCCL, or through the caller's callback
    int gather_row(int k, size_t n) {
        if (comm) { RCCLCHK(g_rccl.AllGather(dShardSend.p, dShardRecv[k].p, n, ncclDouble, comm, stream)); return 0; }
        HIPCHK(hipStreamSynchronize(stream));
        if (exch(exch_user, dShardSend.p, dShardRecv[k].p, n * sizeof(double)) != 0) return fail(ERM_ERR_STATE, "the shard exchange callback failed");
        return 0;
    }
    // element-wise sum over the devices of a small host vector, in rank order on every device (data constants in erm_set_data)
    int shard_allsum(std::vector<double>& v) {
        if (!sharded()) return 0;
        const size_t nb = v.size() * sizeof(double);
        if (nb > dShardSend.bytes) return fail(ERM_ERR_STATE, "shard scratch too small");
        HIPCHK(hipMemcpyAsync(dShardSend.p, v.data(), nb, hipMemcpyHostToDevice, stream));
        if (int rc = gather_row(0, v.size())) return rc;
        HIPCHK(hipStreamSynchronize(stream));
        std::vector<double> all(v.size() * (size_t)shard_count);
        HIPCHK(hipMemcpy(all.data(), dShardRecv[0].p, nb * (size_t)shard_count, hipMemcpyDeviceToHost));
        for (size_t e = 0; e < v.size(); ++e) { double t = 0.0; for (int r = 0; r < shard_count; ++r) t += all[(size_t)r * v.size() + e]; v[e] = t; }
        return 0;
    }
    int set_shard(int rank, int count, int64_t ntot, int64_t base, erm_exchange_fn fn, void* user, const void* rccl_id) override {
        if (has_data || rows_done > 0 || sharded()) return fail(ERM_ERR_STATE, "erm_set_shard must precede erm_set_data and be called once");
        if (pw_unit != PW_OFF) return fail(ERM_ERR_STATE, "an engine with WAIC enabled cannot become a shard (sharding: erm_set_pointwise)");
        if (pred_thin > 0) return fail(ERM_ERR_STATE, "an engine with posterior predictive checks enabled cannot become a shard (sharding: erm_set_predictive)");
        if (count < 1 || rank < 0 || rank >= count) return fail(ERM_ERR_ARG, "bad shard rank / count");
        if (!fn && !rccl_id) return fail(ERM_ERR_ARG, "exchange callback / RCCL id is NULL");
        if (base < 0 || ntot < N || base + N > ntot) return fail(ERM_ERR_ARG, "local subjects must lie inside [0, n_subj_total)");
        if (ntot >= (1LL << 32)) return fail(ERM_ERR_ARG, "n_subj_total must fit 32 bits");
        HIPCHK(hipSetDevice(cfg.device));
        const size_t width = (size_t)std::max(std::max(G.ns[0], G.ns[1]), 3 * J + PMAX * PMAX + 8);
        if (int rc = dShardSend.alloc(width * sizeof(double))) return rc;
        for (int k = 0; k < (m_cq() ? 2 : 1); ++k) { if (int rc = dShardRecv[k].alloc(width * (size_t)std::max(count, GROUP) * sizeof(double))) return rc; }   // >= GROUP rows: see dGslab0B
        if (rccl_id) {
            if (int rc = g_rccl.load()) return rc;
            ncclUniqueId id;
            std::memcpy(&id, rccl_id, sizeof(id));
            RCCLCHK(g_rccl.CommInitRank(&comm, count, id, rank));
        }
        shard_rank = rank; shard_count = count; n_total = ntot; row_base = base; exch = fn; exch_user = user;
        set_persist_avail(false);          // a sharded sweep exchanges its statistics rows on the host side of every launch
        return 0;
    }
    // one whole sweep of a single-pass model: tiny step + row pass in one launch; reads buffers [cur], writes [1 - cur]
    template <int MODEL> int launch_fused(bool timed) {
        PassArgs<real> a = pass_args(0, 1, true);
        TinyArgs t = tiny_args(0, true);
        if (timed) { if (int rc = bracket(false)) return rc; }
        hipLaunchKernelGGL((pass_kernel<MODEL, real, 0, true>), dim3(G.grid_blocks), dim3(G.block_threads), G.lds_fused, stream, a, t);
        if (int rc = launch_behind<MODEL>(1 - cur)) return rc;      // the sweep published its parameter block and counters in buffer [1 - cur]
        if (timed) { if (int rc = bracket(true, 1)) return rc; }
        if (sharded()) return shard_exchange(0, a.gslab);     // a.gslab: the group rows this launch wrote
        return 0;
    }
    // nsweeps whole sweeps in ONE launch (small data sets): reads buffers [cur] first, alternates inside the launch
    template <int MODEL> int launch_persist(int64_t nsweeps, bool timed) {
        PassArgs<real> a = pass_args(0, 1, true);
        TinyArgs t = tiny_args(0, true);
        a.nsweeps = (uint32_t)nsweeps; a.cur0 = (uint32_t)cur;
        if (xtag > 0x7fffffffu - (uint32_t)nsweeps) { HIPCHK(hipMemsetAsync(dXbuf.p, 0, dXbuf.bytes, stream)); xtag = 0; }
        a.tag0 = xtag; xtag += (uint32_t)nsweeps;
        if (timed) { if (int rc = bracket(false)) return rc; }
        hipLaunchKernelGGL((pass_kernel<MODEL, real, 0, true, true>), dim3(G.grid_blocks), dim3(G.block_threads), G.lds_fused, stream, a, t);
        return bracket(true, nsweeps);
    }
    template <int MODEL, int STEP> int launch_tiny(int mode) {
        TinyArgs t = tiny_args(mode);
        hipLaunchKernelGGL((tiny_kernel<MODEL, STEP>), dim3(1), dim3(TINY_THREADS), G.lds_tiny, stream, t);
        return 0;
    }

    // One sweep = tiny step + row pass (CrossQr: two of each).  Kernel arguments never change between sweeps -- the sweep / trace-row counters and the
    // "first sweep of this call" flag live in device memory (Ctl) -- so EVERY sweep of a run is the same launch sequence and can be captured once into a
    // hipGraph and replayed.  Which graphs, single sweeps and event brackets a call consists of is decided by plan_run (erm_schedule.hpp) and nowhere else.
    static constexpr int GRAPH_SWEEPS = 32;
    // block[gi]: block_sweeps(gi) sweeps; full[k], tail[r]: see StepKind.  Each is built by the first call whose plan replays it.
    hipGraphExec_t graphs[NBLOCK] = {}, graphs_full[GRAPH_SWEEPS + 1] = {}, graphs_tail[GRAPH_SWEEPS + 1] = {};
    hipGraphExec_t* graph_of(const Step& s) { return s.kind == STEP_BLOCK ? &graphs[s.gi] : s.kind == STEP_FULL ? &graphs_full[s.n] : &graphs_tail[s.n]; }
    void drop_graphs() {
        for (auto& g : graphs) { if (g) (void)hipGraphExecDestroy(g); g = nullptr; }
        for (auto* arr : {graphs_full, graphs_tail}) for (int k = 0; k <= GRAPH_SWEEPS; ++k) { if (arr[k]) (void)hipGraphExecDestroy(arr[k]); arr[k] = nullptr; }
    }
    bool ev_calibrated = false; double ev_null_ms = 0.0;
    template <int MODEL> int enqueue_sweep(bool timed) {
        if constexpr (!fam_cq(MODEL)) { if (fused()) return launch_fused<MODEL>(timed); }
        if (int rc = launch_tiny<MODEL, 0>(0)) return rc;
        if (int rc = launch_pass<MODEL, 0>(1, timed, !fam_cq(MODEL))) return rc;
        if constexpr (fam_cq(MODEL)) {
            if (int rc = launch_tiny<MODEL, 1>(0)) return rc;
            // WAIC / predictive checks on GibbsRtIrtCrossQr: pass B overwrites nu_t with nu_{t+1} in the phase that uses it, so nu_t is copied first (a memcpy node inside a graph)
            if (model_traits(MODEL).nu == NU_CELL && aux_pass()) HIPCHK(hipMemcpyAsync(dNuSnap.p, dNu.p, dNu.bytes, hipMemcpyDeviceToDevice, stream));
            if (int rc = launch_pass<MODEL, 1>(1, timed, true)) return rc;
        }
        return 0;
    }
    // ---- WAIC: the pointwise pass behind a sweep (erm_waic_kernels.hpp).  buf: the half of the double buffers the sweep published its parameter block and
    // counters in.  The same launch for every sweep (the kernel itself skips burn-in rows), so it sits inside the captured graphs like the sweep's own kernels.
    int64_t pw_units(int unit) const { return unit == PW_SUBJECT ? N : unit == PW_CELL ? N * (int64_t)J : 0; }
    // the geometry of every pass behind a sweep and of DIC's loglik_kernel: pass_geom (erm_geometry.hpp) and nothing else
    PassGeom pgeom() const { return pass_geom(cfg.model, N, J, cu_count); }
    // A pass whose launch was refused must not leave zeros behind a run that reports success: outside stream capture the launch status is read, inside a
    // capture (where a refused node invalidates the capture) the capture's own status.  (hipGetLastError also returns an earlier error of this thread that nobody
    // read: the message names the launch it was found behind, not necessarily its cause.)
    int behind_status(const char* what) {
        hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
        HIPCHK(hipStreamIsCapturing(stream, &cs));
        if (cs == hipStreamCaptureStatusNone) {
            const hipError_t e = hipGetLastError();
            if (e != hipSuccess) return fail(ERM_ERR_HIP, std::string("HIP error pending behind the launch of ") + what + ": " + hipGetErrorString(e));
        } else if (cs != hipStreamCaptureStatusActive) {
            return fail(ERM_ERR_HIP, std::string("launch of ") + what + " invalidated the stream capture");
        }
        return 0;
    }
    // the resident cell as every pass behind a sweep reads it (CellArgs, erm_waic_kernels.hpp)
    CellArgs cell_args(int buf) const {
        CellArgs c{};
        c.Y = dY.as<uint8_t>(); c.C = dC.p; c.nu = mt().nu == NU_CELL ? dNuSnap.p : nullptr; c.theta = dTheta.p; c.zeta = dZeta.p;
        c.par = dParB[buf].template as<double>(); c.cm = dCst.as<double>() + cst_off_m(J); c.ctl = dCtlB[buf].template as<Ctl>();
        c.N = N; c.J = J; c.logW = pgeom().logW;
        const QuantileConsts k = quantile_consts();
        c.k1 = k.k1; c.k2 = k.k2;
        return c;
    }
    template <int MODEL> int launch_pointwise(int buf) {
        if (pw_unit == PW_OFF) return 0;
        PwArgs a{};
        a.cell = cell_args(buf);
        a.acc_ms = dPwMs.as<double2>(); a.acc_w = dPwW.as<double2>();
        const PassGeom g = pgeom();
        if (pw_unit == PW_SUBJECT) hipLaunchKernelGGL((pointwise_kernel<MODEL, real, PW_SUBJECT>), dim3(g.nb_pw_subject), dim3(PASS_THREADS), g.lds_pw, stream, a);
        else hipLaunchKernelGGL((pointwise_kernel<MODEL, real, PW_CELL>), dim3(g.nb_pw_cell), dim3(PASS_THREADS), g.lds_pw, stream, a);
        return behind_status("the WAIC pass");
    }
    // The one way a pass behind the sweep is switched (erm_set_pointwise, erm_set_predictive).  sw: the pass's switch (pw_unit / pred_thin, 0 = off), want: its new
    // value; bufs: the buffers the pass owns and the sizes it wants of them now (0 = released).  The refusals, in this order; the device drained; `configure` (the
    // pass's own preparation, may fail); the buffers whose size changes staged and only then moved into place, so that a failed allocation leaves the engine
    // exactly as it was; the captured graphs dropped if the switch moved; the schedule decided again.  The caller clears its accumulators afterwards.
    struct PassBuf { DevBuf* buf; size_t bytes; const char* what; };
    int switch_pass(const char* api, const char* subject, int& sw, int want, std::vector<PassBuf> bufs, const char* snap_what, const std::function<int()>& configure = nullptr) {
        if (rows_done > 0) return fail(ERM_ERR_STATE, std::string(api) + " is allowed only while no trace row is recorded (after erm_create or erm_reset_trace)");
        if (want && sharded()) return fail(ERM_ERR_STATE, std::string(subject) + " not available under subject sharding (the accumulators of the shards would have to be merged across devices)");
        HIPCHK(hipSetDevice(cfg.device));
        HIPCHK(hipStreamSynchronize(stream));
        if (configure) { if (int rc = configure()) return rc; }
        const int prev = sw;
        sw = want;      // what follows is a function of the resulting state (put back if an allocation fails)
        // GibbsRtIrtCrossQr's copy of nu_t: kept iff any pass is on
        bufs.push_back({&dNuSnap, mt().nu == NU_CELL && aux_pass() ? dNu.bytes : 0, snap_what});
        std::vector<DevBuf> staged(bufs.size());
        for (size_t k = 0; k < bufs.size(); ++k) {
            if (bufs[k].bytes == bufs[k].buf->bytes) continue;
            if (int rc = staged[k].try_alloc(bufs[k].bytes, bufs[k].what)) { sw = prev; return rc; }
        }
        for (size_t k = 0; k < bufs.size(); ++k) { if (bufs[k].bytes != bufs[k].buf->bytes) *bufs[k].buf = std::move(staged[k]); }
        if (want != prev) drop_graphs();      // the captured sweeps hold (or lack) the pass's launches, and its switch as a kernel argument
        set_persist_avail(persist_avail);
        return 0;
    }
    int pw_clear() {
        if (dPwMs.p) { HIPCHK(hipMemsetAsync(dPwMs.p, 0, dPwMs.bytes, stream)); HIPCHK(hipMemsetAsync(dPwW.p, 0, dPwW.bytes, stream)); }
        return 0;
    }
    int set_pointwise(int unit) override {
        if (unit != PW_OFF && unit != PW_SUBJECT && unit != PW_CELL) return fail(ERM_ERR_ARG, "unknown pointwise unit (ERM_POINTWISE_OFF / _SUBJECT / _CELL)");
        const size_t nb = (size_t)pw_units(unit) * sizeof(double2);
        const char* what = "the WAIC accumulators";
        if (int rc = switch_pass("erm_set_pointwise", "WAIC is", pw_unit, unit, {{&dPwMs, nb, what}, {&dPwW, nb, what}}, what)) return rc;
        return pw_clear();
    }
    int64_t pointwise_units() const override { return pw_units(pw_unit); }
    int pw_ready() {
        if (pw_unit == PW_OFF) return fail(ERM_ERR_STATE, "WAIC is not enabled on this engine (erm_set_pointwise)");
        if (poisoned) return fail(ERM_ERR_STATE, "a previous erm_run failed part-way: the state is undefined until erm_set_state");
        if (post_rows < 2) return fail(ERM_ERR_STATE, "WAIC needs at least two post-burn-in rows");
        HIPCHK(hipSetDevice(cfg.device));
        return 0;
    }
    int pw_finish(double center, double* lppd_out, double* p_out, double* sums) {
        return pw_finish_on(dPwMs.as<double2>(), dPwW.as<double2>(), pointwise_units(), post_rows, center, lppd_out, p_out, stream, sums);
    }
    int get_waic(double* out8) override {
        if (int rc = pw_ready()) return rc;
        return pw_totals(dPwMs.as<double2>(), dPwW.as<double2>(), pointwise_units(), post_rows, stream, out8);
    }
    // ---- the passes over the item trace, computed after the run from the resident data set and item-trace rows (defined where ItemSource is: below erm_item_pass.hpp)
    const double* item_trace_dev() const override { return dTrItem.as<double>(); }
    int item_source(int pass, ItemSource& S) override;
    int get_pointwise(double* lppd_u, double* p_u) override {
        if (int rc = pw_ready()) return rc;
        const int64_t U = pointwise_units();
        DevBuf dL, dP;
        if (lppd_u) { if (int rc = dL.alloc((size_t)U * sizeof(double))) return rc; }
        if (p_u) { if (int rc = dP.alloc((size_t)U * sizeof(double))) return rc; }
        double sums[PW_FIN_COLS];
        if (int rc = pw_finish(0.0, dL.as<double>(), dP.as<double>(), sums)) return rc;
        auto down = [&](const DevBuf& d, double* dst) -> int {
            if (!dst) return 0;
            if (pw_unit == PW_SUBJECT) { HIPCHK(hipMemcpy(dst, d.p, (size_t)U * sizeof(double), hipMemcpyDeviceToHost)); return 0; }
            std::vector<double> t((size_t)U);      // cells: device order (row-major) -> the caller's column-major [nSubj][nItem]
            HIPCHK(hipMemcpy(t.data(), d.p, t.size() * sizeof(double), hipMemcpyDeviceToHost));
            rows_to_cols(t.data(), dst, N, J);
            return 0;
        };
        if (int rc = down(dL, lppd_u)) return rc;
        return down(dP, p_u);
    }
    // ---- posterior predictive checks: the replicate pass behind a sweep and the item / total step behind it (erm_predictive_kernels.hpp).  Like the WAIC pass
    // the same two launches for every sweep (the kernels skip rows that are no replicate rows), inside the captured graphs; with both enabled, both run.
    // The geometry is a function of (N, J) alone: the accumulators do not depend on the device, the sweep kernels' geometry or the schedule.
    template <int MODEL> int launch_behind(int buf) {
        if (int rc = launch_pointwise<MODEL>(buf)) return rc;
        return launch_predictive<MODEL>(buf);
    }
    template <int MODEL> int launch_predictive(int buf) {
        if (pred_thin == 0) return 0;
        const PassGeom g = pgeom();
        PredArgs a{};
        a.cell = cell_args(buf);
        a.subj = dPredSubj.as<double>(); a.slab = dPredSlab.as<double>(); a.thin = (uint32_t)pred_thin;
        a.seed = cfg.seed; a.chain = (uint32_t)cfg.chain_id; a.row_base = (uint32_t)row_base;
        hipLaunchKernelGGL((predictive_kernel<MODEL, real>), dim3(g.nb_pred), dim3(g.T), g.lds_pred, stream, a);
        if (int rc = behind_status("the replicate pass")) return rc;
        PredItemArgs b{};
        b.slab = dPredSlab.as<double>(); b.nb = g.nb_pred; b.nq = g.nq; b.J = J; b.N = (double)N; b.k0 = dCst.as<double>() + cst_off_k0(J);
        b.ctl = a.cell.ctl; b.thin = a.thin; b.item = dPredItem.as<double>(); b.tot = dPredItem.as<double>() + (size_t)J * PRED_ITEM;
        hipLaunchKernelGGL(predictive_items_kernel, dim3(1), dim3(PRED_IT_THREADS), 0, stream, b);
        return behind_status("the replicate pass's item step");
    }
    int pred_clear() {
        if (dPredSubj.p) { HIPCHK(hipMemsetAsync(dPredSubj.p, 0, dPredSubj.bytes, stream)); HIPCHK(hipMemsetAsync(dPredItem.p, 0, dPredItem.bytes, stream)); }
        return 0;
    }
    int set_predictive(int on, int32_t thin) override {
        if (on && thin < 1) return fail(ERM_ERR_ARG, "erm_set_predictive: thin must be at least 1");
        const PassGeom g = pgeom();
        const size_t dbl = on ? sizeof(double) : 0;      // off: every buffer released
        const char* acc = "the predictive accumulators";
        auto lds_limit = [&]() -> int {
            if (!on) return 0;
            return dispatch([&](auto m) -> int {
                HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(&predictive_kernel<decltype(m)::value, real>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)g.lds_pred));
                return 0; });
        };
        if (int rc = switch_pass("erm_set_predictive", "posterior predictive checks are", pred_thin, on ? thin : 0,
                                 {{&dPredSubj, (size_t)N * PRED_SUBJ * dbl, acc}, {&dPredItem, ((size_t)J * PRED_ITEM + PRED_TOT + 1) * dbl, acc},
                                  {&dPredSlab, (size_t)g.nb_pred * g.nq * J * dbl, "the predictive slab"}}, "the copy of nu", lds_limit)) return rc;
        return pred_clear();
    }
    int64_t predictive_reps() const override { return pred_thin > 0 ? (post_rows + pred_thin - 1) / pred_thin : 0; }
    int get_predictive(double* item, double* subj, double* total) override {
        if (pred_thin == 0) return fail(ERM_ERR_STATE, "posterior predictive checks are not enabled on this engine (erm_set_predictive)");
        if (poisoned) return fail(ERM_ERR_STATE, "a previous erm_run failed part-way: the state is undefined until erm_set_state");
        const int64_t R = predictive_reps();
        if (R < 1) return fail(ERM_ERR_STATE, "posterior predictive checks need at least one replicate row");
        HIPCHK(hipSetDevice(cfg.device));
        HIPCHK(hipStreamSynchronize(stream));
        const double nan = std::nan("");
        std::vector<double> it((size_t)J * PRED_ITEM + PRED_TOT + 1);
        HIPCHK(hipMemcpy(it.data(), dPredItem.p, it.size() * sizeof(double), hipMemcpyDeviceToHost));
        unsigned long long dev_reps = 0;
        std::memcpy(&dev_reps, &it[(size_t)J * PRED_ITEM + PRED_TOT], sizeof(dev_reps));
        if ((int64_t)dev_reps != R) return fail(ERM_ERR_STATE, "internal: the device counted " + std::to_string(dev_reps) + " replicate rows, the host " + std::to_string(R));
        if (item) for (int c = 0; c < 3; ++c) for (int q = 0; q < 4; ++q) for (int j = 0; j < J; ++j)
            item[((size_t)c * 4 + q) * J + j] = (c == 1 && !is_rt()) ? nan : it[(size_t)j * PRED_ITEM + c * 4 + q];
        if (total) for (int c = 0; c < 2; ++c) for (int q = 0; q < 4; ++q) total[c * 4 + q] = (c == 1 && !is_rt()) ? nan : it[(size_t)J * PRED_ITEM + c * 4 + q];
        if (subj) {
            std::vector<double> su((size_t)N * PRED_SUBJ);
            HIPCHK(hipMemcpy(su.data(), dPredSubj.p, su.size() * sizeof(double), hipMemcpyDeviceToHost));
            for (int c = 0; c < 2; ++c) for (int q = 0; q < 4; ++q) for (int64_t i = 0; i < N; ++i)
                subj[((size_t)c * 4 + q) * N + i] = (c == 1 && !is_rt()) ? nan : su[(size_t)i * PRED_SUBJ + c * 4 + q];
        }
        return 0;
    }
    void launch_run_begin() {
        hipLaunchKernelGGL(run_begin_kernel, dim3(1), dim3(256), 0, stream, dCtlB[0].template as<Ctl>(), dCtlB[1].template as<Ctl>(), host_run_dev, dGcnt.as<unsigned int>(), 2 * G.n_groups + 4);
    }
    void launch_run_end() {
        hipLaunchKernelGGL(run_end_kernel, dim3(1), dim3(64), 0, stream, dCtlB[0].template as<Ctl>(), dCtlB[1].template as<Ctl>(), dGcnt.as<unsigned int>() + 2 * G.n_groups,
                           host_ctl_dev + 1, reinterpret_cast<unsigned int*>(host_ctl_dev + 3));
    }
    Plan plan;                                       // the call being enqueued
    // run_steps' executor: one launch per step kind, the graphs, the event brackets, the buffer parity
    template <int MODEL> struct Exec {
        Engine& e;
        bool built(const Step& s) const { return *e.graph_of(s) != nullptr; }
        int build(const Step& s) { return e.template build_graph<MODEL>(s); }
        int bracket(bool close, int64_t sweeps) { return e.bracket(close, sweeps); }
        void flip(int64_t sweeps) { e.cur = (int)((e.cur + sweeps) & 1); }
        int launch(const Step& s, bool timed) {
            switch (s.kind) {
            case STEP_RUN_BEGIN: e.launch_run_begin(); return 0;
            case STEP_RUN_END: e.launch_run_end(); return 0;
            case STEP_PROLOGUE:
                if (int rc = e.template launch_pass<MODEL, 0>(0, false)) return rc;
                if constexpr (fam_cq(MODEL)) return e.template launch_pass<MODEL, 1>(0, false);
                return 0;
            case STEP_PERSIST:
                if constexpr (!fam_cq(MODEL)) return e.template launch_persist<MODEL>(s.n, timed);
                return fail(ERM_ERR_STATE, "internal: a persistent step in a Cross-family plan");
            case STEP_SINGLE: return e.template enqueue_sweep<MODEL>(timed);
            case STEP_TINY_CLOSE: return e.template launch_tiny<MODEL, 0>(1);
            default: HIPCHK(hipGraphLaunch(*e.graph_of(s), e.stream)); return 0;
            }
        }
    };
    int run_model(const Plan& P, int from, int to) {
        return dispatch([&](auto m) -> int { Exec<decltype(m)::value> x{*this}; return run_steps(P, from, to, x); });
    }
    // Captures what graph step `s` stands for (graph_body).  The capture starts at buffer parity 0 -- a graph is only ever replayed there -- and leaves the
    // parity alone, also when it fails: the replay moves it.
    template <int MODEL> int build_graph(const Step& s) {
        hipGraphExec_t* out = graph_of(s);
        hipGraph_t g = nullptr;
        const int cur0 = cur;
        const Plan body = graph_body(plan, s);
        HIPCHK(hipStreamBeginCapture(stream, hipStreamCaptureModeThreadLocal));
        Exec<MODEL> x{*this};
        int rc = run_steps(body, 0, body.n, x);
        const hipError_t e = hipStreamEndCapture(stream, &g);      // always ends the capture, also after a failed enqueue
        if (!rc && e != hipSuccess) rc = fail(ERM_ERR_HIP, std::string("hipStreamEndCapture: ") + hipGetErrorString(e));
        if (!rc) {
            const hipError_t ei = hipGraphInstantiate(out, g, nullptr, nullptr, 0);
            if (ei != hipSuccess) { *out = nullptr; rc = fail(ERM_ERR_HIP, std::string("hipGraphInstantiate: ") + hipGetErrorString(ei)); }
        }
        if (g) (void)hipGraphDestroy(g);             // on every exit
        cur = cur0;
        return rc;
    }

    // ---- the state an erm_run changes in place (persistent launches save it first: a launch that times out is replayed per sweep from the copy).
    // Counters and tickets are re-initialised by every run, trace rows >= rows_done are simply written again, and the host's own counters move only
    // after a run has succeeded; what is left: theta, zeta, omega, LatentQr's nu, the parameter block and statistics of buffer 0 (every run starts
    // there), and the post-burn-in sums.
    template <typename Fn> void snap_each(Fn&& f) const {
        f(dTheta); if (is_rt()) f(dZeta);
        f(dOmega); if (mt().nu == NU_SUBJECT) f(dNu);
        f(dParB[0]); f(dGslab0B[0]);
        f(dSumTheta); if (is_rt()) f(dSumZeta); if (dSumNu.p) f(dSumNu);
    }
    size_t snap_bytes() const {
        // (called before the buffers exist: sizes from the configuration and the planned geometry)
        const size_t NJ = (size_t)N * J, r = sizeof(real);
        const size_t nnu = mt().nu == NU_SUBJECT ? (size_t)N : 0;      // (a persistent launch never serves CrossQr: two passes per sweep)
        size_t b = (size_t)N * r + (is_rt() ? (size_t)N * r : 0) + NJ * r + nnu * r;
        b += (size_t)par_size(J) * 8 + (size_t)std::max(G.n_groups, GROUP) * G.ns[0] * 8;
        b += (size_t)N * 8 + (is_rt() ? (size_t)N * 8 : 0) + nnu * 8;
        return b + 10 * 256;                         // every segment starts on a 256-byte boundary
    }
    int snap_copy(bool restore) {
        CopySegs S{};
        size_t off = 0;
        bool ok = true;
        snap_each([&](const DevBuf& d) {
            if (S.n >= 10 || off + d.bytes > dSnap.bytes) { ok = false; return; }
            char* sp = dSnap.as<char>() + off;
            S.src[S.n] = restore ? (const void*)sp : (const void*)d.p; S.dst[S.n] = restore ? d.p : (void*)sp; S.bytes[S.n] = d.bytes; ++S.n;
            off = (off + d.bytes + 255) & ~(size_t)255;
        });
        if (!ok) return fail(ERM_ERR_STATE, "internal: the persistent launch's snapshot buffer is too small");
        hipLaunchKernelGGL(copy_segments_kernel, dim3(256), dim3(256), 0, stream, S);
        HIPCHK(hipGetLastError());
        return 0;
    }

    // A run that fails after it has started enqueueing leaves the double buffers, the counters and the traces in an unknown state: the
    // stream is drained, the buffer parity reset, and the engine refuses to continue until the caller installs a state again.
    bool poisoned = false;
    bool stats_valid = false;                        // omega_{t+1} (nu_{t+1}) and the statistics of the CURRENT state are resident (set by a completed run)
    Ctl* host_ctl = nullptr;                         // pinned: [1], [2] the two device copies of the counters, [3] the time-out word (run_end_kernel stores them)
    Ctl* host_ctl_dev = nullptr;                     // the same memory as the device addresses it
    RunParams* host_run = nullptr;                   // pinned: the parameters of the erm_run being enqueued (run_begin_kernel reads them)
    RunParams* host_run_dev = nullptr;
    bool has_stats_state() const { return host_ctl != nullptr; }
    int run(int64_t nsweeps) override {
        if (!has_data) return fail(ERM_ERR_STATE, "erm_set_data has not been called");
        if (poisoned) return fail(ERM_ERR_STATE, "a previous erm_run failed part-way: call erm_set_state (and erm_reset_trace) before running again");
        if (nsweeps < 0) return fail(ERM_ERR_ARG, "nsweeps must be non-negative");
        if (rows_done + nsweeps > rows_cap) return fail(ERM_ERR_ARG, "trace capacity exceeded: n_iter*n_chain rows were allocated");
        int rc = run_checked(nsweeps);
        if (rc == ERM_PERSIST_TIMEOUT) {
            // the persistent launch never had all its workgroups resident (another process holds compute units): every workgroup has left the launch;
            // put back what the call found, leave the persistent schedule for good and run the call again, one launch per sweep at the same geometry
            // (bit for bit the chain the persistent launch would have produced)
            set_persist_avail(false); ++timing.persist_fallbacks;
            rc = snap_copy(true);
            if (rc == 0) { cur = 0; stats_valid = snap_stats_valid; rc = run_checked(nsweeps); }
            if (rc == ERM_PERSIST_TIMEOUT) rc = fail(ERM_ERR_STATE, "internal: persistent time-out reported by a per-sweep run");
        }
        if (rc != 0 && rc != ERM_ERR_NONFINITE) {
            const std::string msg = g_err;            // keep the first error's message
            (void)hipStreamSynchronize(stream);
            (void)hipGetLastError();
            cur = 0;
            poisoned = true;
            stats_valid = false;
            g_err = msg;
        }
        return rc;
    }
    static constexpr int ERM_PERSIST_TIMEOUT = -1000;      // internal: run_checked -> run
    int run_checked(int64_t nsweeps) {
        HIPCHK(hipSetDevice(cfg.device));
        if (sharded() || !has_stats_state()) stats_valid = false;
        Ctl c{};
        c.sweep = sweeps_total; c.row = (uint32_t)rows_done; c.burn_rows = (uint32_t)((int64_t)cfg.n_burnin * cfg.n_chain); c.err = 0;
        c.first = 1u;                                // no sweep of this call has been drawn yet: the first one writes trace row rows_done itself
        if (cur == 1) {      // every run starts from buffer 0 so that a captured graph always replays with the buffer parity it was built with
            HIPCHK(hipMemcpyAsync(dParB[0].p, dParB[1].p, dParB[0].bytes, hipMemcpyDeviceToDevice, stream));
            if (stats_valid) HIPCHK(hipMemcpyAsync(dGslab0B[0].p, dGslab0B[1].p, dGslab0B[0].bytes, hipMemcpyDeviceToDevice, stream));
            cur = 0;
        }
        const bool calibrate = cfg.profile && pass_ev.size() >= 64 && !ev_calibrated;
        {
            RunIn in;
            in.nsweeps = nsweeps; in.cq = m_cq(); in.fused = fused(); in.persist = persist; in.shard = exch ? SHARD_CALLBACK : comm ? SHARD_RCCL : SHARD_NONE;
            in.no_graph = (cfg.flags & ERM_FLAG_NO_GRAPH) != 0; in.profile = cfg.profile != 0; in.stats_valid = stats_valid; in.calibrate = calibrate; in.graph_sweeps = GRAPH_SWEEPS;
            plan = plan_run(in);
        }
        const Plan& P = plan;
        const bool persistent_run = P.persistent;
        // counters, tickets, the persistent launch's wait bound (1 s of the 100 MHz wall clock; 2 ms under the test hook) in ONE small launch, its parameters in pinned memory
        const bool fault = persistent_run && persist_fault_countdown > 0 && --persist_fault_countdown == 0;
        host_run->v = c; host_run->tmo_ticks = fault ? 200000u : 100000000u; host_run->tmo_fault = fault ? 1u : 0u;
        volatile unsigned int* h_tmo = reinterpret_cast<volatile unsigned int*>(&host_ctl[3]);
        *h_tmo = 0u;
        n_pass_timed = 0; n_brackets = 0; bracket_launches.clear(); bracket_open = false;
        // run-begin and run-end stand outside the call's own event pair when they are launches of their own (inside it when the call's graphs hold them)
        const int first = P.step[0].kind == STEP_RUN_BEGIN ? 1 : 0, last = P.step[P.n - 1].kind == STEP_RUN_END ? P.n - 1 : P.n;
        auto enqueue = [&](int from, int to) -> int {
            if (from == to) return 0;
            if (int rc = run_model(P, from, to)) return rc;
            HIPCHK(hipGetLastError());
            return 0;
        };
        if (int rc = enqueue(0, first)) return rc;
        if (persistent_run) { snap_stats_valid = stats_valid; if (int rc = snap_copy(false)) return rc; }
        if (calibrate) {   // empty event pairs, once per engine: the bracketing overhead that is subtracted from every timed launch
            for (int k = 0; k < 16; ++k) { HIPCHK(hipEventRecord(pass_ev[pass_ev.size() - 2 - 2 * k], stream)); HIPCHK(hipEventRecord(pass_ev[pass_ev.size() - 1 - 2 * k], stream)); }
        }
        // persistent launches of one process take turns on a device (see g_persist_mu); held until the stream has drained
        std::unique_lock<std::mutex> turn;
        if (persistent_run) turn = std::unique_lock<std::mutex>(g_persist_mu[(unsigned)cfg.device % 64u]);
        // (a one-graph call in profile mode: its bracket IS the call -- two event records ahead of the graph's launch instead of one keep the device idle 4 us longer)
        const bool own_events = !(P.step[0].kind == STEP_FULL && P.step[0].stride > 0 && pass_ev.size() >= 66);
        if (own_events) HIPCHK(hipEventRecord(ev0, stream));
        if (int rc = enqueue(first, last)) return rc;
        if (own_events) HIPCHK(hipEventRecord(ev1, stream));
        // the counters of both buffers and the time-out word, stored into pinned host memory by one small launch (no copy operations)
        if (int rc = enqueue(last, P.n)) return rc;
        HIPCHK(hipStreamSynchronize(stream));
        if (turn.owns_lock()) turn.unlock();
        if (*h_tmo != 0u) {
            g_err = "the persistent sweep kernel timed out waiting for another workgroup's statistics (its workgroups were not all resident)";
            return persistent_run ? ERM_PERSIST_TIMEOUT : fail(ERM_ERR_STATE, "internal: " + g_err);
        }
        float ms = 0.f;
        if (own_events) HIPCHK(hipEventElapsedTime(&ms, ev0, ev1)); else HIPCHK(hipEventElapsedTime(&ms, pass_ev[0], pass_ev[1]));
        timing.run_ms = ms; timing.sweeps = nsweeps; timing.pass_ms_total = 0.0; timing.pass_launches = n_pass_timed;
        if (calibrate) {
            double t16 = 0.0;
            for (int k = 0; k < 16; ++k) { float t = 0.f; HIPCHK(hipEventElapsedTime(&t, pass_ev[pass_ev.size() - 2 - 2 * k], pass_ev[pass_ev.size() - 1 - 2 * k])); t16 += t; }
            ev_null_ms = t16 / 16.0; ev_calibrated = true;
        }
        const double null_ms = ev_null_ms;
        timing.event_overhead_ms = null_ms;
        for (int64_t k = 0; k < n_brackets; ++k) {   // a bracket holds 1 kernel, one persistent launch, or up to BRACKET_REPLAYS replayed graphs
            float t = 0.f;
            HIPCHK(hipEventElapsedTime(&t, pass_ev[2 * k], pass_ev[2 * k + 1]));
            timing.pass_ms_total += std::max(0.0, (double)t - null_ms);
        }
        Ctl back = host_ctl[1 + cur];
        back.err = host_ctl[1].err;                  // the sticky flag lives in buffer 0
        {   // the diagnostic counters (ERM_PASS_STOP=9 of a diagnostic build) accumulate in whichever buffer a launch read: add the other one
            const Ctl& b1 = host_ctl[1 + (1 - cur)];
            back.dbg_attempts += b1.dbg_attempts; back.dbg_trips += b1.dbg_trips; back.dbg_cells += b1.dbg_cells;
        }
        const int64_t burn = (int64_t)cfg.n_burnin * cfg.n_chain;
        const int64_t lo = std::max<int64_t>(rows_done, burn), hi = rows_done + nsweeps;
        if (hi > lo) post_rows += hi - lo;
        rows_done += nsweeps;
        sweeps_total += (uint32_t)nsweeps;
        if (diag_stop("ERM_PASS_STOP") == 9)
            fprintf(stderr, "[erm dbg] attempts %llu cells %llu wave-trips %llu -> attempts/cell %.4f, lane efficiency %.4f\n", back.dbg_attempts, back.dbg_cells, back.dbg_trips,
                    (double)back.dbg_attempts / (double)back.dbg_cells, (double)back.dbg_attempts / (64.0 * (double)back.dbg_trips));
        if (dDbgTs.p) {      // per-wave phase timeline of the LAST launch (us since the workgroup's first stamp)
            std::vector<unsigned long long> ts(2 * 16 * 16);
            HIPCHK(hipMemcpy(ts.data(), dDbgTs.p, ts.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
            static const char* names[16] = {"start", "B1", "B3", "struct", "sums", "ready", "draws", "PG", "barrier", "gstats", "phase2", "slab", "ticket", "end", "hd-str0", "hd-item"};
            for (int b = 0; b < 2; ++b) {
                unsigned long long t0 = ~0ull;
                for (int w = 0; w < 16; ++w) if (ts[(b * 16 + w) * 16] && ts[(b * 16 + w) * 16] < t0) t0 = ts[(b * 16 + w) * 16];
                fprintf(stderr, "[erm timeline] workgroup %s\n  wave", b == 0 ? "0" : "grid/2");
                for (int k = 0; k < 16; ++k) fprintf(stderr, " %7s", names[k]);
                fprintf(stderr, "\n");
                for (int w = 0; w < 16; ++w) {
                    fprintf(stderr, "  %4d", w);
                    for (int k = 0; k < 16; ++k) { const unsigned long long v = ts[(b * 16 + w) * 16 + k]; fprintf(stderr, " %7.2f", v ? (double)(v - t0) * 0.01 : -1.0); }
                    fprintf(stderr, "\n");
                }
            }
        }
        stats_valid = back.err == 0;
        if (back.err) {
            const int e = (int)back.err - 1;
            std::string what = e < par_off_sigp(J) ? std::string(FIELDS[e / J].name) + "[" + std::to_string(e % J) + "]"
                             : (e < par_off_beta(J) ? "Sigp[" + std::to_string(e - par_off_sigp(J)) + "]" : "beta[" + std::to_string(e - par_off_beta(J)) + "]");
            return fail(ERM_ERR_NONFINITE, "non-finite parameter " + what + " at sweep " + std::to_string(back.sweep));
        }
        return 0;
    }

    int reset_trace() override {
        rows_done = 0; post_rows = 0;
        // on the engine's own stream: ordered after the run that filled the sums and before the next one (a NULL-stream fill is ordered with neither)
        HIPCHK(hipSetDevice(cfg.device));
        HIPCHK(hipMemsetAsync(dSumTheta.p, 0, dSumTheta.bytes, stream));
        HIPCHK(hipMemsetAsync(dSumZeta.p, 0, dSumZeta.bytes, stream));
        if (dSumNu.p) HIPCHK(hipMemsetAsync(dSumNu.p, 0, dSumNu.bytes, stream));
        if (int rc = pw_clear()) return rc;
        return pred_clear();
    }

    // -------------------------------------------------------------------------------------------- data
    // InputData (src/Base.pl.jl:67-78) -> the resident data set.  The column-major host arrays are uploaded as they are and turned into the
    // engine's row-major buffers ON the device (transposition, column sums, centring of logT by its column means, centred sums of squares);
    // the host only adds up per-workgroup partial sums in a fixed order and forms x'x (N p^2 flops).
    int set_data(const uint8_t* Y, const double* logT, const double* X) override {
        if (!Y) return fail(ERM_ERR_ARG, "Y is NULL");
        if (is_rt() && !logT) return fail(ERM_ERR_ARG, "logT is required for response-time models");
        if (Fk > 0 && !X) return fail(ERM_ERR_ARG, "X is required when n_feat > 0");
        HIPCHK(hipSetDevice(cfg.device));
        HIPCHK(hipStreamSynchronize(stream));
        // the resident buffers are overwritten from here on: until this call succeeds the engine holds NO data set (a rejected Y / logT must
        // not leave the previous set's flags -- and its statistics -- standing over the new bytes)
        has_data = false; stats_valid = false;
        const size_t NJ = (size_t)N * J;
        const double Ntot = sharded() ? (double)n_total : (double)N;      // a shard's column sums are completed over the devices
        const int pp = p();
        std::vector<double> cst(cst_size(J), 0.0);
        std::vector<double> g1((size_t)2 * J + PMAX * PMAX, 0.0);         // K0 | column sums of logT | x'x : summed over the devices
        DevBuf dYc, dLc, dStat, dFlag;
        if (int rc = dYc.alloc(NJ)) return rc;
        H2D(dYc.p, Y, NJ);
        if (is_rt()) { if (int rc = dLc.alloc(NJ * sizeof(double))) return rc; H2D(dLc.p, logT, NJ * sizeof(double)); }
        if (int rc = dStat.alloc((size_t)2 * J * sizeof(double))) return rc;
        if (int rc = dFlag.alloc(sizeof(unsigned int))) return rc;
        hipLaunchKernelGGL(colstats_cm_kernel, dim3(J), dim3(256), 0, stream, dYc.as<uint8_t>(), dLc.as<double>(), (long long)N, is_rt() ? 1 : 0, dStat.as<double>(), J, dFlag.as<unsigned int>());
        const dim3 tgrid((unsigned)((N + 31) / 32), (unsigned)((J + 31) / 32));
        hipLaunchKernelGGL((to_rows_kernel<uint8_t, uint8_t>), tgrid, dim3(256), 0, stream, dYc.as<uint8_t>(), (long long)N, J, (const double*)nullptr, dY.as<uint8_t>());
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(stream));
        {
            unsigned int flags = 0;
            HIPCHK(hipMemcpy(&flags, dFlag.p, sizeof(flags), hipMemcpyDeviceToHost));
            if (flags & 1u) return fail(ERM_ERR_ARG, "Y must be 0/1");
            if (flags & 2u) return fail(ERM_ERR_ARG, "logT must be finite");
            HIPCHK(hipMemcpy(g1.data(), dStat.p, (size_t)2 * J * sizeof(double), hipMemcpyDeviceToHost));      // K0 | column sums of logT
        }
        for (int u = 0; u < pp; ++u) for (int v = u; v < pp; ++v) {     // x'x with x = [1 X]
            double t = 0.0;
            if (u == 0 && v == 0) t = (double)N;
            else if (u == 0) { const double* xv = X + (size_t)(v - 1) * N; for (int64_t i = 0; i < N; ++i) t += xv[i]; }
            else { const double* xu = X + (size_t)(u - 1) * N; const double* xv = X + (size_t)(v - 1) * N; for (int64_t i = 0; i < N; ++i) t += xu[i] * xv[i]; }
            g1[(size_t)2 * J + u + v * PMAX] = t; g1[(size_t)2 * J + v + u * PMAX] = t;
        }
        if (int rc = shard_allsum(g1)) return rc;
        for (int j = 0; j < J; ++j) cst[cst_off_k0(J) + j] = g1[j];
        if (is_rt()) {
            // column-centred logT; mean/std(Data.logT) are the kwargs of drawItemIntensity (src/Draw.pl.jl:215)
            std::vector<double> mean(J), g2(J, 0.0);
            double tot = 0.0;
            for (int j = 0; j < J; ++j) { tot += g1[(size_t)J + j]; mean[j] = g1[(size_t)J + j] / Ntot; cst[cst_off_m(J) + j] = mean[j]; }
            DevBuf dMean, dPart;
            const int NB = 256;
            if (int rc = dMean.alloc((size_t)J * sizeof(double))) return rc;
            if (int rc = dPart.alloc((size_t)NB * J * sizeof(double))) return rc;
            H2D(dMean.p, mean.data(), (size_t)J * sizeof(double));
            hipLaunchKernelGGL((to_rows_kernel<double, real>), tgrid, dim3(256), 0, stream, dLc.as<double>(), (long long)N, J, dMean.as<double>(), dC.as<real>());
            hipLaunchKernelGGL((colsq_kernel<real>), dim3(NB), dim3(128), 0, stream, dC.as<real>(), (long long)N, J, dPart.as<double>());
            HIPCHK(hipGetLastError());
            HIPCHK(hipStreamSynchronize(stream));
            std::vector<double> part((size_t)NB * J);
            HIPCHK(hipMemcpy(part.data(), dPart.p, part.size() * sizeof(double), hipMemcpyDeviceToHost));
            for (int j = 0; j < J; ++j) { double sq = 0.0; for (int b = 0; b < NB; ++b) sq += part[(size_t)b * J + j]; g2[j] = sq; }
            if (int rc = shard_allsum(g2)) return rc;
            for (int j = 0; j < J; ++j) cst[cst_off_csq(J) + j] = g2[j];
            const double mu = tot / (Ntot * (double)J);
            double ss = 0.0;
            for (int j = 0; j < J; ++j) { const double dm = cst[cst_off_m(J) + j] - mu; ss += cst[cst_off_csq(J) + j] + Ntot * dm * dm; }
            cst[cst_off_mu(J)] = mu; cst[cst_off_mu(J) + 1] = std::sqrt(ss / (Ntot * (double)J - 1.0));
        }
        {   // X -> row-major
            for (int u = 0; u < pp; ++u) for (int v = 0; v < pp; ++v) cst[cst_off_xtx(J) + u + v * PMAX] = g1[(size_t)2 * J + u + v * PMAX];
            if (int rc = invert_xtx(cst)) return rc;
            if (Fk > 0) {
                DevBuf dXc;
                if (int rc = dXc.alloc((size_t)N * Fk * sizeof(double))) return rc;
                H2D(dXc.p, X, (size_t)N * Fk * sizeof(double));
                hipLaunchKernelGGL((to_rows_kernel<double, real>), dim3((unsigned)((N + 31) / 32), (unsigned)((Fk + 31) / 32)), dim3(256), 0, stream, dXc.as<double>(), (long long)N, Fk,
                                   (const double*)nullptr, dX.as<real>());
                HIPCHK(hipGetLastError());
                HIPCHK(hipStreamSynchronize(stream));
            }
        }
        H2D(dCst.p, cst.data(), cst.size() * sizeof(double));
        has_data = true;
        stats_valid = false;
        return 0;
    }

    // (x'x)^-1 by Gauss-Jordan with partial pivoting (fp64, p <= PMAX); x'x is in cst at cst_off_xtx with leading dimension PMAX
    int invert_xtx(std::vector<double>& cst) {
        const int pp = p();
        std::vector<double> M((size_t)pp * 2 * pp, 0.0);
        for (int i = 0; i < pp; ++i) { for (int jx = 0; jx < pp; ++jx) M[(size_t)i * 2 * pp + jx] = cst[cst_off_xtx(J) + i + jx * PMAX]; M[(size_t)i * 2 * pp + pp + i] = 1.0; }
        for (int c = 0; c < pp; ++c) {
            int piv = c;
            for (int r = c + 1; r < pp; ++r) if (std::fabs(M[(size_t)r * 2 * pp + c]) > std::fabs(M[(size_t)piv * 2 * pp + c])) piv = r;
            if (!(std::fabs(M[(size_t)piv * 2 * pp + c]) > 0.0)) return fail(ERM_ERR_ARG, "x'x is singular (collinear covariates)");
            if (piv != c) for (int jx = 0; jx < 2 * pp; ++jx) std::swap(M[(size_t)c * 2 * pp + jx], M[(size_t)piv * 2 * pp + jx]);
            const double d = M[(size_t)c * 2 * pp + c];
            for (int jx = 0; jx < 2 * pp; ++jx) M[(size_t)c * 2 * pp + jx] /= d;
            for (int r = 0; r < pp; ++r) if (r != c) {
                const double f = M[(size_t)r * 2 * pp + c];
                if (f != 0.0) for (int jx = 0; jx < 2 * pp; ++jx) M[(size_t)r * 2 * pp + jx] -= f * M[(size_t)c * 2 * pp + jx];
            }
        }
        for (int i = 0; i < pp; ++i) for (int jx = 0; jx < pp; ++jx) cst[cst_off_xinv(J) + i + jx * PMAX] = M[(size_t)i * 2 * pp + pp + jx];
        return 0;
    }

    // -------------------------------------------------------------------------------------------- synthetic data on the device
    DevBuf dTruthTheta, dTruthZeta;
    std::vector<double> col_mean;      // column means of logT (kept for erm_get_data)
    int simulate_data(const erm_state* tr, uint64_t seed, int noise) override {
        if (sharded()) return fail(ERM_ERR_STATE, "erm_simulate_data is not available on a shard");
        if (!tr || !tr->a || !tr->b) return fail(ERM_ERR_ARG, "truth needs a and b");
        if (is_rt() && (!tr->lambda || !tr->sig2t)) return fail(ERM_ERR_ARG, "truth needs lambda and sig2t for response-time models");
        if (noise < 0 || noise > 2) return fail(ERM_ERR_ARG, "noise must be 0 (norm), 1 (tail) or 2 (skew)");
        const int gen = mt().gen;
        if ((gen == GEN_MLIRT || gen == GEN_RTIRT || gen == GEN_LATENT) && Fk > 0 && !tr->beta) return fail(ERM_ERR_ARG, "truth needs beta");
        if (gen == GEN_CROSS && !tr->rho) return fail(ERM_ERR_ARG, "truth needs rho");
        HIPCHK(hipSetDevice(cfg.device));
        HIPCHK(hipStreamSynchronize(stream));
        has_data = false; stats_valid = false;
        // truth vector: a b lambda sig2t rho | chol(Sigp) | beta
        std::vector<double> tv((size_t)5 * J + 3 + 2 * PMAX + 2, 0.0);
        for (const auto& f : FIELDS) { const double* src = tr->*f.member; for (int j = 0; j < J; ++j) tv[f.off(J) + j] = src ? src[j] : f.init; }
        for (int j = 0; j < J; ++j) if (is_rt() && !(tv[PAR_SIG2T * J + j] > 0.0)) return fail(ERM_ERR_ARG, "sig2t must be positive");
        double S00 = 1.0, S10 = 0.0, S11 = 1.0;
        if (tr->sigp) { S00 = tr->sigp[0]; S10 = tr->sigp[1]; S11 = tr->sigp[3]; }
        if (!(S00 > 0.0) || !(S11 - S10 * S10 / S00 > 0.0)) return fail(ERM_ERR_ARG, "Sigp must be positive definite");
        tv[5 * J] = std::sqrt(S00); tv[5 * J + 1] = S10 / tv[5 * J]; tv[5 * J + 2] = std::sqrt(S11 - tv[5 * J + 1] * tv[5 * J + 1]);
        // beta: the generators' truth has no intercept row (src/SimTools.jl:86,107,283): RtIrt [nFeat][2] column-major -> (f, c) at 2f + c
        double* bt = &tv[5 * J + 3];
        if (tr->beta) {
            if (gen == GEN_RTIRT) for (int f = 0; f < Fk; ++f) { bt[2 * f] = tr->beta[f]; bt[2 * f + 1] = tr->beta[Fk + f]; }
            else if (gen == GEN_MLIRT) for (int f = 0; f < Fk; ++f) bt[f] = tr->beta[f];
            else if (gen == GEN_LATENT) for (int f = 0; f <= Fk; ++f) bt[f] = tr->beta[f];
        }
        DevBuf dT;
        if (int rc = dT.alloc(tv.size() * sizeof(double))) return rc;
        H2D(dT.p, tv.data(), tv.size() * sizeof(double));
        if (!dTruthTheta.p) { if (int rc = dTruthTheta.alloc((size_t)N * sizeof(double))) return rc; if (int rc = dTruthZeta.alloc((size_t)N * sizeof(double))) return rc; }
        GenArgs g{};
        g.Y = dY.as<uint8_t>(); g.C = dC.p; g.X = dX.p; g.theta = dTruthTheta.as<double>(); g.zeta = dTruthZeta.as<double>();
        g.truth = dT.as<double>(); g.N = N; g.J = J; g.F = Fk; g.gen = gen; g.noise = noise; g.seed = seed;
        hipLaunchKernelGGL((gen_kernel<real>), dim3((unsigned)((N + 127) / 128)), dim3(128), 0, stream, g);
        // ---- constants of the data set (the same as erm_set_data's): K0, column means / centred squares of logT, x'x and its inverse
        const int NB = 256, pp = p(), PW = 3 * J + pp * pp;
        DevBuf dPart, dMean, dPart2;
        if (int rc = dPart.alloc((size_t)NB * PW * sizeof(double))) return rc;
        hipLaunchKernelGGL((colsum_kernel<real>), dim3(NB), dim3(128), 0, stream, dY.as<uint8_t>(), dC.as<real>(), dX.as<real>(), (long long)N, J, Fk,
                           is_rt() ? 1 : 0, dPart.as<double>());
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(stream));
        std::vector<double> part((size_t)NB * PW), cst(cst_size(J), 0.0);
        HIPCHK(hipMemcpy(part.data(), dPart.p, part.size() * sizeof(double), hipMemcpyDeviceToHost));
        col_mean.assign(J, 0.0);
        for (int j = 0; j < J; ++j) {
            double sk = 0.0, s1 = 0.0;
            for (int b = 0; b < NB; ++b) { sk += part[(size_t)b * PW + j]; s1 += part[(size_t)b * PW + J + j]; }
            cst[cst_off_k0(J) + j] = sk; col_mean[j] = s1 / (double)N; cst[cst_off_m(J) + j] = col_mean[j];
        }
        for (int e = 0; e < pp * pp; ++e) { double t = 0.0; for (int b = 0; b < NB; ++b) t += part[(size_t)b * PW + 3 * J + e]; cst[cst_off_xtx(J) + (e % pp) + (e / pp) * PMAX] = t; }
        if (int rc = invert_xtx(cst)) return rc;
        if (is_rt()) {
            if (int rc = dMean.alloc((size_t)J * sizeof(double))) return rc;
            if (int rc = dPart2.alloc((size_t)NB * J * sizeof(double))) return rc;
            H2D(dMean.p, col_mean.data(), (size_t)J * sizeof(double));
            hipLaunchKernelGGL((center_kernel<real>), dim3(NB), dim3(128), 0, stream, dC.as<real>(), (long long)N, J, dMean.as<double>(), dPart2.as<double>());
            HIPCHK(hipGetLastError());
            HIPCHK(hipStreamSynchronize(stream));
            std::vector<double> p2((size_t)NB * J);
            HIPCHK(hipMemcpy(p2.data(), dPart2.p, p2.size() * sizeof(double), hipMemcpyDeviceToHost));
            double tot = 0.0;
            for (int j = 0; j < J; ++j) { double sq = 0.0; for (int b = 0; b < NB; ++b) sq += p2[(size_t)b * J + j]; cst[cst_off_csq(J) + j] = sq; tot += col_mean[j]; }
            const double mu = tot / (double)J;              // equal column lengths: the grand mean is the mean of the column means
            double ss = 0.0;
            for (int j = 0; j < J; ++j) { const double dm = col_mean[j] - mu; ss += cst[cst_off_csq(J) + j] + (double)N * dm * dm; }
            cst[cst_off_mu(J)] = mu; cst[cst_off_mu(J) + 1] = std::sqrt(ss / ((double)N * J - 1.0));
        }
        H2D(dCst.p, cst.data(), cst.size() * sizeof(double));
        has_data = true;
        stats_valid = false;
        return 0;
    }
    // the resident data set back in the caller's (column-major) layout: Y bytes, logT = centred value + column mean, X
    int get_data(uint8_t* Y, double* logT, double* X) override {
        if (!has_data) return fail(ERM_ERR_STATE, "no data set is resident");
        HIPCHK(hipSetDevice(cfg.device));
        HIPCHK(hipStreamSynchronize(stream));
        const size_t NJ = (size_t)N * J;
        if (Y) { std::vector<uint8_t> t(NJ); HIPCHK(hipMemcpy(t.data(), dY.p, NJ, hipMemcpyDeviceToHost)); rows_to_cols(t.data(), Y, N, J); }
        if (logT && is_rt()) {
            std::vector<double> cst(cst_size(J));
            HIPCHK(hipMemcpy(cst.data(), dCst.p, cst.size() * sizeof(double), hipMemcpyDeviceToHost));
            std::vector<real> t(NJ);
            HIPCHK(hipMemcpy(t.data(), dC.p, NJ * sizeof(real), hipMemcpyDeviceToHost));
            rows_to_cols(t.data(), logT, N, J, [&](real v, int64_t j) { return (double)v + cst[cst_off_m(J) + j]; });
        }
        if (X && Fk > 0) { std::vector<real> t((size_t)N * Fk); HIPCHK(hipMemcpy(t.data(), dX.p, t.size() * sizeof(real), hipMemcpyDeviceToHost)); rows_to_cols(t.data(), X, N, Fk); }
        return 0;
    }
    int get_truth(double* theta, double* zeta) override {
        if (!dTruthTheta.p) return fail(ERM_ERR_STATE, "erm_simulate_data has not been called");
        HIPCHK(hipSetDevice(cfg.device));
        HIPCHK(hipStreamSynchronize(stream));
        if (theta) HIPCHK(hipMemcpy(theta, dTruthTheta.p, (size_t)N * sizeof(double), hipMemcpyDeviceToHost));
        if (zeta) HIPCHK(hipMemcpy(zeta, dTruthZeta.p, (size_t)N * sizeof(double), hipMemcpyDeviceToHost));
        return 0;
    }

    int up_real(DevBuf& d, const double* src, size_t n) {
        std::vector<real> t(n);
        for (size_t k = 0; k < n; ++k) t[k] = (real)src[k];
        H2D(d.p, t.data(), n * sizeof(real));
        return 0;
    }
    int down_real(const DevBuf& d, double* dst, size_t n) {
        std::vector<real> t(n);
        HIPCHK(hipMemcpy(t.data(), d.p, n * sizeof(real), hipMemcpyDeviceToHost));
        for (size_t k = 0; k < n; ++k) dst[k] = (double)t[k];
        return 0;
    }

    int set_state(const erm_state* st) override {
        if (!st) return fail(ERM_ERR_ARG, "state is NULL");
        HIPCHK(hipSetDevice(cfg.device));
        HIPCHK(hipStreamSynchronize(stream));
        poisoned = false;
        stats_valid = false;
        std::vector<double> par(par_size(J));
        HIPCHK(hipMemcpy(par.data(), dParB[cur].p, par.size() * sizeof(double), hipMemcpyDeviceToHost));
        for (const auto& f : FIELDS) {
            const double* src = st->*f.member;
            if (!src) continue;
            if (f.k == PAR_SIG2T) for (int j = 0; j < J; ++j) if (!(src[j] > 0.0)) return fail(ERM_ERR_ARG, "sig2t must be positive");
            memcpy(&par[f.off(J)], src, J * sizeof(double));
        }
        if (st->sigp) memcpy(&par[par_off_sigp(J)], st->sigp, 4 * sizeof(double));
        if (st->beta) beta_pack(mt().beta, F, st->beta, &par[par_off_beta(J)]);
        { double t = 0.0; for (int j = 0; j < J; ++j) t += 1.0 / par[PAR_SIG2T * J + j]; par[par_off_derived(J)] = t; }
        H2D(dParB[cur].p, par.data(), par.size() * sizeof(double));
        if (st->theta) if (int rc = up_real(dTheta, st->theta, N)) return rc;
        if (st->zeta) if (int rc = up_real(dZeta, st->zeta, N)) return rc;
        if (st->nu && dNu.p) {
            if (mt().nu == NU_SUBJECT) { if (int rc = up_real(dNu, st->nu, N)) return rc; }
            else {
                std::vector<real> t((size_t)N * J);
                if (!cols_to_rows(st->nu, t.data(), N, J, AsIs(), [](double v) { return v > 0.0; })) return fail(ERM_ERR_ARG, "nu must be positive");   // @assert src/Draw.pl.jl:477
                H2D(dNu.p, t.data(), t.size() * sizeof(real));
            }
        }
        return 0;
    }

    int get_state(erm_state* st) override {
        if (!st) return fail(ERM_ERR_ARG, "state is NULL");
        if (poisoned) return fail(ERM_ERR_STATE, "a previous erm_run failed part-way: the state is undefined until erm_set_state");
        HIPCHK(hipSetDevice(cfg.device));
        HIPCHK(hipStreamSynchronize(stream));
        std::vector<double> par(par_size(J));
        HIPCHK(hipMemcpy(par.data(), dParB[cur].p, par.size() * sizeof(double), hipMemcpyDeviceToHost));
        for (const auto& f : FIELDS) if (double* dst = st->*f.member) memcpy(dst, &par[f.off(J)], J * sizeof(double));
        if (st->sigp) memcpy(st->sigp, &par[par_off_sigp(J)], 4 * sizeof(double));
        if (st->beta) beta_unpack(mt().beta, F, &par[par_off_beta(J)], st->beta);
        if (st->theta) if (int rc = down_real(dTheta, st->theta, N)) return rc;
        if (st->zeta) if (int rc = down_real(dZeta, st->zeta, N)) return rc;
        if (st->nu && dNu.p) {
            if (mt().nu == NU_SUBJECT) { if (int rc = down_real(dNu, st->nu, N)) return rc; }
            else {
                std::vector<real> t((size_t)N * J);
                HIPCHK(hipMemcpy(t.data(), dNu.p, t.size() * sizeof(real), hipMemcpyDeviceToHost));
                rows_to_cols(t.data(), st->nu, N, J);
            }
        }
        return 0;
    }

    // -------------------------------------------------------------------------------------------- traces
    int fetch_item_trace(std::vector<double>& it) {
        it.resize((size_t)std::max<int64_t>(rows_done, 0) * item_trace_width());
        if (!it.empty()) HIPCHK(hipMemcpy(it.data(), dTrItem.p, it.size() * sizeof(double), hipMemcpyDeviceToHost));
        return 0;
    }
    int get_item_trace(double* out) override {
        HIPCHK(hipSetDevice(cfg.device));
        std::vector<double> it;
        if (int rc = fetch_item_trace(it)) return rc;
        if (!it.empty()) memcpy(out, it.data(), it.size() * sizeof(double));
        return 0;
    }

    // Julia layout [nIter][width][nChain], nIter fastest; trace row r = m*nChain + l
    int get_trace(int which, double* out) override {
        HIPCHK(hipSetDevice(cfg.device));
        const int64_t nIter = cfg.n_iter, nChain = cfg.n_chain, wd = trace_width(which);
        if (wd <= 0) return fail(ERM_ERR_ARG, "this model has no such trace");
        if (rows_done != rows_cap) return fail(ERM_ERR_STATE, "trace incomplete: run n_iter*n_chain sweeps first");
        auto at = [&](int64_t r, int64_t k) -> double& { const int64_t m = r / nChain, l = r % nChain; return out[m + nIter * (k + wd * l)]; };
        if (which == ERM_TRACE_LOGLIKE) {
            std::vector<double> ll(rows_cap);
            HIPCHK(hipMemcpy(ll.data(), dTrLl.p, rows_cap * sizeof(double), hipMemcpyDeviceToHost));
            for (int64_t r = 0; r < rows_cap; ++r) at(r, 0) = ll[r];
            return 0;
        }
        if (cfg.trace_mode != ERM_TRACE_FULL) return fail(ERM_ERR_NOTRACE, "subject-level traces need trace_mode = ERM_TRACE_FULL");
        const TraceBlocks blocks = trace_blocks(which);
        for (const TraceBlock& b : blocks) if (b.kind == BLK_CELL && !dTrNu.p)
            return fail(ERM_ERR_NOTRACE, "the per-sweep nu trace (N*J values per sweep) exceeds erm_config.nu_trace_max_gb; use erm_get_item_trace (rho, Sigp) + erm_get_mean (nu)");
        std::vector<double> it;
        if (int rc = fetch_item_trace(it)) return rc;
        const int64_t wi = item_trace_width();
        // subject block of a trace: transposed to Julia's iteration-fastest layout ON the device (one chain at a time into a scratch buffer of
        // nSubj x nIter doubles), then ONE contiguous copy per chain; if the scratch buffer cannot be had, row by row through the host
        auto subj = [&](const DevBuf& d, int64_t k0) -> int {
            double* tmp = nullptr;
            const size_t need = (size_t)N * (size_t)nIter * sizeof(double);
            if (hipMalloc(reinterpret_cast<void**>(&tmp), need) == hipSuccess) {
                int rc = 0;
                for (int64_t l = 0; l < nChain && !rc; ++l) {
                    hipLaunchKernelGGL((trace_transpose_kernel<real>), dim3((unsigned)((N + 31) / 32), (unsigned)((nIter + 31) / 32)), dim3(256), 0, stream,
                                       d.as<real>(), (long long)N, (long long)N, (int)nIter, (int)nChain, (int)l, tmp);
                    hipError_t e = hipGetLastError();
                    if (e == hipSuccess) e = hipStreamSynchronize(stream);
                    if (e == hipSuccess) e = hipMemcpy(out + nIter * (k0 + wd * l), tmp, need, hipMemcpyDeviceToHost);
                    if (e != hipSuccess) rc = fail(ERM_ERR_HIP, std::string("trace transpose: ") + hipGetErrorString(e));
                }
                (void)hipFree(tmp);
                return rc;
            }
            (void)hipGetLastError();
            std::vector<real> rowbuf(N);
            for (int64_t r = 0; r < rows_cap; ++r) {
                HIPCHK(hipMemcpy(rowbuf.data(), d.as<real>() + (size_t)r * N, N * sizeof(real), hipMemcpyDeviceToHost));
                for (int64_t i = 0; i < N; ++i) at(r, k0 + i) = (double)rowbuf[i];
            }
            return 0;
        };
        for (const TraceBlock& b : blocks) {
            switch (b.kind) {
            case BLK_SUBJECT: if (int rc = subj(subj_trace(b.src), b.col0)) return rc; break;
            case BLK_CELL: {                    // vec(nu): column-major N x J for the caller
                std::vector<real> cells((size_t)b.ncol);
                for (int64_t r = 0; r < rows_cap; ++r) {
                    HIPCHK(hipMemcpy(cells.data(), dTrNu.as<real>() + (size_t)r * cells.size(), cells.size() * sizeof(real), hipMemcpyDeviceToHost));
                    rows_to_cols(cells.data(), &at(r, b.col0), N, J, AsIs(), nIter);
                }
                break;
            }
            case BLK_ITEM: for (int64_t r = 0; r < rows_cap; ++r) for (int64_t k = 0; k < b.ncol; ++k) at(r, b.col0 + k) = it[r * wi + b.src + k]; break;
            case BLK_ZERO: for (int64_t r = 0; r < rows_cap; ++r) for (int64_t k = 0; k < b.ncol; ++k) at(r, b.col0 + k) = 0.0; break;
            }
        }
        return 0;
    }

    BlockSrc block_src(const TraceBlock& b) const override {
        switch (b.kind) {
        case BLK_SUBJECT: case BLK_CELL: return { subj_trace(b.src).p, b.ncol, sizeof(real) };
        case BLK_ITEM: return { dTrItem.p ? dTrItem.as<double>() + b.src : nullptr, item_trace_width(), sizeof(double) };
        }
        return { nullptr, 0, 0 };
    }
    hipStream_t work_stream() const override { return stream; }

    // item-level means (an item-trace row's layout) -> the fields of Post.mean (src/GibbsRtIrt.pl.jl:249-254, 327-343; Cross :304-318; Latent :316-330)
    void unpack_items(const double* m, erm_state* out) const {
        for (int k = 0; k < item_trace_fields(cfg.model); ++k) if (double* dst = out->*FIELDS[k].member) memcpy(dst, &m[FIELDS[k].off(J)], J * sizeof(double));
        const double* q = &m[4 * J];                  // the kernels' small part of qr: [beta or rho | Sigp at qr_sigp_off]
        if (out->beta && mt().beta == BETA_ZERO_PAIR) memset(out->beta, 0, nbeta() * sizeof(double));
        else if (out->beta) memcpy(out->beta, q, nbeta() * sizeof(double));
        if (out->sigp && is_rt()) memcpy(out->sigp, q + qr_sigp_off(cfg.model, J, F), 4 * sizeof(double));
    }
    // Post.mean of one engine: a farm of one.  Only the blocks `out` asks for are added, copied or transposed (the accumulator ends with the last of them).
    int get_mean(erm_state* out) override {
        if (!out) return fail(ERM_ERR_ARG, "state is NULL");
        HIPCHK(hipSetDevice(cfg.device));
        HIPCHK(hipStreamSynchronize(stream));
        if (post_rows <= 0) return fail(ERM_ERR_STATE, "no post-burn-in sweeps recorded");
        const SummaryLayout L = summary();
        DevBuf acc;
        if (int rc = acc.alloc((size_t)(wants_nu(out) ? L.len : wants_zeta(out) ? L.zeta + N : out->theta ? L.theta + N : L.theta) * sizeof(double))) return rc;
        if (int rc = summary_add(acc.as<double>(), out)) return rc;
        return mean_from_summary(acc.as<double>(), 1.0 / (double)post_rows, out);
    }

    // ---- the summary vector (chain farms, Post.mean, DIC): [item sums (wi) | sum theta (N) | sum zeta (N, response-time models) | sum nu (N or N*J, quantile models)]
    SummaryLayout summary() const { return summary_layout(cfg.model, N, J, F); }
    int64_t summary_len() const override { return summary().len; }
    // the subject-level blocks a request for Post.mean names (want == NULL: all the model has)
    bool wants_zeta(const erm_state* want) const { return is_rt() && (!want || want->zeta); }
    bool wants_nu(const erm_state* want) const { return m_nu() && (!want || want->nu); }
    int summary_add(double* acc, const erm_state* want) override {
        HIPCHK(hipSetDevice(cfg.device));
        auto add = [&](int64_t off, const DevBuf& src, int64_t n) {
            hipLaunchKernelGGL(acc_kernel, dim3((unsigned)std::min<int64_t>((n + 255) / 256, 4096)), dim3(256), 0, stream, acc + off, src.as<double>(), (long long)n);
        };
        // item-level columns: summed over the post-burn-in rows of the resident item trace ON the device, in row order from 0.0
        const int64_t wi = item_trace_width(), burn = (int64_t)cfg.n_burnin * cfg.n_chain;
        hipLaunchKernelGGL(item_sum_kernel, dim3((unsigned)((wi + 255) / 256)), dim3(256), 0, stream, dTrItem.as<double>(), (long long)wi, (long long)std::min(burn, rows_done), (long long)rows_done, acc);
        const SummaryLayout L = summary();
        if (!want || want->theta) add(L.theta, dSumTheta, N);
        if (wants_zeta(want)) add(L.zeta, dSumZeta, N);
        if (wants_nu(want)) add(L.nu, dSumNu, nu_len());
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(stream));
        return 0;
    }
    // the inverse step: the blocks `out` asks for copied down from the accumulated sums `dacc` (this engine's device), scaled by inv, in the caller's layout
    int mean_from_summary(const double* dacc, double inv, erm_state* out) override {
        HIPCHK(hipSetDevice(cfg.device));
        const SummaryLayout L = summary();
        std::vector<double> t;
        auto down = [&](int64_t off, int64_t n, double* dst) -> int {      // dst == NULL: into t
            if (!dst) { t.resize((size_t)n); dst = t.data(); }
            HIPCHK(hipMemcpy(dst, dacc + off, (size_t)n * sizeof(double), hipMemcpyDeviceToHost));
            for (int64_t k = 0; k < n; ++k) dst[k] *= inv;
            return 0;
        };
        if (int rc = down(0, item_trace_width(), nullptr)) return rc;
        unpack_items(t.data(), out);
        if (out->theta) if (int rc = down(L.theta, N, out->theta)) return rc;
        if (wants_zeta(out)) if (int rc = down(L.zeta, N, out->zeta)) return rc;
        if (wants_nu(out)) {
            if (int rc = down(L.nu, nu_len(), mt().nu == NU_CELL ? nullptr : out->nu)) return rc;
            if (mt().nu == NU_CELL) rows_to_cols(t.data(), out->nu, N, J);
        }
        return 0;
    }

    // ---- DIC from device-resident state (include/ertirt.h, erm_get_dic)
    int loglik_at(const double* dsum, double inv, double* ll) override {
        if (!has_data) return fail(ERM_ERR_STATE, "no data set is resident");
        HIPCHK(hipSetDevice(cfg.device));
        const PassGeom g = pgeom();
        const int nb = g.nb_loglik;
        DevBuf dPart;
        if (int rc = dPart.alloc((size_t)nb * sizeof(double))) return rc;
        LogLikArgs D{};
        D.Y = dY.as<uint8_t>(); D.C = dC.p; D.X = dX.p; D.cm = dCst.as<double>() + cst_off_m(J);
        D.sum = dsum; D.inv = inv; D.N = N; D.J = J; D.F = Fk; D.model = cfg.model;
        const SummaryLayout L = summary();
        D.off_theta = L.theta; D.off_zeta = L.zeta; D.off_nu = L.nu;
        const QuantileConsts k = quantile_consts();
        D.k1 = k.k1; D.k2 = k.k2;
        D.rows_per_block = g.rows_per_block; D.part = dPart.as<double>();
        hipLaunchKernelGGL((loglik_kernel<real>), dim3(nb), dim3(PASS_THREADS), g.lds_loglik, stream, D);
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(stream));
        std::vector<double> part(nb);
        HIPCHK(hipMemcpy(part.data(), dPart.p, part.size() * sizeof(double), hipMemcpyDeviceToHost));
        double t = 0.0;
        for (double v : part) t += v;
        *ll = t;
        return 0;
    }
    int ll_trace_sum(double* out) override {
        HIPCHK(hipSetDevice(cfg.device));
        DevBuf d;
        if (int rc = d.alloc(sizeof(double))) return rc;
        hipLaunchKernelGGL(ll_trace_sum_kernel, dim3(1), dim3(256), 0, stream, dTrLl.as<double>(), (long long)rows_done, d.as<double>());
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(stream));
        HIPCHK(hipMemcpy(out, d.p, sizeof(double), hipMemcpyDeviceToHost));
        return 0;
    }
    int get_dic(double* out4) override {
        if (poisoned) return fail(ERM_ERR_STATE, "a previous erm_run failed part-way: the state is undefined until erm_set_state");
        if (sharded()) return fail(ERM_ERR_STATE, "erm_get_dic is not available on a shard (the log-likelihood at Post.mean needs every subject)");
        if (rows_done <= 0 || post_rows <= 0) return fail(ERM_ERR_STATE, "no post-burn-in sweeps recorded");
        HIPCHK(hipSetDevice(cfg.device));
        DevBuf acc;
        if (int rc = acc.alloc((size_t)summary_len() * sizeof(double))) return rc;
        if (int rc = summary_add(acc.as<double>(), nullptr)) return rc;
        EngineBase* self = this;
        return dic_from_summary(&self, 1, acc.as<double>(), post_rows, out4);
    }
    int set_seed(uint64_t seed) override {
        HIPCHK(hipSetDevice(cfg.device));
        HIPCHK(hipStreamSynchronize(stream));
        cfg.seed = seed;
        sweeps_total = 0;            // a new seed starts a new chain: its streams are addressed from sweep 1, as a freshly created engine's are
        drop_graphs();               // the captured launches carry the seed as a kernel argument
        stats_valid = false;         // the resident omega_{t+1} / nu_{t+1} were drawn from the old streams: the next run draws them again
        return pred_clear();         // the replicates of the old chain do not mix with the new one's
    }
};

}  // namespace

struct erm_engine { std::unique_ptr<EngineBase> e; };

// Chain farm (first bullet; north_star): nChain INDEPENDENT chains, chain l on device devices[l] with random stream
// chain_id = l and its own copy of the data; one host thread per chain drives its engine's stream; no communication while sampling.
// Post.mean (src/GibbsRtIrt.pl.jl:327-343: mean over iterations AND chains jointly) = (sum over chains of their post-burn-in sums) /
// (total rows): the sums of the chains that share a device are added on that device, the devices' vectors are summed by ONE
// ncclAllReduce over RCCL (xGMI), and device 0's copy is divided by the count.
struct erm_farm {
    erm_config cfg{};
    std::vector<std::unique_ptr<erm_engine>> eng;      // eng[l]: chain l
    std::vector<int> dev;                                // dev[l]: its device
    std::vector<int> udev;                               // distinct devices, in order of first use
    std::vector<ncclComm_t> comms;                       // one communicator rank per distinct device (empty until the first reduction over > 1 device)
    std::vector<hipStream_t> rstream;                    // one stream per distinct device for the reduction (never the NULL stream: the engines' streams are non-blocking)
    bool used_rccl = false;
    erm_farm_timing tm{};
    ~erm_farm() {
        stop_workers();
        for (auto c : comms) if (c) (void)g_rccl.CommDestroy(c);
        for (size_t d = 0; d < rstream.size(); ++d) if (rstream[d]) { (void)hipSetDevice(udev[d]); (void)hipStreamDestroy(rstream[d]); }
    }
    // One PERSISTENT host thread per chain (created with the farm, joined by its destructor): erm_farm_run / set_data / get_trace hand each chain's
    // call to its thread and wait.  (Creating the threads per call cost ~25 us per chain -- an eighth of a 20-sweep erm_farm_run on eight GPUs.)
    struct Worker {
        std::thread th;
        std::mutex mu;
        std::condition_variable cv;
        std::function<int()> job;
        bool has_job = false, done = false, quit = false;
        int rc = 0;
        std::string msg;
    };
    std::vector<std::unique_ptr<Worker>> workers;
    void start_workers() {
        for (size_t l = workers.size(); l < eng.size(); ++l) {
            workers.emplace_back(new Worker());
            Worker* w = workers.back().get();
            w->th = std::thread([w] {
                std::unique_lock<std::mutex> lk(w->mu);
                for (;;) {
                    w->cv.wait(lk, [w] { return w->has_job || w->quit; });
                    if (w->quit) return;
                    w->has_job = false;
                    lk.unlock();
                    const int rc = w->job();
                    const std::string m = rc ? g_err : std::string();      // g_err is thread-local: the chain's message lives in THIS thread
                    lk.lock();
                    w->rc = rc; w->msg = m; w->done = true;
                    w->cv.notify_all();
                }
            });
        }
    }
    void stop_workers() {
        for (auto& w : workers) {
            { std::lock_guard<std::mutex> lk(w->mu); w->quit = true; }
            w->cv.notify_all();
            if (w->th.joinable()) w->th.join();
        }
        workers.clear();
    }
    // runs f(l) for every chain on the chain's thread; returns the first non-zero code (its message becomes the calling thread's last error)
    template <typename Fn> int parallel(Fn&& f) {
        const int n = (int)eng.size();
        start_workers();
        for (int l = 0; l < n; ++l) {
            Worker* w = workers[l].get();
            { std::lock_guard<std::mutex> lk(w->mu); w->job = [&f, l] { return f(l); }; w->done = false; w->has_job = true; }
            w->cv.notify_all();
        }
        int first = -1;
        for (int l = 0; l < n; ++l) {
            Worker* w = workers[l].get();
            std::unique_lock<std::mutex> lk(w->mu);
            w->cv.wait(lk, [w] { return w->done; });
            if (w->rc && first < 0) first = l;
        }
        if (first >= 0) return fail(workers[first]->rc, "chain " + std::to_string(first) + ": " + workers[first]->msg);
        return 0;
    }
};

// erm_debug_rank_diagnostics / erm_debug_diagnostics: caller-supplied draws through the kernels the engine runs on its traces.  The upload: Julia layout
// x[m + n_draw (k + n_col l)] -> the engine's trace layout [row = m n_chain + l][column k] in the engine's trace type
template <typename T>
static int debug_upload(const double* x, int64_t n_draw, int64_t n_col, int32_t n_chain, DevBuf& dTr)
{
    std::vector<T> tr((size_t)n_draw * n_col * n_chain);
    for (int64_t l = 0; l < n_chain; ++l) for (int64_t k = 0; k < n_col; ++k) for (int64_t m = 0; m < n_draw; ++m)
        tr[(size_t)((m * n_chain + l) * n_col + k)] = (T)x[m + n_draw * (k + n_col * l)];
    if (int rc = dTr.try_alloc(tr.size() * sizeof(T), "the draws")) return rc;
    H2D(dTr.p, tr.data(), tr.size() * sizeof(T));
    return 0;
}

#include "erm_diagnostics.hpp"             // the convergence diagnostics' host path: the engine's, the farm's and the debug entries'
#include "erm_item_pass.hpp"               // the six item-trace passes' host path: marginal WAIC and LOO, scores, plausible values, person fit, item fit

namespace {
// an engine as the source of a pass (EngineBase::item_source)
template <typename real> int Engine<real>::item_source(int pass, ItemSource& S)
{
    if (sharded()) return fail(ERM_ERR_STATE, item_pass_on_shard(pass));
    if (poisoned) return fail(ERM_ERR_STATE, "a previous erm_run failed part-way: the state is undefined until erm_set_state");
    if (!has_data) return fail(ERM_ERR_STATE, "no data set is resident");
    if (!S.rows) {
        if (post_rows < ITEM_PASSES[pass].engine_rows) return fail(ERM_ERR_STATE, item_pass_needs_rows(pass));
        S.rows = dTrItem.as<double>() + (size_t)(rows_done - post_rows) * item_trace_width(); S.n_rows = post_rows;
    }
    HIPCHK(hipSetDevice(cfg.device));
    S.D = MargData{dY.as<uint8_t>(), dC.p, dX.p, is_rt() ? dCst.as<double>() + cst_off_m(J) : nullptr, N, J, Fk, cfg.model, sizeof(real), cfg.q_rt};
    S.stream = stream;
    return 0;
}
// what every entry of a pass checks first: its output, the node count -- and the plausible values' the number of draws
static int item_entry_args(const void* out, int32_t n_nodes, int* Q)
{
    if (!out) return fail(ERM_ERR_ARG, "out is NULL");
    return marg_nodes(n_nodes, Q);
}
static int pv_entry_args(int32_t n_nodes, int32_t n_draws, const double* pv, int* Q)
{
    if (int rc = item_entry_args(pv, n_nodes, Q)) return rc;
    if (!pv_draws_ok(n_draws)) return fail(ERM_ERR_ARG, "n_draws must be in " + std::to_string(PV_DRAWS_MIN) + " .. " + std::to_string(PV_DRAWS_MAX));
    return 0;
}
// erm_get_* (H = erm_handle) and erm_farm_get_* (H = erm_farm_handle) of the six passes: the checks, the source, the product
template <typename H> static int get_marginal_waic(H h, int32_t n_nodes, double* out10, double* lppd_u, double* p_u, int family = FAMILY_GAUSSIAN)
{
    int Q = 0;
    ItemSource S;
    if (int rc = item_entry_args(out10, n_nodes, &Q)) return rc;
    if (int rc = item_source(h, PASS_WAIC, S, family)) return rc;
    return item_waic(S, Q, nullptr, out10, lppd_u, p_u);
}
template <typename H> static int get_marginal_loo(H h, int32_t n_nodes, double* out12, double* pw, int family = FAMILY_GAUSSIAN)
{
    int Q = 0;
    ItemSource S;
    if (int rc = item_entry_args(out12, n_nodes, &Q)) return rc;
    if (int rc = item_source(h, PASS_LOO, S, family)) return rc;
    return item_loo(S, Q, out12, pw);
}
template <typename H> static int get_scores(H h, int32_t n_nodes, double* score, double* out4)
{
    int Q = 0;
    ItemSource S;
    if (int rc = item_entry_args(score, n_nodes, &Q)) return rc;
    if (int rc = item_source(h, PASS_SCORES, S)) return rc;
    return item_scores(S, Q, SCORE_EQUAL, score, out4);
}
template <typename H> static int get_person_fit(H h, int32_t n_nodes, double* fit, double* out4)
{
    int Q = 0;
    ItemSource S;
    if (int rc = item_entry_args(fit, n_nodes, &Q)) return rc;
    if (int rc = item_source(h, PASS_FIT, S)) return rc;
    return item_fit(S, Q, SCORE_EQUAL, fit, out4);
}
template <typename H> static int get_item_fit(H h, int32_t n_nodes, double* fit, double* out4)
{
    int Q = 0;
    ItemSource S;
    if (int rc = item_entry_args(fit, n_nodes, &Q)) return rc;
    if (int rc = item_source(h, PASS_ITEM_FIT, S)) return rc;
    return item_itemfit(S, Q, fit, out4);
}
template <typename H> static int get_plausible_values(H h,int32_t n_nodes, int32_t n_draws, uint64_t seed, double* pv, int32_t* node, int32_t* coarse, double* out4)
{
    int Q = 0;
    ItemSource S;
    if (int rc = pv_entry_args(n_nodes, n_draws, pv, &Q)) return rc;
    if (int rc = item_source(h, PASS_PV, S)) return rc;
    return item_pv(S, Q, n_draws, seed, pv, node, coarse, out4);
}
// The caller-data entries of a pass, erm_X and erm_X_masked, are ONE body: the model, the node count, the pass's own checks, the source, the product.  what names
// the entry in the allocation messages; obs may be NULL (complete data), and n_obs (may be NULL) is then n_item for every subject once the pass has succeeded.
static int obs_all(int rc, const CallerData& d, const uint8_t* obs, int32_t* n_obs)
{
    if (rc == 0 && !obs && n_obs) for (int64_t i = 0; i < d.n_subj; ++i) n_obs[i] = d.n_item;
    return rc;
}
static int caller_marginal_loglik(const CallerData& d, const char* what, const uint8_t* obs, int32_t* n_obs, int32_t n_nodes, double* l, double* out10, double* lppd_u, double* p_u,
                                  int family = FAMILY_GAUSSIAN, double q_rt = 0.0)
{
    if (int rc = marg_refuse_model(d.model, family)) return rc;
    int Q = 0;
    if (int rc = marg_nodes(n_nodes, &Q)) return rc;
    ItemSource S;
    if (int rc = item_source(what, d, out10 || lppd_u || p_u ? 2 : 1, "n_rows must be at least 1 (at least 2 for the WAIC outputs)", S, family, q_rt, obs, n_obs)) return rc;
    return obs_all(item_waic(S, Q, l, out10, lppd_u, p_u), d, obs, n_obs);
}
// (the scores' and the person fit's: product is item_scores or item_fit)
template <typename Product>
static int caller_subject_table(const CallerData& d, const char* what, const uint8_t* obs, int32_t* n_obs, int32_t n_nodes, int32_t weighting, double* table, double* out4, Product&& product)
{
    if (int rc = marg_refuse_model(d.model)) return rc;
    int Q = 0;
    if (int rc = marg_nodes(n_nodes, &Q)) return rc;
    if (!score_weighting_ok(weighting)) return fail(ERM_ERR_ARG, "weighting must be ERM_SCORE_EQUAL or ERM_SCORE_LIKELIHOOD");
    if (!table) return fail(ERM_ERR_ARG, "out is NULL");
    ItemSource S;
    if (int rc = item_source(what, d, 1, "n_rows must be at least 1", S, FAMILY_GAUSSIAN, 0.0, obs, n_obs)) return rc;
    return obs_all(product(S, Q, weighting, table, out4), d, obs, n_obs);
}
static int caller_plausible_values(const CallerData& d, const char* what, const uint8_t* obs, int32_t* n_obs, int32_t n_nodes, int32_t n_draws, uint64_t seed, double* pv, int32_t* node,
                                   int32_t* coarse, double* out4)
{
    if (int rc = marg_refuse_model(d.model)) return rc;
    int Q = 0;
    if (int rc = pv_entry_args(n_nodes, n_draws, pv, &Q)) return rc;
    ItemSource S;
    if (int rc = item_source(what, d, 1, "n_rows must be at least 1", S, FAMILY_GAUSSIAN, 0.0, obs, n_obs)) return rc;
    return obs_all(item_pv(S, Q, n_draws, seed, pv, node, coarse, out4), d, obs, n_obs);
}
}  // namespace

extern "C" {

int erm_create(const erm_config* cfg, erm_handle* out)
{
    if (!cfg || !out) return fail(ERM_ERR_ARG, "cfg/out is NULL");
    *out = nullptr;
    std::unique_ptr<EngineBase> e;
    if (cfg->precision == ERM_PREC_F32) e.reset(new Engine<float>());
    else if (cfg->precision == ERM_PREC_F64) e.reset(new Engine<double>());
    else return fail(ERM_ERR_ARG, "unknown precision");
    e->cfg = *cfg;
    if (int rc = e->init()) return rc;
    *out = new erm_engine{std::move(e)};
    return ERM_OK;
}
void erm_destroy(erm_handle h) { delete h; }
#define CHK_H if (!h) return fail(ERM_ERR_ARG, "handle is NULL")
int erm_set_data(erm_handle h, const uint8_t* Y, const double* logT, const double* X) { CHK_H; return h->e->set_data(Y, logT, X); }
int erm_set_state(erm_handle h, const erm_state* st) { CHK_H; return h->e->set_state(st); }
int erm_get_state(erm_handle h, erm_state* st) { CHK_H; return h->e->get_state(st); }
int erm_run(erm_handle h, int64_t nsweeps) { CHK_H; return h->e->run(nsweeps); }
int64_t erm_rows_done(erm_handle h) { return h ? h->e->rows_done : -1; }
int erm_reset_trace(erm_handle h) { CHK_H; return h->e->reset_trace(); }
int64_t erm_trace_width(erm_handle h, int which) { return h ? h->e->trace_width(which) : -1; }
int erm_get_trace(erm_handle h, int which, double* out) { CHK_H; if (!out) return fail(ERM_ERR_ARG, "out is NULL"); return h->e->get_trace(which, out); }
int64_t erm_item_trace_width(erm_handle h) { return h ? h->e->item_trace_width() : -1; }
int erm_get_item_trace(erm_handle h, double* out) { CHK_H; if (!out) return fail(ERM_ERR_ARG, "out is NULL"); return h->e->get_item_trace(out); }
int erm_get_mean(erm_handle h, erm_state* out) { CHK_H; return h->e->get_mean(out); }
int64_t erm_post_count(erm_handle h) { return h ? h->e->post_rows : -1; }
int erm_simulate_data(erm_handle h, const erm_state* truth, uint64_t seed, int noise) { CHK_H; return h->e->simulate_data(truth, seed, noise); }
int erm_get_data(erm_handle h, uint8_t* Y, double* logT, double* X) { CHK_H; return h->e->get_data(Y, logT, X); }
int erm_get_truth(erm_handle h, double* theta, double* zeta) { CHK_H; return h->e->get_truth(theta, zeta); }
// the convergence diagnostics (diag_query, erm_diagnostics.hpp): the basic entries require both vectors, the rank entries skip a NULL one
int erm_get_diagnostics(erm_handle h, int which, double* ess, double* rhat) { CHK_H; if (!ess || !rhat) return fail(ERM_ERR_ARG, "out is NULL"); double* v[3] = { ess, rhat, nullptr }; return diag_query(h, which, false, v, nullptr); }
int erm_get_convergence(erm_handle h, int which, int64_t* counts4) { CHK_H; if (!counts4) return fail(ERM_ERR_ARG, "out is NULL"); return diag_query(h, which, false, nullptr, counts4); }
int erm_get_rank_diagnostics(erm_handle h, int which, double* ess_bulk, double* ess_tail, double* rhat_rank) { CHK_H; double* v[3] = { ess_bulk, ess_tail, rhat_rank }; return diag_query(h, which, true, v, nullptr); }
int erm_get_rank_convergence(erm_handle h, int which, int64_t* counts6) { CHK_H; if (!counts6) return fail(ERM_ERR_ARG, "out is NULL"); return diag_query(h, which, true, nullptr, counts6); }
int erm_get_dic(erm_handle h, double* out4) { CHK_H; if (!out4) return fail(ERM_ERR_ARG, "out is NULL"); return h->e->get_dic(out4); }
int erm_set_pointwise(erm_handle h, int unit) { CHK_H; return h->e->set_pointwise(unit); }
int erm_get_waic(erm_handle h, double* out_eight) { CHK_H; if (!out_eight) return fail(ERM_ERR_ARG, "out is NULL"); return h->e->get_waic(out_eight); }
int64_t erm_pointwise_units(erm_handle h) { return h ? h->e->pointwise_units() : -1; }
int erm_get_pointwise(erm_handle h, double* lppd_u, double* p_u) { CHK_H; return h->e->get_pointwise(lppd_u, p_u); }
int erm_get_marginal_waic(erm_handle h, int32_t n_nodes, double* out10, double* lppd_u, double* p_u) { CHK_H; return get_marginal_waic(h, n_nodes, out10, lppd_u, p_u); }
int erm_get_marginal_loo(erm_handle h, int32_t n_nodes, double* out12, double* pw) { CHK_H; return get_marginal_loo(h, n_nodes, out12, pw); }
int erm_get_quantile_marginal_waic(erm_handle h, int32_t n_nodes, double* out10, double* lppd_u, double* p_u) { CHK_H; return get_marginal_waic(h, n_nodes, out10, lppd_u, p_u, FAMILY_QUANTILE); }
int erm_get_quantile_marginal_loo(erm_handle h, int32_t n_nodes, double* out12, double* pw) { CHK_H; return get_marginal_loo(h, n_nodes, out12, pw, FAMILY_QUANTILE); }
int erm_get_scores(erm_handle h, int32_t n_nodes, double* score, double* out4) { CHK_H; return get_scores(h, n_nodes, score, out4); }
int erm_get_person_fit(erm_handle h, int32_t n_nodes, double* fit, double* out4) { CHK_H; return get_person_fit(h, n_nodes, fit, out4); }
int erm_get_item_fit(erm_handle h, int32_t n_nodes, double* fit, double* out4) { CHK_H; return get_item_fit(h, n_nodes, fit, out4); }
int erm_get_plausible_values(erm_handle h, int32_t n_nodes, int32_t n_draws, uint64_t seed, double* pv, int32_t* node, int32_t* coarse, double* out4)
{
    CHK_H;
    return get_plausible_values(h, n_nodes, n_draws, seed, pv, node, coarse, out4);
}
int erm_set_predictive(erm_handle h, int on, int32_t thin) { CHK_H; return h->e->set_predictive(on, thin); }
int64_t erm_predictive_reps(erm_handle h) { return h ? h->e->predictive_reps() : -1; }
int erm_get_predictive(erm_handle h, double* item, double* subj, double* total) { CHK_H; return h->e->get_predictive(item, subj, total); }
int erm_set_seed(erm_handle h, uint64_t seed) { CHK_H; return h->e->set_seed(seed); }
int erm_get_timing(erm_handle h, erm_timing* out) { CHK_H; if (!out) return fail(ERM_ERR_ARG, "out is NULL"); *out = h->e->timing; return 0; }
int erm_set_shard(erm_handle h, int rank, int count, int64_t n_subj_total, int64_t row_base, erm_exchange_fn exchange, void* user)
{
    CHK_H;
    if (!exchange) return fail(ERM_ERR_ARG, "exchange callback is NULL");
    return h->e->set_shard(rank, count, n_subj_total, row_base, exchange, user, nullptr);
}
int erm_rccl_unique_id(void* out128)
{
    if (!out128) return fail(ERM_ERR_ARG, "out is NULL");
    if (int rc = g_rccl.load()) return rc;
    ncclUniqueId id;
    RCCLCHK(g_rccl.GetUniqueId(&id));
    std::memcpy(out128, &id, sizeof(id));
    return 0;
}
int erm_set_shard_rccl(erm_handle h, int rank, int count, int64_t n_subj_total, int64_t row_base, const void* unique_id128)
{
    CHK_H;
    if (!unique_id128) return fail(ERM_ERR_ARG, "unique id is NULL");
    return h->e->set_shard(rank, count, n_subj_total, row_base, nullptr, nullptr, unique_id128);
}
int erm_copy(void* dst, const void* src, size_t bytes)
{
    if (bytes == 0) return 0;
    if (!dst || !src) return fail(ERM_ERR_ARG, "dst/src is NULL");
    HIPCHK(hipMemcpy(dst, src, bytes, hipMemcpyDefault));
    return 0;
}

/* ---- chain farm ---- */
int erm_farm_create(const erm_config* cfg, const int32_t* devices, int32_t n_chains, erm_farm_handle* out)
{
    if (!cfg || !out || !devices) return fail(ERM_ERR_ARG, "cfg/devices/out is NULL");
    *out = nullptr;
    if (n_chains < 1 || n_chains > 255) return fail(ERM_ERR_ARG, "n_chains must be in [1, 255]");
    int ndev = 0;
    HIPCHK(hipGetDeviceCount(&ndev));
    std::unique_ptr<erm_farm> f(new erm_farm());
    f->cfg = *cfg;
    for (int l = 0; l < n_chains; ++l) {
        if (devices[l] < 0 || devices[l] >= ndev) return fail(ERM_ERR_ARG, "chain " + std::to_string(l) + ": no such device " + std::to_string(devices[l]));
        erm_config c = *cfg;
        c.device = devices[l]; c.chain_id = l; c.n_chain = 1;      // every chain records n_iter rows of its own
        erm_handle h = nullptr;
        if (int rc = erm_create(&c, &h)) return fail(rc, "chain " + std::to_string(l) + ": " + g_err);
        f->eng.emplace_back(h);
        f->dev.push_back(devices[l]);
        bool seen = false;
        for (int d : f->udev) seen = seen || d == devices[l];
        if (!seen) f->udev.push_back(devices[l]);
    }
    *out = f.release();
    return ERM_OK;
}
void erm_farm_destroy(erm_farm_handle f) { delete f; }
#define CHK_F if (!f) return fail(ERM_ERR_ARG, "farm handle is NULL")
int32_t erm_farm_chains(erm_farm_handle f) { return f ? (int32_t)f->eng.size() : -1; }
erm_handle erm_farm_engine(erm_farm_handle f, int32_t chain) { return (f && chain >= 0 && chain < (int32_t)f->eng.size()) ? f->eng[chain].get() : nullptr; }
int erm_farm_set_data(erm_farm_handle f, const uint8_t* Y, const double* logT, const double* X)
{
    CHK_F;
    return f->parallel([&](int l) { return f->eng[l]->e->set_data(Y, logT, X); });
}
int erm_farm_set_state(erm_farm_handle f, int32_t chain, const erm_state* st)
{
    CHK_F;
    if (chain < 0 || chain >= (int32_t)f->eng.size()) return fail(ERM_ERR_ARG, "no such chain");
    return f->eng[chain]->e->set_state(st);
}
int erm_farm_get_state(erm_farm_handle f, int32_t chain, erm_state* st)
{
    CHK_F;
    if (chain < 0 || chain >= (int32_t)f->eng.size()) return fail(ERM_ERR_ARG, "no such chain");
    return f->eng[chain]->e->get_state(st);
}
int erm_farm_run(erm_farm_handle f, int64_t nsweeps)
{
    CHK_F;
    const auto t0 = std::chrono::steady_clock::now();
    const int rc = f->parallel([&](int l) { return f->eng[l]->e->run(nsweeps); });
    f->tm.run_wall_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return rc;
}
int erm_farm_get_timing(erm_farm_handle f, erm_farm_timing* out, double* run_ms)
{
    CHK_F;
    if (!out) return fail(ERM_ERR_ARG, "out is NULL");
    *out = f->tm;
    out->n_devices = (int32_t)f->udev.size();
    out->rccl_ranks = 0;
    if (!f->comms.empty() && f->comms[0]) { int n = 0; RCCLCHK(g_rccl.CommCount(f->comms[0], &n)); out->rccl_ranks = n; }
    if (run_ms) for (size_t l = 0; l < f->eng.size(); ++l) run_ms[l] = f->eng[l]->e->timing.run_ms;
    return 0;
}
int erm_farm_reset_trace(erm_farm_handle f)
{
    CHK_F;
    for (auto& e : f->eng) if (int rc = e->e->reset_trace()) return rc;
    return 0;
}
int64_t erm_farm_post_count(erm_farm_handle f)
{
    if (!f) return -1;
    int64_t n = 0;
    for (auto& e : f->eng) n += e->e->post_rows;
    return n;
}
int erm_farm_used_rccl(erm_farm_handle f) { return f ? (f->used_rccl ? 1 : 0) : -1; }
int erm_farm_get_trace(erm_farm_handle f, int which, double* out)
{
    CHK_F;
    if (!out) return fail(ERM_ERR_ARG, "out is NULL");
    // Julia layout [nIter][width][nChain], nIter fastest: chain l's (nIter x width x 1) block is contiguous at offset l * nIter * width
    const int64_t wd = f->eng[0]->e->trace_width(which);
    if (wd <= 0) return fail(ERM_ERR_ARG, "this model has no such trace");
    const int64_t blk = (int64_t)f->cfg.n_iter * wd;
    return f->parallel([&](int l) { return f->eng[l]->e->get_trace(which, out + (size_t)l * blk); });
}
// The farm's one collective: every chain's post-burn-in sums added into its device's accumulator (chains that share a device add in chain order), the
// devices' vectors summed by ONE ncclAllReduce (RCCL over xGMI), each rank on a stream of its own.  Leaves the total on every device (acc[d]) and returns the
// number of post-burn-in rows.  ERM_FLAG_FARM_FORCE_RCCL takes the RCCL path with a one-device communicator too (tests).
static int farm_reduce(erm_farm_handle f, std::vector<DevBuf>& acc, int64_t* total_out, double* init_ms_out)
{
    const int64_t total = erm_farm_post_count(f);
    if (total <= 0) return fail(ERM_ERR_STATE, "no post-burn-in sweeps recorded");
    const int64_t len = f->eng[0]->e->summary_len();
    const int nd = (int)f->udev.size();
    acc.clear(); acc.resize(nd);
    for (int d = 0; d < nd; ++d) {
        HIPCHK(hipSetDevice(f->udev[d]));
        if (int rc = acc[d].alloc((size_t)len * sizeof(double))) return rc;      // zeroed, complete on return
    }
    for (size_t l = 0; l < f->eng.size(); ++l) {
        int d = 0;
        while (f->udev[d] != f->dev[l]) ++d;
        if (int rc = f->eng[l]->e->summary_add(acc[d].as<double>(), nullptr)) return fail(rc, "chain " + std::to_string(l) + ": " + g_err);      // synchronises its stream
    }
    const bool force = (f->cfg.flags & ERM_FLAG_FARM_FORCE_RCCL) != 0;
    f->used_rccl = false;
    f->tm.allreduce_ms = 0.0;
    *init_ms_out = 0.0;                       // communicator creation inside THIS call (first reduction only): reported apart from gather_ms
    if (nd > 1 || force) {
        if (int rc = g_rccl.load()) return rc;
        if (f->rstream.empty()) {
            f->rstream.assign(nd, nullptr);
            for (int d = 0; d < nd; ++d) { HIPCHK(hipSetDevice(f->udev[d])); HIPCHK(hipStreamCreateWithFlags(&f->rstream[d], hipStreamNonBlocking)); }
        }
        if (f->comms.empty()) {
            const auto c0 = std::chrono::steady_clock::now();
            f->comms.assign(nd, nullptr);
            const ncclResult_t r = g_rccl.CommInitAll(f->comms.data(), nd, f->udev.data());
            if (r != ncclSuccess) { f->comms.clear(); return fail(ERM_ERR_STATE, std::string("ncclCommInitAll: ") + g_rccl.GetErrorString(r)); }
            f->tm.comm_init_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - c0).count();
            *init_ms_out = f->tm.comm_init_ms;
        }
        const auto a0 = std::chrono::steady_clock::now();
        // a group that has been started is always ended, whatever happens inside it
        ncclResult_t r = g_rccl.GroupStart();
        if (r != ncclSuccess) return fail(ERM_ERR_STATE, std::string("ncclGroupStart: ") + g_rccl.GetErrorString(r));
        std::string what;
        for (int d = 0; d < nd && r == ncclSuccess; ++d) {
            if (hipSetDevice(f->udev[d]) != hipSuccess) { what = "hipSetDevice"; r = ncclUnhandledCudaError; break; }
            r = g_rccl.AllReduce(acc[d].p, acc[d].p, (size_t)len, ncclDouble, ncclSum, f->comms[d], f->rstream[d]);
            if (r != ncclSuccess) what = "ncclAllReduce";
        }
        const ncclResult_t re = g_rccl.GroupEnd();
        if (r != ncclSuccess) return fail(ERM_ERR_STATE, what + ": " + g_rccl.GetErrorString(r));
        if (re != ncclSuccess) return fail(ERM_ERR_STATE, std::string("ncclGroupEnd: ") + g_rccl.GetErrorString(re));
        for (int d = 0; d < nd; ++d) { HIPCHK(hipSetDevice(f->udev[d])); HIPCHK(hipStreamSynchronize(f->rstream[d])); }
        f->tm.allreduce_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - a0).count();
        f->used_rccl = true;
    }
    *total_out = total;
    return 0;
}
int erm_farm_get_mean(erm_farm_handle f, erm_state* out)
{
    CHK_F;
    if (!out) return fail(ERM_ERR_ARG, "state is NULL");
    const auto t0 = std::chrono::steady_clock::now();
    std::vector<DevBuf> acc;
    int64_t total = 0;
    double init_ms = 0.0;
    if (int rc = farm_reduce(f, acc, &total, &init_ms)) return rc;
    const int rc = f->eng[0]->e->mean_from_summary(acc[0].as<double>(), 1.0 / (double)total, out);      // (chain 0 runs on the first distinct device)
    f->tm.gather_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count() - init_ms;
    return rc;
}
// getDic of the farm: Dbar over the logLike rows of ALL chains, Dhat at the joint Post.mean -- the vector erm_farm_get_mean reduces, evaluated where it lies
// (the first chain's device and data copy; every chain holds the same data set); only the four numbers cross the boundary
int erm_farm_get_dic(erm_farm_handle f, double* out4)
{
    CHK_F;
    if (!out4) return fail(ERM_ERR_ARG, "out is NULL");
    std::vector<DevBuf> acc;
    int64_t total = 0;
    double init_ms = 0.0;
    if (int rc = farm_reduce(f, acc, &total, &init_ms)) return rc;
    int d0 = 0;
    while (f->udev[d0] != f->dev[0]) ++d0;
    std::vector<EngineBase*> chains;
    for (auto& e : f->eng) chains.push_back(e->e.get());
    return dic_from_summary(chains.data(), chains.size(), acc[d0].as<double>(), total, out4);
}
// the farm's passes over the item trace: the engine's, over the post-burn-in rows of all chains as one table on chain 0's device (erm_item_pass.hpp)
int erm_farm_get_marginal_waic(erm_farm_handle f, int32_t n_nodes, double* out10, double* lppd_u, double* p_u) { CHK_F; return get_marginal_waic(f, n_nodes, out10, lppd_u, p_u); }
int erm_farm_get_marginal_loo(erm_farm_handle f, int32_t n_nodes, double* out12, double* pw) { CHK_F; return get_marginal_loo(f, n_nodes, out12, pw); }
int erm_farm_get_quantile_marginal_waic(erm_farm_handle f, int32_t n_nodes, double* out10, double* lppd_u, double* p_u) { CHK_F; return get_marginal_waic(f, n_nodes, out10, lppd_u, p_u, FAMILY_QUANTILE); }
int erm_farm_get_quantile_marginal_loo(erm_farm_handle f, int32_t n_nodes, double* out12, double* pw) { CHK_F; return get_marginal_loo(f, n_nodes, out12, pw, FAMILY_QUANTILE); }
int erm_farm_get_scores(erm_farm_handle f, int32_t n_nodes, double* score, double* out4) { CHK_F; return get_scores(f, n_nodes, score, out4); }
int erm_farm_get_person_fit(erm_farm_handle f, int32_t n_nodes, double* fit, double* out4) { CHK_F; return get_person_fit(f, n_nodes, fit, out4); }
int erm_farm_get_item_fit(erm_farm_handle f, int32_t n_nodes, double* fit, double* out4) { CHK_F; return get_item_fit(f, n_nodes, fit, out4); }
int erm_farm_get_plausible_values(erm_farm_handle f, int32_t n_nodes, int32_t n_draws, uint64_t seed, double* pv, int32_t* node, int32_t* coarse, double* out4)
{
    CHK_F;
    return get_plausible_values(f, n_nodes, n_draws, seed, pv, node, coarse, out4);
}
int erm_farm_set_seed(erm_farm_handle f, uint64_t seed)
{
    CHK_F;
    for (auto& e : f->eng) if (int rc = e->e->set_seed(seed)) return rc;
    return 0;
}
// the farm's joint diagnostics, over its chains as over an engine's interleaved ones (diag_query): NULL outputs as the engine entries treat them
int erm_farm_get_diagnostics(erm_farm_handle f, int which, double* ess, double* rhat) { CHK_F; if (!ess || !rhat) return fail(ERM_ERR_ARG, "out is NULL"); double* v[3] = { ess, rhat, nullptr }; return diag_query(f, which, false, v, nullptr); }
int erm_farm_get_convergence(erm_farm_handle f, int which, int64_t* counts4) { CHK_F; if (!counts4) return fail(ERM_ERR_ARG, "out is NULL"); return diag_query(f, which, false, nullptr, counts4); }
int erm_farm_get_rank_diagnostics(erm_farm_handle f, int which, double* ess_bulk, double* ess_tail, double* rhat_rank) { CHK_F; double* v[3] = { ess_bulk, ess_tail, rhat_rank }; return diag_query(f, which, true, v, nullptr); }
int erm_farm_get_rank_convergence(erm_farm_handle f, int which, int64_t* counts6) { CHK_F; if (!counts6) return fail(ERM_ERR_ARG, "out is NULL"); return diag_query(f, which, true, nullptr, counts6); }

const char* erm_last_error(void) { return g_err.c_str(); }
const char* erm_version(void) { return "ertirt-amd 0.4.0 (gfx950)"; }
int erm_abi_version(void) { return ERM_ABI_VERSION; }

// ---- the passes on caller-supplied data and rows (the bodies: caller_* above).  An entry with an observed mask given obs == NULL is its complete
// sibling, by that name in the allocation messages too.
int erm_marginal_loglik(int device, int model, int64_t n_subj, int32_t n_item, int32_t n_feat, const uint8_t* Y, const double* logT, const double* X, const double* rows,
                        int64_t n_rows, int32_t n_nodes, double* l, double* out10, double* lppd_u, double* p_u)
{
    return caller_marginal_loglik({device, model, n_subj, n_item, n_feat, Y, logT, X, rows, n_rows}, "erm_marginal_loglik's inputs", nullptr, nullptr, n_nodes, l, out10, lppd_u, p_u);
}
int erm_marginal_loglik_masked(int device, int model, int64_t n_subj, int32_t n_item, int32_t n_feat, const uint8_t* Y, const double* logT, const double* X, const uint8_t* obs,
                               const double* rows, int64_t n_rows, int32_t n_nodes, double* l, double* out10, double* lppd_u, double* p_u, int32_t* n_obs)
{
    return caller_marginal_loglik({device, model, n_subj, n_item, n_feat, Y, logT, X, rows, n_rows},
                                  obs ? "erm_marginal_loglik_masked's inputs" : "erm_marginal_loglik's inputs", obs, n_obs, n_nodes, l, out10, lppd_u, p_u);
}
// LatentQr's: the same body with the quantile family's checks and the caller's q_rt
int erm_quantile_marginal_loglik(int device, int model, int64_t n_subj, int32_t n_item, int32_t n_feat, const uint8_t* Y, const double* logT, const double* X, const double* rows,
                                 int64_t n_rows, double q_rt, int32_t n_nodes, double* l, double* out10, double* lppd_u, double* p_u)
{
    return caller_marginal_loglik({device, model, n_subj, n_item, n_feat, Y, logT, X, rows, n_rows},
                                  "erm_quantile_marginal_loglik's inputs", nullptr, nullptr, n_nodes, l, out10, lppd_u, p_u, FAMILY_QUANTILE, q_rt);
}

int erm_psis_loo(int device, const double* l, int64_t n_subj, int64_t n_rows, double* out12, double* pw, double* lw)
{
    if (!l || !out12) return fail(ERM_ERR_ARG, "l / out is NULL");
    if (n_subj <= 0 || n_subj >= (1LL << 32)) return fail(ERM_ERR_ARG, "n_subj out of range");
    if (int rc = psis_rows_ok(n_rows)) return rc;
    const int64_t N = n_subj, S = n_rows;
    for (size_t e = 0; e < (size_t)N * S; ++e) if (!std::isfinite(l[e])) return fail(ERM_ERR_NONFINITE, "NaN or Inf in l (unit " + std::to_string(e % (size_t)N) + ", row " + std::to_string(e / (size_t)N) + ")");
    HIPCHK(hipSetDevice(device));
    auto fill = [&](int64_t c0, int64_t nc, double* dst) -> int {
        HIPCHK(hipMemcpy2D(dst, (size_t)nc * sizeof(double), l + c0, (size_t)N * sizeof(double), (size_t)nc * sizeof(double), (size_t)S, hipMemcpyHostToDevice));
        return 0;
    };
    auto take = [&](int64_t c0, int64_t nc, const double* src) -> int {
        HIPCHK(hipMemcpy2D(lw + c0, (size_t)N * sizeof(double), src, (size_t)nc * sizeof(double), (size_t)nc * sizeof(double), (size_t)S, hipMemcpyDeviceToHost));
        return 0;
    };
    double s8[8];
    if (int rc = psis_run(N, S, nullptr, fill, take, lw != nullptr, s8, pw)) return rc;
    psis_out12(s8, N, S, 0, 0, out12);
    return 0;
}

int erm_score(int device, int model, int64_t n_subj, int32_t n_item, int32_t n_feat, const uint8_t* Y, const double* logT, const double* X, const double* rows,
              int64_t n_rows, int32_t n_nodes, int32_t weighting, double* score, double* out4)
{
    return caller_subject_table({device, model, n_subj, n_item, n_feat, Y, logT, X, rows, n_rows}, "erm_score's inputs", nullptr, nullptr, n_nodes, weighting, score, out4, item_scores);
}
int erm_score_masked(int device, int model, int64_t n_subj, int32_t n_item, int32_t n_feat, const uint8_t* Y, const double* logT, const double* X, const uint8_t* obs,
                     const double* rows, int64_t n_rows, int32_t n_nodes, int32_t weighting, double* score, double* out4, int32_t* n_obs)
{
    return caller_subject_table({device, model, n_subj, n_item, n_feat, Y, logT, X, rows, n_rows},
                                obs ? "erm_score_masked's inputs" : "erm_score's inputs", obs, n_obs, n_nodes, weighting, score, out4, item_scores);
}

int erm_plausible_values(int device, int model, int64_t n_subj, int32_t n_item, int32_t n_feat, const uint8_t* Y, const double* logT, const double* X, const double* rows,
                         int64_t n_rows, int32_t n_nodes, int32_t n_draws, uint64_t seed, double* pv, int32_t* node, int32_t* coarse, double* out4)
{
    return caller_plausible_values({device, model, n_subj, n_item, n_feat, Y, logT, X, rows, n_rows}, "erm_plausible_values' inputs", nullptr, nullptr, n_nodes, n_draws, seed, pv, node, coarse, out4);
}
int erm_plausible_values_masked(int device, int model, int64_t n_subj, int32_t n_item, int32_t n_feat, const uint8_t* Y, const double* logT, const double* X, const uint8_t* obs,
                                const double* rows, int64_t n_rows, int32_t n_nodes, int32_t n_draws, uint64_t seed, double* pv, int32_t* node, int32_t* coarse, double* out4,
                                int32_t* n_obs)
{
    return caller_plausible_values({device, model, n_subj, n_item, n_feat, Y, logT, X, rows, n_rows},
                                   obs ? "erm_plausible_values_masked's inputs" : "erm_plausible_values' inputs", obs, n_obs, n_nodes, n_draws, seed, pv, node, coarse, out4);
}

// person fit
int erm_person_fit(int device, int model, int64_t n_subj, int32_t n_item, int32_t n_feat, const uint8_t* Y, const double* logT, const double* X, const double* rows,
                   int64_t n_rows, int32_t n_nodes, int32_t weighting, double* fit, double* out4)
{
    return caller_subject_table({device, model, n_subj, n_item, n_feat, Y, logT, X, rows, n_rows}, "erm_person_fit's inputs", nullptr, nullptr, n_nodes, weighting, fit, out4, item_fit);
}
int erm_person_fit_masked(int device, int model, int64_t n_subj, int32_t n_item, int32_t n_feat, const uint8_t* Y, const double* logT, const double* X, const uint8_t* obs,
                          const double* rows, int64_t n_rows, int32_t n_nodes, int32_t weighting, double* fit, double* out4, int32_t* n_obs)
{
    return caller_subject_table({device, model, n_subj, n_item, n_feat, Y, logT, X, rows, n_rows},
                                obs ? "erm_person_fit_masked's inputs" : "erm_person_fit's inputs", obs, n_obs, n_nodes, weighting, fit, out4, item_fit);
}

// item fit: one entry, obs may be NULL (complete data: the unmasked kernel); it reports no n_obs
int erm_item_fit(int device, int model, int64_t n_subj, int32_t n_item, int32_t n_feat, const uint8_t* Y, const double* logT, const double* X, const uint8_t* obs,
                 const double* rows, int64_t n_rows, int32_t n_nodes, double* fit, double* out4)
{
    if (int rc = marg_refuse_model(model)) return rc;
    int Q = 0;
    if (int rc = marg_nodes(n_nodes, &Q)) return rc;
    if (!fit) return fail(ERM_ERR_ARG, "out is NULL");
    ItemSource S;
    if (int rc = item_source("erm_item_fit's inputs", {device, model, n_subj, n_item, n_feat, Y, logT, X, rows, n_rows},
                                                      1, "n_rows must be at least 1", S, FAMILY_GAUSSIAN, 0.0, obs, nullptr)) return rc;
    return item_itemfit(S, Q, fit, out4);
}

int erm_debug_invwishart(int device, uint64_t seed, uint32_t sweep, int64_t n, double nu, const double* psi4, double* out)
{
    if (n <= 0 || !out || !psi4) return fail(ERM_ERR_ARG, "bad n / psi / out");
    if (!(nu > 1.0) || !(psi4[0] > 0.0) || !(psi4[0] * psi4[3] - psi4[1] * psi4[2] > 0.0)) return fail(ERM_ERR_ARG, "InverseWishart(nu, Psi) needs nu > 1 and a positive definite Psi");
    HIPCHK(hipSetDevice(device));
    DevBuf dout;
    if (int rc = dout.alloc((size_t)n * 4 * sizeof(double))) return rc;
    hipLaunchKernelGGL(invwishart_batch_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, seed, sweep, (long long)n, nu, psi4[0], psi4[1], psi4[2], psi4[3], dout.as<double>());
    HIPCHK(hipGetLastError());
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(out, dout.p, (size_t)n * 4 * sizeof(double), hipMemcpyDeviceToHost));
    return 0;
}

int erm_debug_convergence(int device, int64_t n, const double* ess, const double* rhat, int64_t* counts4)
{
    if (n <= 0 || !ess || !rhat || !counts4) return fail(ERM_ERR_ARG, "bad n / ess / rhat / out");
    HIPCHK(hipSetDevice(device));
    DevBuf dE, dR;
    if (int rc = dE.alloc((size_t)n * sizeof(double))) return rc;
    if (int rc = dR.alloc((size_t)n * sizeof(double))) return rc;
    H2D(dE.p, ess, (size_t)n * sizeof(double));
    H2D(dR.p, rhat, (size_t)n * sizeof(double));
    return count_converged(dE, dR, n, nullptr, counts4);
}

int erm_debug_rank_diagnostics(int device, int precision, const double* x, int64_t n_draw, int64_t n_col, int32_t n_chain, double* ess_bulk, double* ess_tail, double* rhat_rank)
{
    double* v[3] = { ess_bulk, ess_tail, rhat_rank };
    return debug_query(device, precision, x, n_draw, n_col, n_chain, true, v);
}

int erm_debug_diagnostics(int device, int precision, const double* x, int64_t n_draw, int64_t n_col, int32_t n_chain, double* ess, double* rhat)
{
    if (!ess || !rhat) return fail(ERM_ERR_ARG, "out is NULL");
    double* v[3] = { ess, rhat, nullptr };
    return debug_query(device, precision, x, n_draw, n_col, n_chain, false, v);
}

int erm_debug_sample(int device, int precision, int which, uint64_t seed, uint32_t site, uint32_t sweep, int64_t n,
                     const double* par0, const double* par1, double* out)
{
    if (n <= 0 || !out) return fail(ERM_ERR_ARG, "bad n/out");
    HIPCHK(hipSetDevice(device));
    DevBuf d0, d1, dout;
    if (int rc = dout.alloc(n * sizeof(double))) return rc;
    if (par0) { if (int rc = d0.alloc(n * sizeof(double))) return rc; H2D(d0.p, par0, n * sizeof(double)); }
    if (par1) { if (int rc = d1.alloc(n * sizeof(double))) return rc; H2D(d1.p, par1, n * sizeof(double)); }
    DevBuf dtab;
    {
        std::vector<double> tab((size_t)PG_NBIN * 4);
        for (int k = 0; k < PG_NBIN; ++k) pg_bin(k, &tab[(size_t)4 * k]);
        if (int rc = dtab.alloc(tab.size() * sizeof(double))) return rc;
        H2D(dtab.p, tab.data(), tab.size() * sizeof(double));
    }
    const int bt = 256; const int gb = (int)((n + bt - 1) / bt);
    if (precision == ERM_PREC_F32)
        hipLaunchKernelGGL((sample_batch_kernel<float>), dim3(gb), dim3(bt), 0, 0, which, seed, site, sweep, (long long)n, d0.as<double>(), d1.as<double>(), dout.as<double>(), dtab.as<double>());
    else
        hipLaunchKernelGGL((sample_batch_kernel<double>), dim3(gb), dim3(bt), 0, 0, which, seed, site, sweep, (long long)n, d0.as<double>(), d1.as<double>(), dout.as<double>(), dtab.as<double>());
    HIPCHK(hipGetLastError());
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(out, dout.p, n * sizeof(double), hipMemcpyDeviceToHost));
    return 0;
}

int erm_sample_gig(int device, uint64_t seed, uint32_t site, uint32_t sweep, int64_t n, double p, double a, double b, double* out)
{
    if (n <= 0 || !out) return fail(ERM_ERR_ARG, "bad n/out");
    if (!(a > 0.0) || !(b > 0.0) || !std::isfinite(p) || p == 0.0) return fail(ERM_ERR_ARG, "GIG(p, a, b) needs a > 0, b > 0 and a finite p != 0");
    HIPCHK(hipSetDevice(device));
    DevBuf dout;
    if (int rc = dout.alloc(n * sizeof(double))) return rc;
    hipLaunchKernelGGL(gig_batch_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, seed, site, sweep, (long long)n, p, a, b, dout.as<double>());
    HIPCHK(hipGetLastError());
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(out, dout.p, n * sizeof(double), hipMemcpyDeviceToHost));
    return 0;
}

}  // extern "C"

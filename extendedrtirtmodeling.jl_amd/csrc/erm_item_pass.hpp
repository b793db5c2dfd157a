// erm_item_pass.hpp -- the host path of the six passes that run after sampling from a data set and a table of item-trace rows: the marginal WAIC,
// the marginal PSIS-LOO, the scores, the plausible values, the person fit (7n) and the item fit (7o).  A pass is ONE row of ITEM_PASSES, ONE product (item_waic /
// item_loo / item_scores / item_pv / item_fit / item_itemfit) and, per kind of source, ONE entry body in ertirt.hip: its argument checks, the source maker
// (item_source: an engine, a farm, or caller data with or without an observed mask) and the product call.  LatentQr's marginal WAIC and LOO
//  are the same makers and products for FAMILY_QUANTILE.
//
// The first half is plain C++: the facts of a pass as one table, the refusals built from it and the chunk rule; g++ compiles this half with
// -fsanitize=undefined -ftrapv into tests/item_pass_check (tests/test_item_pass_host.py).
// The second half (hipcc only) is what the tile kernels share of a launch, the coarse flags, the resolved source with its three makers, the tail the four table
// products share (item_finish) and the products.
// ertirt.hip includes this header where its DevBuf, fail / HIPCHK, pw_totals / pw_finish_on, EngineBase and the two handles are in scope.
#pragma once
#include <algorithm>
#include <cstdint>
#include <string>
#include "erm_obs.hpp"

namespace erm {

enum ItemPass { PASS_WAIC = 0, PASS_LOO, PASS_SCORES, PASS_PV, PASS_FIT, PASS_ITEM_FIT, N_ITEM_PASSES };
// the family of models an entry serves: the five without quantile weights (zeta's integral is Gaussian: erm_marginal.hpp), or LatentQr with nu integrated out
// (erm_qmarginal.hpp: the marginal WAIC and LOO only)
enum ItemFamily { FAMILY_GAUSSIAN = 0, FAMILY_QUANTILE };
// noun: the pass as its refusals name it; engine_rows: the fewest post-burn-in rows an engine must hold (0: the pass has limits of its own -- PSIS-LOO's
// 25 .. 8192); farm_rows: the fewest every chain of a farm must hold; need: what the refusal of too few rows asks for
struct ItemPassFacts { const char* noun; bool plural; int engine_rows, farm_rows; const char* need; };
constexpr ItemPassFacts ITEM_PASSES[N_ITEM_PASSES] = {
    { "the marginal WAIC",    false, 2, 2, "at least two post-burn-in rows" },
    { "the marginal LOO",     false, 0, 1, "post-burn-in rows (25 .. 8192 over the chains)" },
    { "the scores",           true,  1, 1, "at least one post-burn-in row" },
    { "the plausible values", true,  1, 1, "at least one post-burn-in row" },
    { "the person fit",       false, 1, 1, "at least one post-burn-in row" },
    { "the item fit",         false, 1, 1, "at least one post-burn-in row" },
};
inline std::string item_pass_on_shard(int pass)
{
    const ItemPassFacts& p = ITEM_PASSES[pass];
    return std::string(p.noun) + (p.plural ? " are" : " is") + " not available on a shard (every subject's data must be resident on one device)";
}
// too few rows: an engine's own (engine_rows > 0) and a farm chain's ("chain l: " in front)
inline std::string item_pass_needs_rows(int pass)
{
    const ItemPassFacts& p = ITEM_PASSES[pass];
    return std::string(p.noun) + (p.plural ? " need " : " needs ") + p.need;
}

// The subjects of a pass go through in chunks whose per-chunk device buffers fit 256 MB whatever a subject costs; cap > 0: a shorter chunk (the callers'
// ERM_PV_CHUNK / ERM_PSIS_CHUNK, for the tests of the chunk tails)
inline int64_t item_pass_chunk(int64_t bytes_per_subject, int64_t N, int64_t cap)
{
    int64_t chunk = std::max<int64_t>(1, ((int64_t)256 << 20) / bytes_per_subject);
    if (cap > 0) chunk = std::min(chunk, cap);
    return std::min(chunk, N);
}

}  // namespace erm

#ifdef __HIPCC__
namespace {      // (as ertirt.hip's own: EngineBase names ItemSource)

// ---- what marginal_kernel, score_kernel and pv_kernel share of a launch.  Everything a launch is given lives on the current device.
// a data set as the kernels read it: row-major, C and X in the element type of `elem` bytes (float or double)
// (q_rt: the quantile level, read for LatentQr only).  off != NULL: an incomplete data set (DESIGN.md 7m, fp64 only) -- Y, C and idx are erm_obs.hpp's compacted
// cell lists, subject i's at the positions off[i] .. off[i + 1]; the tile kernels' MASKED instantiations read it
struct MargData { const uint8_t* Y; const void* C; const void* X; const double* cm; int64_t N; int J, Fk, model; size_t elem; double q_rt;
                  const uint16_t* idx = nullptr; const int64_t* off = nullptr; };
static int marg_refuse_crossqr()
{
    return fail(ERM_ERR_ARG, "CrossQr is not served: with the quantile weights nu_ij integrated out every cell's response time is asymmetric Laplace in zeta, "
                             "so the zeta integral is piecewise with J kinks that move with theta and has no closed form");
}
// what the entries of a family refuse: the other family's models, by name of the entry that serves them
static int marg_refuse_model(int model, int family = FAMILY_GAUSSIAN)
{
    if (family == FAMILY_QUANTILE) {
        if (model == ERM_MODEL_CROSSQR) return marg_refuse_crossqr();
        if (marg_served(model)) return fail(ERM_ERR_ARG, "the quantile entries serve LatentQr only: this model has no quantile weights, use erm_get_marginal_waic / erm_get_marginal_loo / erm_marginal_loglik");
        return qmarg_served(model) ? 0 : fail(ERM_ERR_ARG, "unknown model");
    }
    if (model == ERM_MODEL_CROSSQR || model == ERM_MODEL_LATENTQR)
        return fail(ERM_ERR_ARG, "this entry serves the five models without quantile weights: with nu integrated out the response-time term is no longer Gaussian in zeta "
                                 "(LatentQr: the zeta integral is that of erm_get_quantile_marginal_waic / erm_get_quantile_marginal_loo; CrossQr: it has no closed form)");
    if (!marg_served(model)) return fail(ERM_ERR_ARG, "unknown model");
    return 0;
}
static int marg_nodes(int32_t n_nodes, int* Q)
{
    *Q = n_nodes == 0 ? MARG_NODES_DEFAULT : n_nodes;
    if (!marg_nodes_ok(*Q)) return fail(ERM_ERR_ARG, "n_nodes must be 0 (= " + std::to_string(MARG_NODES_DEFAULT) + ") or odd and in " + std::to_string(MARG_NODES_MIN) + " .. " + std::to_string(MARG_NODES_MAX));
    return 0;
}
// the arguments common to the three kernels (the outputs are the caller's to set), the LDS of the row double buffer, the grid of one tile per workgroup, the
// instantiation for the data set's model and element type -- launch(model constant, real()) --, and the subjects [c0, c0 + nc) of a data set as a data set of their own
static MargArgs marg_args(const MargData& D, const double* rows, int64_t n_rows, int Q)
{
    MargArgs a{};
    a.Y = D.Y; a.C = D.C; a.X = D.X; a.cm = D.cm; a.rows = rows; a.n_rows = n_rows; a.ld = item_trace_width(D.model, D.J, D.Fk); a.N = D.N; a.J = D.J; a.F = D.Fk; a.Q = Q; a.q = D.q_rt;
    a.idx = D.idx; a.off = reinterpret_cast<const long long*>(D.off);
    return a;
}
static size_t marg_lds(const MargArgs& a) { return (size_t)2 * marg_row_lds(a.ld, a.J) * sizeof(double); }
static dim3 marg_grid(const MargArgs& a) { return dim3((unsigned)((a.N + MARG_TILE - 1) / MARG_TILE)); }
template <typename Launch>
static int marg_dispatch(const MargData& D, Launch&& launch)
{
    auto of = [&](auto M) -> int { return D.elem == sizeof(float) ? launch(M, float()) : launch(M, double()); };
    switch (D.model) {
    case ERM_MODEL_MLIRT: return of(std::integral_constant<int, MLIRT>{});
    case ERM_MODEL_RTIRT: return of(std::integral_constant<int, RTIRT>{});
    case ERM_MODEL_NULL: return of(std::integral_constant<int, NULLM>{});
    case ERM_MODEL_CROSS: return of(std::integral_constant<int, CROSS>{});
    case ERM_MODEL_LATENT: return of(std::integral_constant<int, LATENT>{});
    default: return marg_refuse_model(D.model);
    }
}
static MargData marg_chunk(const MargData& D, int64_t c0, int64_t nc)
{
    MargData Dc = D;
    Dc.N = nc;
    Dc.X = D.X ? static_cast<const char*>(D.X) + (size_t)c0 * D.Fk * D.elem : nullptr;
    if (D.off) { Dc.off = D.off + c0; return Dc; }        // an incomplete data set: the offsets are absolute, so the lists stay where they are
    Dc.Y = D.Y + (size_t)c0 * D.J;
    Dc.C = D.C ? static_cast<const char*>(D.C) + (size_t)c0 * D.J * D.elem : nullptr;
    return Dc;
}
// the instantiation for a data set's completeness as well: launch(model constant, real(), masked constant); the compacted lists are fp64
template <typename Launch>
static int marg_dispatch_obs(const MargData& D, Launch&& launch)
{
    if (!D.off) return marg_dispatch(D, [&](auto M, auto real) { return launch(M, real, std::false_type{}); });
    if (D.elem != sizeof(double)) return fail(ERM_ERR_STATE, "an incomplete data set is fp64");
    return marg_dispatch(D, [&](auto M, auto real) -> int {
        if constexpr (std::is_same_v<decltype(real), double>) return launch(M, real, std::true_type{});
        else return fail(ERM_ERR_STATE, "an incomplete data set is fp64");
    });
}
// one launch of a tile kernel with the arguments a (and the kernel's own), waited for
template <typename... P, typename... A>
static int marg_tile_launch(void (*kernel)(P...), const MargArgs& a, hipStream_t stream, const A&... own)
{
    const size_t lds = marg_lds(a);
    HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(kernel, marg_grid(a), dim3(256), lds, stream, a, own...);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(stream));
    return 0;
}
// one launch of marginal_kernel over the subjects of D and the table of rows: l_dev [n_rows][D.N], the accumulators and the flags [D.N], any of them NULL
static int marginal_launch(const MargData& D, const double* rows, int64_t n_rows, int Q, hipStream_t stream, double* l_dev, double2* acc_ms, double2* acc_w, unsigned int* coarse)
{
    MargArgs a = marg_args(D, rows, n_rows, Q);
    a.l_out = l_dev; a.acc_ms = acc_ms; a.acc_w = acc_w; a.coarse = coarse;
    if (D.model == ERM_MODEL_LATENTQR)      // the one kernel LatentQr has (a source of FAMILY_QUANTILE; marg_dispatch's kernels refuse the model)
        return D.elem == sizeof(float) ? marg_tile_launch(&marginal_kernel<LATENTQR, float>, a, stream) : marg_tile_launch(&marginal_kernel<LATENTQR, double>, a, stream);
    return marg_dispatch_obs(D, [&](auto M, auto real, auto masked) { return marg_tile_launch(&marginal_kernel<decltype(M)::value, decltype(real), decltype(masked)::value>, a, stream); });
}

// The coarse flags of a pass: flags()[i] = 1 if subject i's grid was too coarse at any row, written by the tile kernels (a chunk's at flags() + c0), and their
// count (marginal_count_kernel).  Not allocated: flags() is NULL, which the kernels take for "no flags".
struct CoarseFlags {
    DevBuf dFlag, dCnt; int64_t N = 0;
    int alloc(int64_t n, const char* what) {
        N = n;
        if (int rc = dFlag.try_alloc((size_t)n * sizeof(unsigned int), what)) return rc;
        return dCnt.try_alloc(sizeof(unsigned long long), what);
    }
    unsigned int* flags() const { return dFlag.as<unsigned int>(); }
    int count(hipStream_t stream, unsigned long long* n) const {
        hipLaunchKernelGGL(marginal_count_kernel, dim3(1), dim3(256), 0, stream, flags(), (long long)N, dCnt.as<unsigned long long>());
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(stream));
        HIPCHK(hipMemcpy(n, dCnt.p, sizeof(*n), hipMemcpyDeviceToHost));
        return 0;
    }
};

// ---- PSIS-LOO (erm_psis_kernels.hpp): the one place that launches psis_kernel -- for item_loo's l, which marginal_kernel writes chunk by chunk, and for
// erm_psis_loo's caller-supplied table.  The subjects go through in chunks (item_pass_chunk; ERM_PSIS_CHUNK caps the chunk length); fill(c0, nc, dst) puts l of the
// subjects [c0, c0 + nc) into dst as [S][nc], and take(c0, nc, src), if wanted, receives their smoothed log-weights in the same layout.
static int psis_rows_ok(int64_t S)
{
    if (S < PSIS_MIN_ROWS) return fail(ERM_ERR_ARG, "PSIS-LOO needs at least " + std::to_string(PSIS_MIN_ROWS) + " rows per unit (" + std::to_string(S) + " given): fewer leave a tail of less than 5 values");
    if (S > PSIS_MAX_ROWS) return fail(ERM_ERR_ARG, "PSIS-LOO takes at most " + std::to_string(PSIS_MAX_ROWS) + " rows per unit (" + std::to_string(S) + " given): a unit's rows are sorted in LDS");
    return 0;
}
static int64_t item_chunk_cap(const char* name) { const char* e = getenv(name); return e ? atoll(e) : 0; }
template <typename Fill, typename Take>
static int psis_run(int64_t N, int64_t S, hipStream_t stream, Fill&& fill, Take&& take, bool want_lw, double* out8, double* pw)
{
    const int P = rk_pad((int)S);
    const int64_t chunk = item_pass_chunk(S * (int64_t)sizeof(double), N, item_chunk_cap("ERM_PSIS_CHUNK"));
    DevBuf dL, dXs, dPw, dOut;
    if (int rc = dL.try_alloc((size_t)chunk * S * sizeof(double), "PSIS-LOO's log-likelihoods")) return rc;
    if (int rc = dXs.try_alloc((size_t)chunk * S * sizeof(double), "PSIS-LOO's staged log-likelihoods")) return rc;
    if (int rc = dPw.try_alloc((size_t)N * PSIS_DEV_COLS * sizeof(double), "PSIS-LOO's pointwise table")) return rc;
    if (int rc = dOut.try_alloc(8 * sizeof(double), "PSIS-LOO's totals")) return rc;
    const int tps = P <= 2048 ? 64 : P <= 4096 ? 128 : 256, ns = 256 / tps;
    const size_t lds = (size_t)ns * P * 10;
    const void* kern = tps == 64 ? reinterpret_cast<const void*>(&psis_kernel<64>) : tps == 128 ? reinterpret_cast<const void*>(&psis_kernel<128>) : reinterpret_cast<const void*>(&psis_kernel<256>);
    HIPCHK(hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    for (int64_t c0 = 0; c0 < N; c0 += chunk) {
        const int64_t nc = std::min(chunk, N - c0);
        if (int rc = fill(c0, nc, dL.as<double>())) return rc;
        hipLaunchKernelGGL(psis_transpose_kernel, dim3((unsigned)((nc + 31) / 32), (unsigned)((S + 31) / 32)), dim3(256), 0, stream, dL.as<double>(), (long long)S, (long long)nc, dXs.as<double>());
        PsisArgs a{};
        a.xs = dXs.as<double>(); a.n = nc; a.S = (int)S; a.P = P; a.pw = dPw.as<double>(); a.n_all = N; a.c0 = c0; a.want_lw = want_lw ? 1 : 0;
        const dim3 grid((unsigned)((nc + ns - 1) / ns));
        if (tps == 64) hipLaunchKernelGGL(psis_kernel<64>, grid, dim3(256), lds, stream, a);
        else if (tps == 128) hipLaunchKernelGGL(psis_kernel<128>, grid, dim3(256), lds, stream, a);
        else hipLaunchKernelGGL(psis_kernel<256>, grid, dim3(256), lds, stream, a);
        if (want_lw) hipLaunchKernelGGL(psis_transpose_kernel, dim3((unsigned)((S + 31) / 32), (unsigned)((nc + 31) / 32)), dim3(256), 0, stream, dXs.as<double>(), (long long)nc, (long long)S, dL.as<double>());
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(stream));
        if (want_lw) if (int rc = take(c0, nc, dL.as<double>())) return rc;
    }
    hipLaunchKernelGGL(psis_totals_kernel, dim3(1), dim3(256), 0, stream, dPw.as<double>(), (long long)N, psis_k_threshold(S), dOut.as<double>());
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(stream));
    HIPCHK(hipMemcpy(out8, dOut.p, 8 * sizeof(double), hipMemcpyDeviceToHost));
    if (pw) HIPCHK(hipMemcpy(pw, dPw.p, (size_t)N * PSIS_COLS * sizeof(double), hipMemcpyDeviceToHost));
    return 0;
}
// out12 from psis_totals_kernel's sums
static void psis_out12(const double* s8, int64_t N, int64_t S, int Q, int64_t n_coarse, double* out12)
{
    const double U = (double)N, var_u = N > 1 ? s8[3] / (U - 1.0) : 0.0;
    out12[0] = s8[0]; out12[1] = s8[1]; out12[2] = -2.0 * s8[0]; out12[3] = 2.0 * std::sqrt(U * var_u); out12[4] = s8[2]; out12[5] = U; out12[6] = (double)S;
    out12[7] = s8[4]; out12[8] = s8[5]; out12[9] = (double)psis_tail_len(S); out12[10] = (double)Q; out12[11] = (double)n_coarse;
}

// ---- The resolved source of a pass: a data set and a table of n_rows item-trace rows on the current device, the stream the kernels run on, and the device
// buffers the source owns (caller data: all four; a farm: its table of rows; an engine: none, everything is read in place).
struct ItemSource {
    MargData D{}; const double* rows = nullptr; int64_t n_rows = 0; hipStream_t stream = nullptr;
    DevBuf dY, dC, dX, dRows, dIdx, dOff;
};
// an engine's resident data set and its own post-burn-in rows, read in place (EngineBase::item_source: the refusals of a shard, a poisoned state, no data set and
// too few rows, in this order, after the model's)
static int item_source(erm_handle h, int pass, ItemSource& S, int family = FAMILY_GAUSSIAN)
{
    if (int rc = marg_refuse_model(h->e->cfg.model, family)) return rc;
    return h->e->item_source(pass, S);
}
// a farm's: the post-burn-in item-trace rows of chain 0, chain 1, ... as ONE table on chain 0's device, whose resident data set supplies the data.  A chain's rows
// cross through the host whatever its device (item-level: a few hundred kilobytes); a farm of one chain takes the same path as several.
static int item_source(erm_farm_handle f, int pass, ItemSource& S, int family = FAMILY_GAUSSIAN)
{
    if (int rc = marg_refuse_model(f->cfg.model, family)) return rc;
    const int L = (int)f->eng.size();
    const EngineBase* e0 = f->eng[0]->e.get();
    const int64_t wi = e0->item_trace_width(), rows = e0->rows_done, post = e0->post_rows;
    for (int l = 0; l < L; ++l) {
        const EngineBase* e = f->eng[l]->e.get();
        if (e->rows_done != rows) return fail(ERM_ERR_STATE, "chain " + std::to_string(l) + ": " + std::to_string(e->rows_done) + " rows recorded where chain 0 has " + std::to_string(rows));
        if (e->post_rows < ITEM_PASSES[pass].farm_rows) return fail(ERM_ERR_STATE, "chain " + std::to_string(l) + ": " + item_pass_needs_rows(pass));
    }
    std::vector<double> table((size_t)L * post * wi);
    for (int l = 0; l < L; ++l) {
        const EngineBase* e = f->eng[l]->e.get();
        HIPCHK(hipSetDevice(f->dev[l]));
        HIPCHK(hipStreamSynchronize(e->work_stream()));
        HIPCHK(hipMemcpy(table.data() + (size_t)l * post * wi, e->item_trace_dev() + (size_t)(rows - post) * wi, (size_t)post * wi * sizeof(double), hipMemcpyDeviceToHost));
    }
    HIPCHK(hipSetDevice(f->dev[0]));
    if (int rc = S.dRows.try_alloc(table.size() * sizeof(double), "the farm's table of item-trace rows")) return rc;
    H2D(S.dRows.p, table.data(), table.size() * sizeof(double));
    S.rows = S.dRows.as<double>(); S.n_rows = (int64_t)L * post;
    return item_source(f->eng[0].get(), pass, S, family);
}
// what every caller-data entry is given of a data set and its rows: Y, logT, X column-major as the ABI takes them, rows [n_rows][item-trace width]
struct CallerData { int device, model; int64_t n_subj; int32_t n_item, n_feat; const uint8_t* Y; const double* logT; const double* X; const double* rows; int64_t n_rows; };
// caller-supplied data and rows (erm_marginal_loglik, erm_score, erm_plausible_values): validated on the host, then uploaded to `device` row-major in fp64, as the
// kernels read an engine's, for the NULL stream.  min_rows / rows_msg: the fewest rows the caller's outputs need.  FAMILY_QUANTILE (the model is LatentQr): q_rt is
// the quantile level, and every row's Sigma_p[2,2], the scale of zeta's law, must be positive.
// obs != NULL (the masked entries): the observed mask, column-major as Y.  The walk that validates the cells compacts them into erm_obs.hpp's lists,
// which are uploaded in the place of the row-major Y and logT; Y and logT are read, and validated, at observed cells only; n_obs [n_subj] (may be NULL) receives n_i.
static int item_source(const char* what, const CallerData& d, int64_t min_rows, const char* rows_msg, ItemSource& S, int family = FAMILY_GAUSSIAN, double q_rt = 0.0,
                       const uint8_t* obs = nullptr, int32_t* n_obs = nullptr)
{
    const auto& [device, model, n_subj, n_item, n_feat, Y, logT, X, rows, n_rows] = d;
    const ModelTraits mt = model_traits(model);
    if (n_subj <= 0 || n_subj >= (1LL << 32) || n_item <= 0 || n_item > 896 || n_feat < 0 || n_feat > MARG_MAXF) return fail(ERM_ERR_ARG, "n_subj, n_item (1 .. 896) or n_feat (0 .. " + std::to_string(MARG_MAXF) + ") out of range");
    const int64_t N = n_subj; const int J = n_item, Fk = kernel_feat(model, n_feat);
    if (!Y || !rows) return fail(ERM_ERR_ARG, "Y / rows is NULL");
    if (mt.rt && !logT) return fail(ERM_ERR_ARG, "logT is required for response-time models");
    if (Fk > 0 && !X) return fail(ERM_ERR_ARG, "X is required when n_feat > 0");
    if (n_rows < min_rows) return fail(ERM_ERR_ARG, rows_msg);
    if (family == FAMILY_QUANTILE && !qmarg_level_ok(q_rt)) return fail(ERM_ERR_ARG, "q_rt must be inside (0, 1)");
    const int64_t wi = item_trace_width(model, J, Fk);
    const size_t NJ = (size_t)N * J;
    // ---- the inputs: a NaN anywhere, then rows outside the model's domain
    for (size_t e = 0; e < (size_t)n_rows * wi; ++e) if (rows[e] != rows[e]) return fail(ERM_ERR_NONFINITE, "NaN in row " + std::to_string(e / (size_t)wi));
    std::vector<int64_t> off;
    std::vector<uint16_t> idx; std::vector<uint8_t> yl; std::vector<double> tl;
    int bad_cells = OBS_OK;
    if (obs) {
        off.resize((size_t)N + 1);
        std::vector<int64_t> cur((size_t)N);
        int64_t bad = 0;
        if (obs_offsets(obs, N, J, off.data(), &bad) != OBS_OK) return fail(ERM_ERR_ARG, "obs must be 0/1 (subject " + std::to_string(bad % N) + ", item " + std::to_string(bad / N) + ")");
        const size_t total = (size_t)off[(size_t)N];
        idx.resize(total); yl.resize(total); if (mt.rt) tl.resize(total);
        bad_cells = obs_compact(Y, mt.rt ? logT : nullptr, obs, N, J, off.data(), cur.data(), idx.data(), yl.data(), mt.rt ? tl.data() : nullptr, &bad);
        if (bad_cells == OBS_NAN_LOGT) return fail(ERM_ERR_NONFINITE, "NaN in logT at an observed cell");
    }
    else if (mt.rt) for (size_t e = 0; e < NJ; ++e) if (logT[e] != logT[e]) return fail(ERM_ERR_NONFINITE, "NaN in logT");
    for (size_t e = 0; e < (size_t)N * Fk; ++e) if (X[e] != X[e]) return fail(ERM_ERR_NONFINITE, "NaN in X");
    if (bad_cells == OBS_BAD_Y) return fail(ERM_ERR_ARG, "Y must be 0/1 at every observed cell");
    if (!obs) for (size_t e = 0; e < NJ; ++e) if (Y[e] > 1) return fail(ERM_ERR_ARG, "Y must be 0/1");
    if (mt.rt) for (int64_t r = 0; r < n_rows; ++r) {
        const double* row = rows + (size_t)r * wi;
        for (int j = 0; j < J; ++j) if (!(row[3 * J + j] > 0.0)) return fail(ERM_ERR_ARG, "row " + std::to_string(r) + ": sig2t must be positive");
        const double* Sp = row + 4 * J + qr_sigp_off(model, J, Fk);
        if (!(Sp[0] > 0.0)) return fail(ERM_ERR_ARG, "row " + std::to_string(r) + ": Sigma_p[1,1] must be positive");
        if (family == FAMILY_QUANTILE && !(Sp[3] > 0.0)) return fail(ERM_ERR_ARG, "row " + std::to_string(r) + ": Sigma_p[2,2] must be positive");
        if (marg_law(model, 0.0, 0.0, 0.0, Sp).v < 0.0) return fail(ERM_ERR_ARG, "row " + std::to_string(r) + ": the conditional variance of zeta given theta is negative (Sigma_p is not positive semi-definite)");
    }
    HIPCHK(hipSetDevice(device));
    // ---- upload: the data set row-major in fp64, as the kernel reads an engine's -- or its compacted lists (one spare element: an empty list still has a base)
    if (obs) {
        const size_t total = idx.size();
        if (int rc = S.dOff.try_alloc(off.size() * sizeof(int64_t), what)) return rc;
        if (int rc = S.dIdx.try_alloc((total + 1) * sizeof(uint16_t), what)) return rc;
        if (int rc = S.dY.try_alloc(total + 1, what)) return rc;
        if (mt.rt) if (int rc = S.dC.try_alloc((total + 1) * sizeof(double), what)) return rc;
        H2D(S.dOff.p, off.data(), off.size() * sizeof(int64_t));
        if (total > 0) {
            H2D(S.dIdx.p, idx.data(), total * sizeof(uint16_t));
            H2D(S.dY.p, yl.data(), total);
            if (mt.rt) H2D(S.dC.p, tl.data(), total * sizeof(double));
        }
        if (n_obs) for (int64_t i = 0; i < N; ++i) n_obs[i] = (int32_t)(off[(size_t)i + 1] - off[(size_t)i]);
    }
    else {
        std::vector<uint8_t> y(NJ);
        cols_to_rows(Y, y.data(), N, (int64_t)J);
        if (int rc = S.dY.try_alloc(NJ, what)) return rc;
        H2D(S.dY.p, y.data(), NJ);
    }
    if (mt.rt && !obs) {
        std::vector<double> c(NJ);
        cols_to_rows(logT, c.data(), N, (int64_t)J);
        if (int rc = S.dC.try_alloc(NJ * sizeof(double), what)) return rc;
        H2D(S.dC.p, c.data(), NJ * sizeof(double));
    }
    if (Fk > 0) {
        std::vector<double> x((size_t)N * Fk);
        cols_to_rows(X, x.data(), N, (int64_t)Fk);
        if (int rc = S.dX.try_alloc(x.size() * sizeof(double), what)) return rc;
        H2D(S.dX.p, x.data(), x.size() * sizeof(double));
    }
    if (int rc = S.dRows.try_alloc((size_t)n_rows * wi * sizeof(double), what)) return rc;
    H2D(S.dRows.p, rows, (size_t)n_rows * wi * sizeof(double));
    S.D = MargData{S.dY.as<uint8_t>(), S.dC.p, S.dX.p, nullptr, N, J, Fk, model, sizeof(double), q_rt, S.dIdx.as<uint16_t>(), S.dOff.as<int64_t>()};
    S.rows = S.dRows.as<double>(); S.n_rows = n_rows;
    return 0;
}

// The tail of the scores, the person fit, the item fit and the plausible values: the count of the coarse flags, the pass's table to the caller (dst NULL: not
// wanted) and out4 = {N, n_rows, Q, n_coarse} (may be NULL)
static int item_finish(const ItemSource& S, int Q, const CoarseFlags& coarse, void* dst, const void* src, size_t bytes, double* out4)
{
    unsigned long long nc = 0;
    if (int rc = coarse.count(S.stream, &nc)) return rc;
    if (dst) HIPCHK(hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost));
    if (out4) { out4[0] = (double)S.D.N; out4[1] = (double)S.n_rows; out4[2] = (double)Q; out4[3] = (double)nc; }
    return 0;
}

// ---- The products of a source.  The makers have refused a source with too few rows for the outputs asked for; all outputs are the caller's host arrays.
// Marginal WAIC (erm_marginal_kernels.hpp; include/ertirt.h: erm_get_marginal_waic, erm_marginal_loglik): l [n_rows][N] (may be NULL), and the totals out10 with
// lppd_u / p_u [N] (all three NULL: l alone)
static int item_waic(const ItemSource& S, int Q, double* l, double* out10, double* lppd_u, double* p_u)
{
    const bool totals = out10 || lppd_u || p_u;
    const int64_t N = S.D.N;
    DevBuf dMs, dW, dL, dP, dLik;
    CoarseFlags coarse;
    const char* what = "the marginal WAIC's accumulators";
    if (l) if (int rc = dLik.try_alloc((size_t)N * S.n_rows * sizeof(double), "erm_marginal_loglik's output")) return rc;
    if (totals) {
        if (int rc = dMs.try_alloc((size_t)N * sizeof(double2), what)) return rc;
        if (int rc = dW.try_alloc((size_t)N * sizeof(double2), what)) return rc;
        if (int rc = coarse.alloc(N, what)) return rc;
        if (lppd_u) if (int rc = dL.try_alloc((size_t)N * sizeof(double), what)) return rc;
        if (p_u) if (int rc = dP.try_alloc((size_t)N * sizeof(double), what)) return rc;
    }
    if (int rc = marginal_launch(S.D, S.rows, S.n_rows, Q, S.stream, dLik.as<double>(), dMs.as<double2>(), dW.as<double2>(), coarse.flags())) return rc;
    if (l) HIPCHK(hipMemcpy(l, dLik.p, (size_t)N * S.n_rows * sizeof(double), hipMemcpyDeviceToHost));
    if (!totals) return 0;
    double out8[8], sums[PW_FIN_COLS];
    if (int rc = pw_totals(dMs.as<double2>(), dW.as<double2>(), N, S.n_rows, S.stream, out8)) return rc;
    if (lppd_u || p_u) {
        if (int rc = pw_finish_on(dMs.as<double2>(), dW.as<double2>(), N, S.n_rows, 0.0, dL.as<double>(), dP.as<double>(), S.stream, sums)) return rc;
        if (lppd_u) HIPCHK(hipMemcpy(lppd_u, dL.p, (size_t)N * sizeof(double), hipMemcpyDeviceToHost));
        if (p_u) HIPCHK(hipMemcpy(p_u, dP.p, (size_t)N * sizeof(double), hipMemcpyDeviceToHost));
    }
    if (out10) {
        unsigned long long nc = 0;
        if (int rc = coarse.count(S.stream, &nc)) return rc;
        for (int k = 0; k < 8; ++k) out10[k] = out8[k];
        out10[8] = (double)Q; out10[9] = (double)nc;
    }
    return 0;
}
// Marginal PSIS-LOO (include/ertirt.h: erm_get_marginal_loo): psis_run on l of every chunk from marginal_kernel; 25 .. 8192 rows
static int item_loo(const ItemSource& S, int Q, double* out12, double* pw)
{
    if (int rc = psis_rows_ok(S.n_rows)) return rc;
    const int64_t N = S.D.N;
    CoarseFlags coarse;
    if (int rc = coarse.alloc(N, "the marginal LOO's flags")) return rc;
    auto fill = [&](int64_t c0, int64_t nc, double* dst) -> int {
        return marginal_launch(marg_chunk(S.D, c0, nc), S.rows, S.n_rows, Q, S.stream, dst, nullptr, nullptr, coarse.flags() + c0);
    };
    double s8[8];
    if (int rc = psis_run(N, S.n_rows, S.stream, fill, [](int64_t, int64_t, const double*) { return 0; }, false, s8, pw)) return rc;
    unsigned long long nc = 0;
    if (int rc = coarse.count(S.stream, &nc)) return rc;
    psis_out12(s8, N, S.n_rows, Q, (int64_t)nc, out12);
    return 0;
}
// The two per-subject tables, table [N][cols]: one launch of the tile kernel that kernel(model constant, real(), masked constant) picks, over all subjects.
// `what` names the pass in the allocation messages.
template <typename Pick>
static int item_subject_table(const ItemSource& S, int Q, int cols, const char* what, Pick&& kernel, double* table, double* out4)
{
    const int64_t N = S.D.N;
    DevBuf dTable;
    CoarseFlags coarse;
    if (int rc = dTable.try_alloc((size_t)N * cols * sizeof(double), what)) return rc;
    if (int rc = coarse.alloc(N, what)) return rc;
    MargArgs a = marg_args(S.D, S.rows, S.n_rows, Q);
    a.coarse = coarse.flags();
    if (int rc = marg_dispatch_obs(S.D, [&](auto M, auto real, auto masked) { return marg_tile_launch(kernel(M, real, masked), a, S.stream, dTable.as<double>()); })) return rc;
    return item_finish(S, Q, coarse, table, dTable.p, (size_t)N * cols * sizeof(double), out4);
}
// Scores of respondents (erm_score_kernels.hpp; include/ertirt.h: erm_get_scores, erm_score): the one place that launches score_kernel; score [N][7]
static int item_scores(const ItemSource& S, int Q, int weighting, double* score, double* out4)
{
    return item_subject_table(S, Q, SCORE_COLS, "the scores", [&](auto M, auto real, auto masked) {
        return weighting == SCORE_LIKELIHOOD ? &score_kernel<decltype(M)::value, decltype(real), true, decltype(masked)::value>
                                             : &score_kernel<decltype(M)::value, decltype(real), false, decltype(masked)::value>; }, score, out4);
}
// Person fit (erm_fit_kernels.hpp; include/ertirt.h: erm_get_person_fit, erm_person_fit): the one place that launches fit_kernel; fit [N][6]
static int item_fit(const ItemSource& S, int Q, int weighting, double* fit, double* out4)
{
    return item_subject_table(S, Q, FIT_COLS, "the person fit", [&](auto M, auto real, auto masked) {
        return weighting == SCORE_LIKELIHOOD ? &fit_kernel<decltype(M)::value, decltype(real), true, decltype(masked)::value>
                                             : &fit_kernel<decltype(M)::value, decltype(real), false, decltype(masked)::value>; }, fit, out4);
}
// Item fit (erm_ifit_kernels.hpp; include/ertirt.h: erm_get_item_fit, erm_item_fit): the one place that launches item_fit_kernel and its two reduction kernels;
// fit [J][6].  The subjects go through in chunks of whole blocks of IFIT_BLOCK (ifit_chunk on item_pass_chunk's budget for the 48 J bytes of a subject's workspace
// and the 8 Q of its parked nodes; ERM_IFIT_CHUNK caps the chunk length); every chunk leaves its block sums in a table that stage B reads once at the end.
static int item_itemfit(const ItemSource& S, int Q, double* fit, double* out4)
{
    const int64_t N = S.D.N;
    const int J = S.D.J;
    const int64_t per_subject = (int64_t)IFIT_VALS * sizeof(double) * J + (int64_t)sizeof(double) * Q;
    const int64_t chunk = ifit_chunk(item_pass_chunk(per_subject, INT64_MAX, 0), item_chunk_cap("ERM_IFIT_CHUNK"));
    const int64_t slots = std::min(chunk, ifit_blocks(N) * IFIT_BLOCK), n_blocks = ifit_blocks(N);      // (a multiple of IFIT_BLOCK, so of MARG_TILE)
    DevBuf dWs, dEq, dBlk, dFit;
    CoarseFlags coarse;
    const char* what = "the item fit";
    const size_t ws_bytes = (size_t)slots * J * IFIT_VALS * sizeof(double);
    if (int rc = dWs.try_alloc(ws_bytes, what)) return rc;
    if (int rc = dEq.try_alloc((size_t)slots * Q * sizeof(double), what)) return rc;
    if (int rc = dBlk.try_alloc((size_t)n_blocks * J * IFIT_SUMS * sizeof(double), what)) return rc;
    if (int rc = dFit.try_alloc((size_t)J * IFIT_COLS * sizeof(double), what)) return rc;
    if (int rc = coarse.alloc(N, what)) return rc;
    for (int64_t c0 = 0; c0 < N; c0 += chunk) {
        const int64_t nc = std::min(chunk, N - c0);
        const MargData Dc = marg_chunk(S.D, c0, nc);
        MargArgs a = marg_args(Dc, S.rows, S.n_rows, Q);
        a.coarse = coarse.flags() + c0;
        HIPCHK(hipMemsetAsync(dWs.p, 0, ws_bytes, S.stream));
        if (int rc = marg_dispatch_obs(S.D, [&](auto M, auto real, auto masked) {
                return marg_tile_launch(&item_fit_kernel<decltype(M)::value, decltype(real), decltype(masked)::value>, a, S.stream, dEq.as<double>(), dWs.as<double>()); })) return rc;
        hipLaunchKernelGGL(item_fit_block_kernel, dim3((unsigned)ifit_blocks(nc), (unsigned)J), dim3(IFIT_BLOCK), 0, S.stream, dWs.as<double>(), (long long)nc, J,
                           a.off, a.idx, dBlk.as<double>() + (size_t)(c0 / IFIT_BLOCK) * J * IFIT_SUMS);
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(S.stream));
    }
    hipLaunchKernelGGL(item_fit_finish_kernel, dim3((unsigned)((J + 255) / 256)), dim3(256), 0, S.stream, dBlk.as<double>(), (long long)n_blocks, J, (long long)S.n_rows,
                       model_traits(S.D.model).rt ? 1 : 0, dFit.as<double>());
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(S.stream));
    return item_finish(S, Q, coarse, fit, dFit.p, (size_t)J * IFIT_COLS * sizeof(double), out4);
}
// Plausible values (erm_pv_kernels.hpp; include/ertirt.h: erm_get_plausible_values, erm_plausible_values): the one place that launches pv_kernel.  The subjects
// go through in chunks whose draws (two doubles and an int each) fit item_pass_chunk's budget whatever K (ERM_PV_CHUNK caps the chunk length); a chunk's draws are
// copied into pv [N][K][2] and node [N][K] (may be NULL), column-major, before the next chunk runs.  coarse [N] may be NULL.
static int item_pv(const ItemSource& S, int Q, int64_t K, uint64_t seed, double* pv, int32_t* node, int32_t* coarse, double* out4)
{
    const int64_t N = S.D.N;
    const int64_t chunk = item_pass_chunk(K * (int64_t)(2 * sizeof(double) + sizeof(int)), N, item_chunk_cap("ERM_PV_CHUNK"));
    DevBuf dPv, dNode;
    CoarseFlags flags;
    const char* what = "the plausible values";
    if (int rc = dPv.try_alloc((size_t)chunk * K * 2 * sizeof(double), what)) return rc;
    if (node) if (int rc = dNode.try_alloc((size_t)chunk * K * sizeof(int), what)) return rc;
    if (int rc = flags.alloc(N, what)) return rc;
    for (int64_t c0 = 0; c0 < N; c0 += chunk) {
        const int64_t nc = std::min(chunk, N - c0);
        MargArgs a = marg_args(marg_chunk(S.D, c0, nc), S.rows, S.n_rows, Q);
        a.coarse = flags.flags() + c0;
        const PvArgs p{(long long)K, (unsigned long long)seed, (long long)c0, dPv.as<double>(), dNode.as<int>()};
        if (int rc = marg_dispatch_obs(S.D, [&](auto M, auto real, auto masked) { return marg_tile_launch(&pv_kernel<decltype(M)::value, decltype(real), decltype(masked)::value>, a, S.stream, p); })) return rc;
        HIPCHK(hipMemcpy2D(pv + c0, (size_t)N * sizeof(double), dPv.p, (size_t)nc * sizeof(double), (size_t)nc * sizeof(double), (size_t)(2 * K), hipMemcpyDeviceToHost));
        if (node) HIPCHK(hipMemcpy2D(node + c0, (size_t)N * sizeof(int), dNode.p, (size_t)nc * sizeof(int), (size_t)nc * sizeof(int), (size_t)K, hipMemcpyDeviceToHost));
    }
    return item_finish(S, Q, flags, coarse, flags.flags(), (size_t)N * sizeof(unsigned int), out4);      // (a flag is 0 or 1: the same four bytes as the caller's int32)
}

}  // namespace
#endif  // __HIPCC__

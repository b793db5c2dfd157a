// erm_model.hpp -- what distinguishes the seven models on the host, in ONE table, and every width, length and offset that follows from it.
// The host side (ertirt.hip) reads this table instead of switching on the model; extendedrtirtmodeling.jl_amd/_lib.py holds the same table
// (MODEL_TRAITS) for the Python side.  Plain C++: also compiled by g++ for the table's CPU test (tests/test_model_traits.py).
#pragma once
#include "erm_layout.hpp"

namespace erm {

enum NuShape : int { NU_NONE = 0, NU_SUBJECT = 1, NU_CELL = 2 };      // the quantile weights: absent, one per subject (N), one per cell (N * J)
// Para.beta: absent | nFeat+1 | (nFeat+1) x 2, column-major | nFeat+2 (zeta on [1 X theta]) | Null's (nFeat+1) x 2 that is zero in every sweep and never stored
enum BetaShape : int { BETA_NONE = 0, BETA_VEC = 1, BETA_PAIR = 2, BETA_LATENT = 3, BETA_ZERO_PAIR = 4 };
enum Generator : int { GEN_MLIRT = 0, GEN_RTIRT = 1, GEN_NULL = 2, GEN_CROSS = 3, GEN_LATENT = 4 };      // erm_simulate_data: setData* of src/SimTools.jl:117-368
enum Trace : int { TRACE_RA = 0, TRACE_RT = 1, TRACE_QR = 2, TRACE_LOGLIKE = 3 };                       // ERM_TRACE_* of include/ertirt.h

struct ModelTraits {
    bool rt;          // response times: logT, zeta, lambda, sig2t, Sigp, Post.rt
    bool rho;         // the cross-relation rho (J values, two row passes per sweep)
    int nu;           // NuShape
    bool sees_x;      // the kernels read Data.X
    int beta;         // BetaShape
    int gen;          // Generator
};

constexpr ModelTraits model_traits(int model)
{
    switch (model) {                                                       //  rt     rho    nu          sees_x beta            gen
    case MLIRT:    return {false, false, NU_NONE,    true,  BETA_VEC,       GEN_MLIRT};      // src/GibbsRtIrt.pl.jl:76-106
    case RTIRT:    return {true,  false, NU_NONE,    true,  BETA_PAIR,      GEN_RTIRT};      // :114-146
    case CROSSQR:  return {true,  true,  NU_CELL,    false, BETA_NONE,      GEN_CROSS};      // src/GibbsRtIrtCross.pl.jl:115-147
    case LATENTQR: return {true,  false, NU_SUBJECT, true,  BETA_LATENT,    GEN_LATENT};     // src/GibbsRtIrtLatent.pl.jl:105-137
    case NULLM:    return {true,  false, NU_NONE,    false, BETA_ZERO_PAIR, GEN_NULL};       // src/GibbsRtIrt.pl.jl:151-183 (beta = 0, :380)
    case CROSS:    return {true,  true,  NU_NONE,    false, BETA_NONE,      GEN_CROSS};      // src/GibbsRtIrtCross.pl.jl:77-110
    case LATENT:   return {true,  false, NU_NONE,    true,  BETA_LATENT,    GEN_LATENT};     // src/GibbsRtIrtLatent.pl.jl:70-102
    }
    return {false, false, NU_NONE, false, BETA_NONE, GEN_MLIRT};           // no such model (Engine::init refuses it)
}

constexpr bool traits_agree_with_families(int M)
{
    const ModelTraits t = model_traits(M);
    return t.rt == (fam_rt(M) || fam_lq(M) || fam_cq(M)) && t.rho == fam_cq(M) && (t.nu != NU_NONE) == has_nu(M) && (t.nu == NU_CELL) == (has_nu(M) && fam_cq(M)) &&
           (t.nu == NU_SUBJECT) == (has_nu(M) && fam_lq(M)) && (t.beta == BETA_PAIR || t.beta == BETA_ZERO_PAIR) == fam_rt(M) && (t.beta == BETA_LATENT) == fam_lq(M) &&
           (t.beta == BETA_NONE) == fam_cq(M) && (t.beta == BETA_VEC) == (M == MLIRT);
}
static_assert(traits_agree_with_families(MLIRT) && traits_agree_with_families(RTIRT) && traits_agree_with_families(CROSSQR) && traits_agree_with_families(LATENTQR) &&
              traits_agree_with_families(NULLM) && traits_agree_with_families(CROSS) && traits_agree_with_families(LATENT), "model_traits disagrees with fam_rt / fam_lq / fam_cq / has_nu");

// covariate columns the kernels see: the Cross family and Null never touch Data.X
constexpr int kernel_feat(int model, int F) { return model_traits(model).sees_x ? F : 0; }
// entries of a beta of shape `shape` over F covariate columns
constexpr int beta_len(int shape, int F) { return shape == BETA_VEC ? F + 1 : (shape == BETA_PAIR || shape == BETA_ZERO_PAIR) ? 2 * (F + 1) : shape == BETA_LATENT ? F + 2 : 0; }
// erm_state.beta as the caller sees it (Null: 2 (nFeat+1) zeros, src/GibbsRtIrt.pl.jl:380)
constexpr int nbeta(int model, int F) { return beta_len(model_traits(model).beta, F); }
// The small part of qr, [beta or rho | vec(Sigp)], twice.  As the kernels publish it in the item trace (tiny_publish): beta over the columns THEY see -- Null's is
// [beta_theta0, beta_zeta0] = 0 -- then Sigp at qr_sigp_off.  As Post.qr holds it (src/GibbsRtIrt.pl.jl:45,67; src/GibbsRtIrtCross.pl.jl:46,65;
// src/GibbsRtIrtLatent.pl.jl:43,60): qr_head columns of beta (over nFeat) or rho, then vec(Sigp).  The two differ for Null only.
constexpr int qr_sigp_off(int model, int J, int F) { return model_traits(model).rho ? J : beta_len(model_traits(model).beta, kernel_feat(model, F)); }
constexpr int nq(int model, int J, int F) { return qr_sigp_off(model, J, F) + (model_traits(model).rt ? 4 : 0); }
constexpr int qr_head(int model, int J, int F) { return model_traits(model).rho ? J : nbeta(model, F); }
// item-level trace row: a, b, lambda, sig2t [4][J], then the kernels' small part of qr
constexpr int64_t item_trace_width(int model, int J, int F) { return 4 * (int64_t)J + nq(model, J, F); }
// erm_state.nu (CrossQr: N x J, row-major on the device and column-major for the caller)
constexpr int64_t nu_len(int model, int64_t N, int J) { return model_traits(model).nu == NU_SUBJECT ? N : model_traits(model).nu == NU_CELL ? N * (int64_t)J : 0; }
// A trace as the caller sees it: at most four consecutive blocks of columns.  Post.ra = [theta; a; b] (src/GibbsRtIrt.pl.jl:44,65), Post.rt = [zeta; lambda; sig2t]
// (:66; MlIrt's stays []), Post.qr = [beta or rho | vec(Sigp) | nu] -- where Null's beta is 2 (nFeat + 1) constant zeros that no kernel stores (:398) and CrossQr's
// vec(nu) is column-major for the caller and row-major on the device.  Every routine that reads a trace back walks this list; nothing else says what a trace is made of.
enum BlockKind : int {
    BLK_SUBJECT = 0,      // one column per subject, from the subject-level trace `src` (SubjTrace)
    BLK_CELL = 1,         // one column per cell of N x J from the nu trace, kept in DEVICE order: column i * J + j of the block is the caller's j * N + i
    BLK_ITEM = 2,         // columns [src, src + ncol) of the item-level trace
    BLK_ZERO = 3          // constant zeros, stored nowhere
};
enum SubjTrace : int { SUBJ_THETA = 0, SUBJ_ZETA = 1, SUBJ_NU = 2 };
struct TraceBlock {
    int kind; int64_t ncol, col0, src;      // col0: the block's first column in the caller's trace
    constexpr bool device_order() const { return kind == BLK_CELL; }
};
struct TraceBlocks {
    int n = 0; TraceBlock b[4] = {};
    constexpr int64_t width() const { return n > 0 ? b[n - 1].col0 + b[n - 1].ncol : 0; }
    constexpr void add(int kind, int64_t ncol, int64_t src) { if (ncol > 0) { b[n] = TraceBlock{kind, ncol, width(), src}; ++n; } }      // (an empty block is no block)
    constexpr const TraceBlock* begin() const { return b; }
    constexpr const TraceBlock* end() const { return b + n; }
};
constexpr TraceBlocks trace_blocks(int model, int which, int64_t N, int J, int F)
{
    const ModelTraits t = model_traits(model);
    TraceBlocks tb;
    if (which == TRACE_RA) { tb.add(BLK_SUBJECT, N, SUBJ_THETA); tb.add(BLK_ITEM, 2 * (int64_t)J, 0); }
    if (which == TRACE_RT && t.rt) { tb.add(BLK_SUBJECT, N, SUBJ_ZETA); tb.add(BLK_ITEM, 2 * (int64_t)J, 2 * (int64_t)J); }
    if (which == TRACE_QR) {
        const int64_t q0 = 4 * (int64_t)J;      // the kernels' small part of qr in the item trace
        if (t.beta == BETA_ZERO_PAIR) { tb.add(BLK_ZERO, nbeta(model, F), 0); tb.add(BLK_ITEM, 4, q0 + qr_sigp_off(model, J, F)); }
        else tb.add(BLK_ITEM, nq(model, J, F), q0);
        tb.add(t.nu == NU_CELL ? BLK_CELL : BLK_SUBJECT, nu_len(model, N, J), SUBJ_NU);
    }
    return tb;
}
// columns of a trace: its blocks' -- and logLike's one, which is made of no block (a column of its own on the device)
constexpr int64_t trace_width(int model, int which, int64_t N, int J, int F) { return which == TRACE_LOGLIKE ? 1 : trace_blocks(model, which, N, J, F).width(); }
// the chain farm's summary vector: [item-level trace columns | theta (N) | zeta (N, response-time models) | nu (quantile models)]; an absent block's offset is -1
struct SummaryLayout { int64_t theta, zeta, nu, len; };
constexpr SummaryLayout summary_layout(int model, int64_t N, int J, int F)
{
    const int64_t wi = item_trace_width(model, J, F), nz = model_traits(model).rt ? N : 0, nn = nu_len(model, N, J);
    return {wi, nz > 0 ? wi + N : -1, nn > 0 ? wi + N + nz : -1, wi + N + nz + nn};
}

// The item-level fields of the parameter block (erm_layout.hpp: a, b, lambda, sig2t, rho : 5 x J), each with the erm_state member that carries it, its offset
// k * J and the constructors' value.  A template over the state struct: this header stays free of the C ABI's, the host side reads PAR_FIELDS<erm_state>.
enum ParFieldId : int { PAR_A = 0, PAR_B = 1, PAR_LAMBDA = 2, PAR_SIG2T = 3, PAR_RHO = 4, N_PAR_FIELDS = 5 };
template <typename State> struct ParField {
    const char* name; double* State::* member; int k; double init;
    constexpr int off(int J) const { return k * J; }
};
template <typename State> constexpr ParField<State> PAR_FIELDS[N_PAR_FIELDS] = {
    {"a", &State::a, PAR_A, 1.0}, {"b", &State::b, PAR_B, 0.0}, {"lambda", &State::lambda, PAR_LAMBDA, 0.0}, {"sig2t", &State::sig2t, PAR_SIG2T, 1.0}, {"rho", &State::rho, PAR_RHO, 0.0}};
// an item-trace row starts with the block's first fields at the same offsets: a, b, lambda, sig2t -- and rho, the head of the small part of qr, where the model has one
constexpr int item_trace_fields(int model) { return model_traits(model).rho ? N_PAR_FIELDS : PAR_RHO; }
// beta between its dense form (erm_state.beta = vec(beta) over F covariate columns; the item trace's small part of qr) and the block's [2 PMAX]: the dense entry that
// slot t of the block holds, -1 for none.  BETA_PAIR's two columns sit at [u] and [PMAX + u], BETA_ZERO_PAIR is never stored and reads as zeros, the others are copied.
constexpr int beta_slot_src(int shape, int F, int t)
{
    const int pp = F + 1;
    if (shape == BETA_PAIR) return t < pp ? t : (t >= PMAX && t < PMAX + pp) ? pp + t - PMAX : -1;
    return ((shape == BETA_VEC || shape == BETA_LATENT) && t < beta_len(shape, F)) ? t : -1;
}
inline void beta_pack(int shape, int F, const double* dense, double* block)
{
    for (int t = 0; t < 2 * PMAX; ++t) if (const int u = beta_slot_src(shape, F, t); u >= 0) block[t] = dense[u];
}
inline void beta_unpack(int shape, int F, const double* block, double* dense)
{
    for (int u = 0; u < beta_len(shape, F); ++u) dense[u] = 0.0;
    for (int t = 0; t < 2 * PMAX; ++t) if (const int u = beta_slot_src(shape, F, t); u >= 0) dense[u] = block[t];
}

// The layout change of an N x J block between the device (row-major, element (i, j) at [i * J + j]) and the caller (column-major, at [j * N + i]):
// dst = conv(src, j), converted to the destination's type.  rows_to_cols may scatter (element (i, j) at dst[(j * N + i) * dst_stride]: the Julia layout of
// a trace row); cols_to_rows stops at the first element `ok` refuses and returns false.
struct AsIs { template <typename T> T operator()(T v, int64_t) const { return v; } };
struct AnyValue { template <typename T> bool operator()(T) const { return true; } };
template <typename S, typename D, typename Conv = AsIs>
void rows_to_cols(const S* src, D* dst, int64_t N, int64_t J, Conv conv = Conv(), int64_t dst_stride = 1)
{
    for (int64_t j = 0; j < J; ++j) for (int64_t i = 0; i < N; ++i) dst[(size_t)(j * N + i) * (size_t)dst_stride] = (D)conv(src[(size_t)(i * J + j)], j);
}
template <typename S, typename D, typename Conv = AsIs, typename Ok = AnyValue>
bool cols_to_rows(const S* src, D* dst, int64_t N, int64_t J, Conv conv = Conv(), Ok ok = Ok())
{
    for (int64_t j = 0; j < J; ++j) for (int64_t i = 0; i < N; ++i) {
        const S v = src[(size_t)(j * N + i)];
        if (!ok(v)) return false;
        dst[(size_t)(i * J + j)] = (D)conv(v, j);
    }
    return true;
}

}  // namespace erm

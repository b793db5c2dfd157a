// tests/model_check.cpp -- the table of per-model facts (extendedrtirtmodeling.jl_amd/csrc/erm_model.hpp) on the CPU.
// Built by tests/test_model_traits.py with g++ -fsanitize=undefined -fno-sanitize-recover -ftrapv.  Prints, for every model and a grid of small (N, J, F), the
// traits and every width, length and offset derived from them as key=value pairs (one line per case), after checking the N x J layout helpers on the same grid.
// Each trace's blocks are printed as kind:ncol:col0:src:device_order joined by ';'.  The parameter block's field table, beta's packing and the offsets
// loglik_kernel reads from the table are checked here.
#include <cstdio>
#include <cstdint>
#include <string>
#include <vector>
#include "ertirt.h"
#include "erm_model.hpp"

using namespace erm;

static int fails = 0;
#define REQUIRE(cond, ...) do { if (!(cond)) { if (fails++ < 20) { fprintf(stderr, "FAIL %s: ", #cond); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); } } } while (0)

// rows_to_cols / cols_to_rows: every element lands where the other layout has it, the conversion sees the column, the scatter stride is honoured, the check stops the copy
static void check_layout(int64_t N, int64_t J)
{
    std::vector<float> rows((size_t)(N * J));
    for (int64_t i = 0; i < N; ++i) for (int64_t j = 0; j < J; ++j) rows[(size_t)(i * J + j)] = (float)(1 + i * J + j);
    std::vector<double> cols((size_t)(N * J), -1.0), wide((size_t)(3 * N * J), -1.0);
    rows_to_cols(rows.data(), cols.data(), N, J);
    rows_to_cols(rows.data(), wide.data(), N, J, [](float v, int64_t j) { return (double)v + 1000.0 * (double)j; }, 3);
    for (int64_t i = 0; i < N; ++i) for (int64_t j = 0; j < J; ++j) {
        REQUIRE(cols[(size_t)(j * N + i)] == (double)(1 + i * J + j), "rows_to_cols %lld x %lld at (%lld, %lld)", (long long)N, (long long)J, (long long)i, (long long)j);
        REQUIRE(wide[(size_t)(3 * (j * N + i))] == (double)(1 + i * J + j) + 1000.0 * (double)j, "strided rows_to_cols at (%lld, %lld)", (long long)i, (long long)j);
        REQUIRE(wide[(size_t)(3 * (j * N + i) + 1)] == -1.0 && wide[(size_t)(3 * (j * N + i) + 2)] == -1.0, "strided rows_to_cols wrote between its elements");
    }
    std::vector<float> back((size_t)(N * J), -1.f);
    REQUIRE(cols_to_rows(cols.data(), back.data(), N, J), "cols_to_rows refused without a check");
    REQUIRE(back == rows, "cols_to_rows does not invert rows_to_cols at %lld x %lld", (long long)N, (long long)J);
    cols[(size_t)(N * J - 1)] = 0.0;       // the last element the copy reaches
    REQUIRE(!cols_to_rows(cols.data(), back.data(), N, J, AsIs(), [](double v) { return v > 0.0; }), "cols_to_rows accepted a refused element");
}

static std::string blocks_str(int model, int which, int64_t N, int J, int F)
{
    std::string s;
    for (const TraceBlock& b : trace_blocks(model, which, N, J, F))
        s += (s.empty() ? "" : ";") + std::string(1, "SCIZ"[b.kind]) + ":" + std::to_string(b.ncol) + ":" + std::to_string(b.col0) + ":" + std::to_string(b.src) + ":" + (b.device_order() ? "1" : "0");
    return s.empty() ? "-" : s;
}

// the five item-level fields of the parameter block: erm_state's members of those names, at 0, J, 2J, 3J, 4J
static void check_fields()
{
    static const char* want[] = {"a", "b", "lambda", "sig2t", "rho"};
    double* erm_state::* const members[] = {&erm_state::a, &erm_state::b, &erm_state::lambda, &erm_state::sig2t, &erm_state::rho};
    REQUIRE(N_PAR_FIELDS == 5 && sizeof(PAR_FIELDS<erm_state>) / sizeof(PAR_FIELDS<erm_state>[0]) == 5, "five fields");
    for (int k = 0; k < 5; ++k) {
        const ParField<erm_state>& f = PAR_FIELDS<erm_state>[k];
        REQUIRE(std::string(f.name) == want[k] && f.member == members[k], "field %d is %s", k, f.name);
        for (int J : {1, 3, 7, 896}) REQUIRE(f.off(J) == k * J && f.off(J) + J <= par_off_sigp(J), "field %s at %d for J = %d", f.name, f.off(J), J);
    }
    REQUIRE(PAR_FIELDS<erm_state>[PAR_SIG2T].name == std::string("sig2t") && PAR_FIELDS<erm_state>[PAR_SIG2T].init == 1.0 && PAR_FIELDS<erm_state>[PAR_A].init == 1.0, "sig2t, a start at 1");
    REQUIRE(item_trace_fields(CROSS) == 5 && item_trace_fields(CROSSQR) == 5 && item_trace_fields(RTIRT) == 4 && item_trace_fields(MLIRT) == 4, "rho heads the small part of qr of the Cross family alone");
}

// beta: pack then unpack is the identity for the stored shapes and gives zeros for BETA_ZERO_PAIR, nothing lands outside the slots the kernels read, and an unpacked
// block that was never packed into (BETA_ZERO_PAIR) stays untouched
static void check_beta(int shape, int F)
{
    const int n = beta_len(shape, F);
    std::vector<double> dense((size_t)n), back((size_t)n, -7.0), block(2 * PMAX, -1.0);
    for (int u = 0; u < n; ++u) dense[(size_t)u] = 0.5 + u;
    beta_pack(shape, F, dense.data(), block.data());
    beta_unpack(shape, F, block.data(), back.data());
    int stored = 0;
    for (int t = 0; t < 2 * PMAX; ++t) stored += block[(size_t)t] != -1.0;
    if (shape == BETA_ZERO_PAIR) {
        REQUIRE(stored == 0, "BETA_ZERO_PAIR stored %d entries", stored);
        for (int u = 0; u < n; ++u) REQUIRE(back[(size_t)u] == 0.0, "BETA_ZERO_PAIR reads %g at %d", back[(size_t)u], u);
        return;
    }
    REQUIRE(stored == n && back == dense, "beta shape %d over F = %d: %d of %d entries stored, round trip %s", shape, F, stored, n, back == dense ? "ok" : "differs");
    if (shape == BETA_PAIR) for (int u = 0; u <= F; ++u) REQUIRE(block[(size_t)u] == dense[(size_t)u] && block[(size_t)(PMAX + u)] == dense[(size_t)(F + 1 + u)], "BETA_PAIR column entry %d", u);
    else for (int u = 0; u < n; ++u) REQUIRE(block[(size_t)u] == dense[(size_t)u], "copied shape %d entry %d", shape, u);
}

// loglik_kernel (erm_kernels.hpp) receives F = kernel_feat(model, nFeat) and reads Sigp at qr_sigp_off(model, J, F) and beta's slots from beta_slot_src: both equal
// the expressions the kernel used to spell out, for every model with a Sigp / a beta (the others take the kernel's constant branch on both sides)
static void check_loglik_offsets(int M, int J, int nFeat)
{
    const int F = kernel_feat(M, nFeat), p = F + 1;
    const int old_sigp = fam_cq(M) ? J : (fam_rt(M) ? 2 * p : p + 1);
    REQUIRE((M == MLIRT) == !model_traits(M).rt, "the model without Sigp is MlIrt");
    if (M != MLIRT) REQUIRE(qr_sigp_off(M, J, F) == old_sigp, "Sigp offset of model %d: %d, was %d", M, qr_sigp_off(M, J, F), old_sigp);
    REQUIRE(fam_cq(M) == model_traits(M).rho, "rho of model %d", M);
    for (int tid = 0; tid < 2 * PMAX; ++tid) {
        int old_src = -1;
        if (M == MLIRT) { if (tid < p) old_src = tid; }
        else if (M == RTIRT) { if (tid < p) old_src = tid; else if (tid >= PMAX && tid < PMAX + p) old_src = p + tid - PMAX; }
        else if (fam_lq(M)) { if (tid < p + 1) old_src = tid; }
        REQUIRE(beta_slot_src(model_traits(M).beta, F, tid) == old_src, "beta slot %d of model %d at F = %d", tid, M, F);
    }
}

int main()
{
    static const char* nu_name[] = {"none", "subject", "cell"};
    static const char* beta_name[] = {"none", "vec", "pair", "latent", "zero_pair"};
    static const long long Ns[] = {1, 2, 5, 160};
    static const int Js[] = {1, 3, 7}, Fs[] = {0, 2, 3};
    for (long long N : Ns) for (int J : Js) check_layout(N, J);
    for (int model = MLIRT; model <= LATENT; ++model)
        for (long long N : Ns) for (int J : Js) for (int F : Fs) {
            const ModelTraits t = model_traits(model);
            const SummaryLayout s = summary_layout(model, N, J, F);
            printf("model=%d N=%lld J=%d F=%d rt=%d rho=%d nu=%s sees_x=%d beta=%s gen=%d kernel_feat=%d nbeta=%d nq=%d sigp_off=%d qr_head=%d item=%lld nu_len=%lld "
                   "ra=%lld rtw=%lld qr=%lld ll=%lld sum_theta=%lld sum_zeta=%lld sum_nu=%lld sum_len=%lld blocks_ra=%s blocks_rt=%s blocks_qr=%s blocks_ll=%s\n",
                   model, N, J, F, (int)t.rt, (int)t.rho, nu_name[t.nu], (int)t.sees_x, beta_name[t.beta], t.gen, kernel_feat(model, F), nbeta(model, F), nq(model, J, F),
                   qr_sigp_off(model, J, F), qr_head(model, J, F), (long long)item_trace_width(model, J, F), (long long)nu_len(model, N, J),
                   (long long)trace_width(model, TRACE_RA, N, J, F), (long long)trace_width(model, TRACE_RT, N, J, F), (long long)trace_width(model, TRACE_QR, N, J, F),
                   (long long)trace_width(model, TRACE_LOGLIKE, N, J, F), (long long)s.theta, (long long)s.zeta, (long long)s.nu, (long long)s.len,
                   blocks_str(model, TRACE_RA, N, J, F).c_str(), blocks_str(model, TRACE_RT, N, J, F).c_str(), blocks_str(model, TRACE_QR, N, J, F).c_str(), blocks_str(model, TRACE_LOGLIKE, N, J, F).c_str());
            check_loglik_offsets(model, J, F);
        }
    check_fields();
    for (int shape = BETA_NONE; shape <= BETA_ZERO_PAIR; ++shape) for (int F : {0, 2, 3, PMAX - 2}) check_beta(shape, F);
    // beyond the models and the traces: nothing, not a crash (Engine::init looks the table up ahead of its range check)
    REQUIRE(!model_traits(-1).rt && !model_traits(7).sees_x && nbeta(7, 3) == 0 && nu_len(-1, 5, 3) == 0 && trace_width(RTIRT, 4, 5, 3, 2) == 0 && trace_width(RTIRT, -1, 5, 3, 2) == 0, "out of range");
    // the engine's limits do not overflow: 2^32 - 1 subjects, 896 items
    REQUIRE(summary_layout(CROSSQR, 4294967295LL, MAX_ITEMS, PMAX - 2).len == 4 * 896 + 900 + 2 * 4294967295LL + 896 * 4294967295LL, "summary length at the limits");
    fprintf(stderr, "layout and range failures %d\n", fails);
    return fails ? 1 : 0;
}

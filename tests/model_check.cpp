// tests/model_check.cpp -- the table of per-model facts (extendedrtirtmodeling.jl_amd/csrc/erm_model.hpp) on the CPU.
// Built by tests/test_model_traits.py with g++ -fsanitize=undefined -fno-sanitize-recover -ftrapv.  Prints, for every model and a grid of small (N, J, F), the
// traits and every width, length and offset derived from them as key=value pairs (one line per case), after checking the N x J layout helpers on the same grid.
#include <cstdio>
#include <cstdint>
#include <vector>
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
                   "ra=%lld rtw=%lld qr=%lld ll=%lld sum_theta=%lld sum_zeta=%lld sum_nu=%lld sum_len=%lld\n",
                   model, N, J, F, (int)t.rt, (int)t.rho, nu_name[t.nu], (int)t.sees_x, beta_name[t.beta], t.gen, kernel_feat(model, F), nbeta(model, F), nq(model, J, F),
                   qr_sigp_off(model, J, F), qr_head(model, J, F), (long long)item_trace_width(model, J, F), (long long)nu_len(model, N, J),
                   (long long)trace_width(model, TRACE_RA, N, J, F), (long long)trace_width(model, TRACE_RT, N, J, F), (long long)trace_width(model, TRACE_QR, N, J, F),
                   (long long)trace_width(model, TRACE_LOGLIKE, N, J, F), (long long)s.theta, (long long)s.zeta, (long long)s.nu, (long long)s.len);
        }
    // beyond the models and the traces: nothing, not a crash (Engine::init looks the table up ahead of its range check)
    REQUIRE(!model_traits(-1).rt && !model_traits(7).sees_x && nbeta(7, 3) == 0 && nu_len(-1, 5, 3) == 0 && trace_width(RTIRT, 4, 5, 3, 2) == 0 && trace_width(RTIRT, -1, 5, 3, 2) == 0, "out of range");
    // the engine's limits do not overflow: 2^32 - 1 subjects, 896 items
    REQUIRE(summary_layout(CROSSQR, 4294967295LL, MAX_ITEMS, PMAX - 2).len == 4 * 896 + 900 + 2 * 4294967295LL + 896 * 4294967295LL, "summary length at the limits");
    fprintf(stderr, "layout and range failures %d\n", fails);
    return fails ? 1 : 0;
}

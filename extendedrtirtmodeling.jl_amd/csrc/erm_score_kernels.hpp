// erm_score_kernels.hpp -- the scores of respondents on the device: every subject's posterior mean and sd of theta and zeta, their covariance and
// the rows' effective size (erm_score.hpp), over a table of item-trace rows.  Include after erm_marginal_kernels.hpp.
//
// score_kernel<MODEL, real, WEIGHTED> has marginal_kernel's geometry and shares its row staging, law, item sums and node loop (marg_stage, marg_stage_law,
// marg_item_sums, marg_lane_nodes): eight lanes per subject, 32 subjects per workgroup of 256 threads taken through all rows, the LDS double buffer of rows, node
// chunks of eight, fixed butterflies.  What differs:
//   3. nodes       each node's (e_q, z_q) enters the lane's ScoreMS -- M and S as in marginal_kernel, and the two sums behind the row's mean and variance of theta:
//                  two multiply-adds per node beside J evaluations of log(1 + e^eta); a fixed butterfly of score_ms_merge joins the eight lanes.
//   4. accumulate  the row's moments (score_row, with the zeta conditional of score_zeta from the item sums the lanes already hold) enter the subject's ScoreAcc --
//                  eleven doubles in registers from the first row to the last; WEIGHTED chooses omega_s = exp(l_s - Lambda) over omega_s = 1.
// One store of seven doubles per subject at the end.  Plain vector loads and stores, no atomics: every output word has one writer.
// MASKED: incomplete response patterns, as marginal_kernel's -- the subject's list of observed cells through the same helpers.
#pragma once
#include "erm_marginal_kernels.hpp"
#include "erm_score.hpp"

namespace erm {

// A: marginal_kernel's arguments (l_out, acc_ms, acc_w unused; coarse [N] receives the flags marginal_count_kernel adds); score: column-major [N][SCORE_COLS]
template <int MODEL, typename real, bool WEIGHTED, bool MASKED = false>
__global__ void __launch_bounds__(256) score_kernel(const MargArgs A, double* __restrict__ score)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    double* sh = reinterpret_cast<double*>(smem);
    constexpr bool RT = MODEL != MLIRT;
    const int J = A.J, F = A.F, Q = A.Q, tid = (int)threadIdx.x;
    const long long half = marg_row_lds(A.ld, J);
    const int s = tid & (MARG_LANES - 1), r = tid >> MARG_LOG_LANES;
    const long long i0 = (long long)blockIdx.x * MARG_TILE;
    const bool ok = i0 + r < A.N;
    const long long i = ok ? i0 + r : A.N - 1;            // idle lanes repeat the last subject: every lane takes part in the butterflies and the barriers
    int n;
    const size_t at = marg_cells<MASKED>(A, i, n);
    const uint8_t* Yi = A.Y + at;
    const real* Ci = RT ? reinterpret_cast<const real*>(A.C) + at : nullptr;
    const unsigned short* Ii = MASKED ? A.idx + at : nullptr;
    double x[MARG_MAXF];
    marg_load_x<MODEL, real>(A, i, x);
    marg_stage<MODEL>(A, 0, sh, tid);
    __syncthreads();

    const double h = marg_step(Q), log_h = log(h);
    ScoreAcc acc{0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    bool coarse = false;
    for (long long row = 0; row < A.n_rows; ++row) {
        const double* sa = sh + (row & 1) * half;
        if (row + 1 < A.n_rows) marg_stage<MODEL>(A, row + 1, sh + ((row + 1) & 1) * half, tid);
        const MargLaw w = marg_stage_law<MODEL>(sa, J, F, x);
        MargSums ms;
        double A1, A0;
        marg_item_sums<MODEL, real, MASKED>(A, sa, Yi, Ci, s, ms, A1, A0, Ii, n);
        ScoreMS part{0.0, 0.0, 0.0, 0.0};
        marg_lane_nodes<MODEL, MASKED>(sa, J, Q, s, h, log_h, w, ms, A1, A0, [&](double e, double z) { score_ms_add(part, e, z); }, 0.0, Ii, n);
        for (int m = 1; m < MARG_LANES; m <<= 1) {
            const ScoreMS o{__shfl_xor(part.M, m, 64), __shfl_xor(part.S, m, 64), __shfl_xor(part.S1, m, 64), __shfl_xor(part.S2, m, 64)};
            part = score_ms_merge(part, o);
        }
        coarse = coarse || part.S < MARG_COARSE_S;
        score_acc_add(acc, score_row(part, w, score_zeta(ms, w)), WEIGHTED);
        __syncthreads();                                  // the next row is staged; this row's half is free for the one after
    }
    if (ok && s == 0) {
        double out[SCORE_COLS];
        score_finish(acc, RT, out);
        out[SCORE_COARSE] = coarse ? 1.0 : 0.0;
#pragma unroll
        for (int c = 0; c < SCORE_COLS; ++c) score[(size_t)c * A.N + i] = out[c];
        A.coarse[i] = coarse ? 1u : 0u;
    }
}

}  // namespace erm

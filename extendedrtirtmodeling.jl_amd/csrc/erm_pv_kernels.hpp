// erm_pv_kernels.hpp -- plausible values on the device: K draws of (theta_i, zeta_i) from every subject's posterior (erm_pv.hpp), over a table of
// item-trace rows.  Include after erm_score_kernels.hpp and erm_rng.hpp (philox4x32_10).
//
// pv_kernel<MODEL, real> has score_kernel's geometry and shares its row staging, law, item sums and node loop (marg_stage, marg_stage_law, marg_item_sums,
// marg_lane_nodes): eight lanes per subject, 32 subjects per workgroup of 256 threads, the LDS double buffer of rows, node chunks of eight, fixed butterflies.
// The loop runs over the draws, not the rows.  Per draw k:
//   1. staging     the row of draw k + 1, r_{k+1} = pv_row(k + 1), is copied into the other half of the LDS buffer before this draw's arithmetic starts; one barrier
//                  per draw.  K and n_rows are the launch's, so every subject of the workgroup is at the same row and every lane reads the same a_j, b_j: LDS
//                  broadcasts, as in score_kernel.  Draws that share a row (K > n_rows) each take their own node pass: the keys differ from draw to draw, and the
//                  usual request (five draws from hundreds of rows) shares none.
//   2. item sums   as score_kernel.
//   3. nodes       each node's (e_q, z_q, q) enters the lane's ScoreMS -- M, S and the two sums behind the row's E and V -- and, with one Philox block at
//                  {i, k, q}, the lane's best (key, q); fixed butterflies of score_ms_merge and pv_best_merge join the eight lanes (both merges are symmetric,
//                  so all eight hold the same result).  One block of ten rounds beside J evaluations of log(1 + e^eta) per node.
//   4. finish      lane 0 draws the finishing block at {i, k, 0xFFFFFFFF} and stores theta, zeta and q* (pv_finish).
// The subject index in the counter is i_base + the index within the launch: a chunk of a larger data set draws what the whole would.  Plain vector loads and
// stores, no atomics: every output word has one writer.
// MASKED: incomplete response patterns, as marginal_kernel's -- the subject's list of observed cells through the same helpers; the counters are unchanged.
#pragma once
#include "erm_score_kernels.hpp"
#include "erm_pv.hpp"

namespace erm {

struct PvArgs {
    long long K;                  // draws per subject
    unsigned long long seed;
    long long i_base;             // the data-set index of the launch's subject 0
    double* pv;                   // [2][K][N]: theta block, zeta block, the subject fastest (N = the launch's subjects)
    int* node;                    // [K][N] or nullptr
};

// A: marginal_kernel's arguments (l_out, acc_ms, acc_w unused; coarse [N] receives the flags: S < MARG_COARSE_S at a row the subject used)
template <int MODEL, typename real, bool MASKED = false>
__global__ void __launch_bounds__(256) pv_kernel(const MargArgs A, const PvArgs P)
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
    marg_stage<MODEL>(A, pv_row(0, P.K, A.n_rows), sh, tid);
    __syncthreads();

    const double h = marg_step(Q), log_h = log(h);
    const uint32_t k0 = (uint32_t)P.seed, k1 = (uint32_t)(P.seed >> 32), ci = (uint32_t)(P.i_base + i), c3 = PV_SITE << 24;
    bool coarse = false;
    for (long long k = 0; k < P.K; ++k) {
        const double* sa = sh + (k & 1) * half;
        if (k + 1 < P.K) marg_stage<MODEL>(A, pv_row(k + 1, P.K, A.n_rows), sh + ((k + 1) & 1) * half, tid);
        const MargLaw w = marg_stage_law<MODEL>(sa, J, F, x);
        MargSums ms;
        double A1, A0;
        marg_item_sums<MODEL, real, MASKED>(A, sa, Yi, Ci, s, ms, A1, A0, Ii, n);
        ScoreMS part{0.0, 0.0, 0.0, 0.0};
        PvBest best{0.0, -1};
        marg_lane_nodes<MODEL, MASKED>(sa, J, Q, s, h, log_h, w, ms, A1, A0, [&](double e, double z, int q) {
            score_ms_add(part, e, z);
            uint32_t w0, w1, w2, w3;
            philox4x32_10(ci, (uint32_t)k, (uint32_t)q, c3, k0, k1, w0, w1, w2, w3);
            pv_best_add(best, e + pv_gumbel(w0), q);
        }, 0.0, Ii, n);
        for (int m = 1; m < MARG_LANES; m <<= 1) {
            const ScoreMS o{__shfl_xor(part.M, m, 64), __shfl_xor(part.S, m, 64), __shfl_xor(part.S1, m, 64), __shfl_xor(part.S2, m, 64)};
            part = score_ms_merge(part, o);
            const PvBest b{__shfl_xor(best.key, m, 64), __shfl_xor(best.q, m, 64)};
            best = pv_best_merge(best, b);
        }
        coarse = coarse || part.S < MARG_COARSE_S;
        if (ok && s == 0) {
            uint32_t w0, w1, w2, w3;
            philox4x32_10(ci, (uint32_t)k, PV_FINISH_CTR, c3, k0, k1, w0, w1, w2, w3);
            const ScoreZeta kz = score_zeta(ms, w);
            const PvDraw d = pv_finish(score_row(part, w, kz), w, kz, best.q, h, RT, w0, w1, w2);
            P.pv[(size_t)k * A.N + i] = d.theta;
            P.pv[(size_t)(P.K + k) * A.N + i] = d.zeta;
            if (P.node) P.node[(size_t)k * A.N + i] = best.q;
        }
        __syncthreads();                                  // the next draw's row is staged; this draw's half is free for the one after
    }
    if (ok && s == 0) A.coarse[i] = coarse ? 1u : 0u;
}

}  // namespace erm

// erm_fit_kernels.hpp -- person fit on the device: every subject's lz, its normal p-value, the Wilson-Hilferty z of the response-time quadratic form,
// its exact chi^2 p-value and the rows' effective size (erm_fit.hpp), over a table of item-trace rows.  Include after erm_score_kernels.hpp.
//
// fit_kernel<MODEL, real, WEIGHTED, MASKED> has score_kernel's geometry and shares its row staging, law and item sums (marg_cells, marg_load_x, marg_stage,
// marg_stage_law, marg_item_sums, as they are): eight lanes per subject, 32 subjects per workgroup of 256 threads taken through all rows, the LDS double buffer of
// rows, fixed butterflies.  Deterministic: no random numbers.  What differs:
//   3. nodes       fit_lane_nodes deals the nodes s, s + 8, ... to lane s in rising order as marg_lane_nodes does, in chunks of FIT_CHUNK, so (M, S) are
//                  marginal_kernel's whatever the chunk.  Every chain carries three accumulators (lse, W, Vw) from one exp per cell-node (fit_cell); y_j is read
//                  beside (a_j, b_j) once per item per chunk -- the eight lanes of a subject read the same byte.  After the items: Qf, its chi^2 tail for the chunk's
//                  nodes together (one reciprocal per term serves them all) and its Wilson-Hilferty z.  Each node's (e_q, lz, Phi(lz), ltz, tail) enters the
//                  lane's FitMS; a fixed butterfly of fit_ms_merge joins the eight lanes.
//   4. accumulate  the row's four weighted means (fit_row) enter the subject's FitAcc -- seven doubles in registers from the first row to the last.
// One store of six doubles per subject at the end.  Plain vector loads and stores, no atomics: every output word has one writer.
// MASKED: incomplete response patterns, as score_kernel's.  The loops over the subject's cells and over the tail's n_i / 2 terms have the subject's
// own trip count; every butterfly and barrier stands outside them.
#pragma once
#include "erm_score_kernels.hpp"
#include "erm_fit.hpp"

namespace erm {

// Three accumulators per chain: with eight chains 24 of the 30 instances spill 32 .. 38 VGPRs to scratch at two waves per SIMD; with four every instance fits in
// 189 .. 254 VGPRs without scratch.  What keeps the four inside 256 registers: the covariates are loaded again at every row instead of being held
// across the nodes (fit_kernel), the sums of g_j * 0 of the models without rho are said to be 0, and the special functions after the cell loop are laid down once
// (fit_lane_nodes).  __launch_bounds__(256, 2) holds the compiler to the two waves.
constexpr int FIT_CHUNK = 4;

// a[0] leaves, the others move down by one, `last` enters at the end
__device__ __forceinline__ void fit_rotate(double (&a)[FIT_CHUNK], double last)
{
#pragma unroll
    for (int c = 0; c + 1 < FIT_CHUNK; ++c) a[c] = a[c + 1];
    a[FIT_CHUNK - 1] = last;
}

// nodes: lane s, nodes s, s + 8, ... in chunks of FIT_CHUNK; sink(e_q, lz, Phi(lz), ltz, tail) receives the lane's nodes in order.  Yi: the subject's responses,
// by item -- MASKED: by list position, beside Ii, the list of its n items, rising.  Nothing inside crosses lanes.
template <int MODEL, bool MASKED, typename Sink>
__device__ __forceinline__ void fit_lane_nodes(const double* sa, int J, int Q, int s, double h, double log_h, const MargLaw& w, const MargSums& ms, double A1, double A0,
                                               const uint8_t* Yi, const unsigned short* Ii, int n, Sink&& sink)
{
    constexpr bool RT = MODEL != MLIRT;
    for (int q0 = s; q0 < Q; q0 += MARG_LANES * FIT_CHUNK) {
        double th[FIT_CHUNK], lse[FIT_CHUNK], W[FIT_CHUNK], Vw[FIT_CHUNK];
#pragma unroll
        for (int c = 0; c < FIT_CHUNK; ++c) {
            const int qq = q0 + c * MARG_LANES;
            th[c] = w.mu + w.sd * marg_node(qq < Q ? qq : Q - 1, h);      // (a slot past the last node repeats it and is dropped below)
            lse[c] = 0.0; W[c] = 0.0; Vw[c] = 0.0;
        }
        for (int k = 0; k < n; ++k) {
            const int j = MASKED ? (int)Ii[k] : k;
            const double a = sa[j], b = sa[J + j];
            const bool y = Yi[k] != 0;
#pragma unroll
            for (int c = 0; c < FIT_CHUNK; ++c) fit_cell(a * (th[c] - b), y, lse[c], W[c], Vw[c]);
        }
        // The special functions behind a node's values (erfc twice, exp, cbrt, log1p) are laid down ONCE: these loops are not unrolled, the chain in turn
        // stands in slot 0 and the arrays rotate by one per trip, so that after FIT_CHUNK trips they stand as they stood.  (Unrolled, the four copies cost some
        // sixty registers more than the cell loop, and the kernel loses its second wave per SIMD.)
        double y[FIT_CHUNK], t[FIT_CHUNK], tail[FIT_CHUNK];
#pragma unroll
        for (int c = 0; c < FIT_CHUNK; ++c) { y[c] = 0.0; t[c] = 0.0; tail[c] = 0.0; }
        if constexpr (RT) {
#pragma nounroll
            for (int c = 0; c < FIT_CHUNK; ++c) {
                double y0, t0;
                const double base0 = fit_tail_start(fit_rt_quad(ms, w, th[0]), n, y0, t0);
                fit_rotate(th, th[0]); fit_rotate(y, y0); fit_rotate(t, t0); fit_rotate(tail, base0);
            }
            fit_tail_sum<FIT_CHUNK>(y, t, n, tail);       // the terms of the four tails together: one reciprocal per term
        }
#pragma nounroll
        for (int c = 0; c < FIT_CHUNK; ++c) {
            const int qq = q0 + c * MARG_LANES;
            if (qq < Q) {
                const double z = marg_node(qq, h);
                double e = marg_log_weight(z, log_h) + (th[0] * A1 - A0 - lse[0]);
                if constexpr (RT) e += marg_T(ms, n, w, th[0]);
                const double lz = fit_lz(W[0], Vw[0]);
                if constexpr (RT) sink(e, lz, fit_phi(lz), fit_wh(fit_rt_quad(ms, w, th[0]), n), tail[0]);
                else sink(e, lz, fit_phi(lz), 0.0, 0.0);
            }
            fit_rotate(th, th[0]); fit_rotate(lse, lse[0]); fit_rotate(W, W[0]); fit_rotate(Vw, Vw[0]); fit_rotate(tail, tail[0]);
        }
    }
}

// A: marginal_kernel's arguments (l_out, acc_ms, acc_w unused; coarse [N] receives the flags marginal_count_kernel adds); fit: column-major [N][FIT_COLS]
template <int MODEL, typename real, bool WEIGHTED, bool MASKED = false>
__global__ void __launch_bounds__(256, 2) fit_kernel(const MargArgs A, double* __restrict__ fit)
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
    marg_stage<MODEL>(A, 0, sh, tid);
    __syncthreads();

    const double h = marg_step(Q), log_h = log(h);
    FitAcc acc{0.0, 0.0, 0.0, {0.0, 0.0, 0.0, 0.0}};
    bool coarse = false;
    for (long long row = 0; row < A.n_rows; ++row) {
        const double* sa = sh + (row & 1) * half;
        if (row + 1 < A.n_rows) marg_stage<MODEL>(A, row + 1, sh + ((row + 1) & 1) * half, tid);
        double x[MARG_MAXF];
        marg_load_x<MODEL, real>(A, i, x);
        const MargLaw w = marg_stage_law<MODEL>(sa, J, F, x);
        MargSums ms;
        double A1, A0;
        marg_item_sums<MODEL, real, MASKED>(A, sa, Yi, Ci, s, ms, A1, A0, Ii, n);
        if constexpr (!model_traits(MODEL).rho) { ms.R1 = 0.0; ms.D1 = 0.0; ms.D2 = 0.0; }      // sums of g_j * 0: said so, they hold no registers across the nodes
        FitMS part{0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        fit_lane_nodes<MODEL, MASKED>(sa, J, Q, s, h, log_h, w, ms, A1, A0, Yi, Ii, n,
                                      [&](double e, double lz, double py, double ltz, double pt) { fit_ms_add(part, e, lz, py, ltz, pt); });
        for (int m = 1; m < MARG_LANES; m <<= 1) {
            const FitMS o{__shfl_xor(part.M, m, 64), __shfl_xor(part.S, m, 64), __shfl_xor(part.LZ, m, 64), __shfl_xor(part.PY, m, 64), __shfl_xor(part.LTZ, m, 64),
                          __shfl_xor(part.PT, m, 64)};
            part = fit_ms_merge(part, o);
        }
        coarse = coarse || part.S < MARG_COARSE_S;
        fit_acc_add(acc, fit_row(part), WEIGHTED);
        __syncthreads();                                  // the next row is staged; this row's half is free for the one after
    }
    if (ok && s == 0) {
        double out[FIT_COLS];
        fit_finish(acc, RT, n, out);
        out[FIT_COARSE] = coarse ? 1.0 : 0.0;
#pragma unroll
        for (int c = 0; c < FIT_COLS; ++c) fit[(size_t)c * A.N + i] = out[c];
        A.coarse[i] = coarse ? 1u : 0u;
    }
}

}  // namespace erm

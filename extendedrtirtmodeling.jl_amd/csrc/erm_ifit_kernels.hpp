// erm_ifit_kernels.hpp -- item fit and drift on the device: every item's infit, outfit, signed response residual, response-time mean square and
// signed response-time residual (erm_ifit.hpp), over a table of item-trace rows.  Include after erm_fit_kernels.hpp.
//
// item_fit_kernel<MODEL, real, MASKED> has fit_kernel's geometry and shares its row staging, law and item sums (marg_cells, marg_load_x, marg_stage,
// marg_stage_law, marg_item_sums, as they are): eight lanes per subject, 32 subjects per workgroup of 256 threads taken through all rows, the LDS double buffer of
// rows, fixed butterflies.  Deterministic: no random numbers.  Per row:
//   pass 1   marg_lane_nodes, as it is: the row's (M, S) with marginal_kernel's bits.  Each lane parks its own nodes' e_q in a lane-private global scratch -- lane s
//            of the r-th subject of workgroup g owns the words s, s + 8, ... of eq[(32 g + r) Q ..]: the only writer, and the thread that reads them again (an idle
//            lane that repeats the last subject has a slot of its own).  After the butterfly each lane turns its e_q into w_q = exp(e_q - M) / S in place.
//   pass 2   cells outside, the lane's nodes inside: for cell k the lane adds the six w_q-weighted values of ifit_resp / ifit_rt_d over its nodes, one exp per
//            cell-node; what does not depend on the node (1 / Pi, the residual's scale) is laid down once per cell.  A 3-step butterfly joins the eight lanes, and
//            lane c < 6 of the subject adds value c into the cell's word c of the dense, zero-filled workspace ws[subject][item][6].  Across the rows a word is
//            read and written by that one thread only.  Idle lanes write nothing.
// MASKED walks the subject's observed list and writes at the item's dense index.  The cell loop of pass 2 holds a butterfly, so its trip count is
// the largest n_i of the wave (one butterfly before the rows) with the cell's work under k < n_i: every butterfly and barrier stands outside the loops whose
// length depends on n_i.  Plain vector loads and stores, no atomics: every word has one writer.
//
// item_fit_block_kernel (stage A): for item j and block b of 256 consecutive subjects, the six sums and the count of the subjects that observed j, by
// ifit_tree_sum's fixed tree; absent subjects and unobserved cells count 0.  item_fit_finish_kernel (stage B): per item, the block sums in rising block order in
// one thread, the division by the number of rows, and ifit_finish.  The block sums outlive the chunks, so the result does not depend on the chunking by a bit.
#pragma once
#include "erm_fit_kernels.hpp"
#include "erm_ifit.hpp"

namespace erm {

// A: marginal_kernel's arguments for the chunk's subjects (l_out, acc_ms, acc_w unused; coarse [N] receives the flags);
// eq: [32 * gridDim.x][Q]; ws: [A.N][J][IFIT_VALS], zero on entry
template <int MODEL, typename real, bool MASKED = false>
__global__ void __launch_bounds__(256, 2) item_fit_kernel(const MargArgs A, double* __restrict__ eq, double* __restrict__ ws)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    double* sh = reinterpret_cast<double*>(smem);
    constexpr bool RT = MODEL != MLIRT;
    constexpr ModelTraits MT = model_traits(MODEL);
    constexpr int VALS = RT ? IFIT_VALS : IFIT_D;         // the values a model has: without times the words of d and d^2 stay 0
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
    double* wq = eq + (size_t)(i0 + r) * Q;               // the slot of this group of eight lanes, idle or not
    double* wi = ws + (size_t)i * J * IFIT_VALS;
    int nmax = n;                                         // the cell loop's trip count: the wave's largest
    if constexpr (MASKED) for (int m = MARG_LANES; m < 64; m <<= 1) nmax = max(nmax, __shfl_xor(nmax, m, 64));
    marg_stage<MODEL>(A, 0, sh, tid);
    __syncthreads();

    const double h = marg_step(Q), log_h = log(h);
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
        // ---- pass 1: (M, S), the lane's e_q parked
        MargMS part{0.0, 0.0};
        marg_lane_nodes<MODEL, MASKED>(sa, J, Q, s, h, log_h, w, ms, A1, A0, [&](double e, double, int q) { marg_ms_add(part, e); wq[q] = e; }, 0.0, Ii, n);
        for (int m = 1; m < MARG_LANES; m <<= 1) {
            const MargMS o{__shfl_xor(part.M, m, 64), __shfl_xor(part.S, m, 64)};
            part = marg_ms_merge(part, o);
        }
        coarse = coarse || part.S < MARG_COARSE_S;
        for (int q = s; q < Q; q += MARG_LANES) wq[q] = exp(wq[q] - part.M) / part.S;
        // ---- pass 2: the cells
        const double* qr = sa + 4 * J;
        for (int k = 0; k < nmax; ++k) {
            double acc[IFIT_VALS] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
            const bool mine = k < n;
            const int j = !mine ? 0 : MASKED ? (int)Ii[k] : k;
            if (mine) {
                const double a = sa[j], b = sa[J + j];
                const bool y = Yi[k] != 0;
                IfitRt cell{0.0, 0.0, 0.0, 0.0, 0.0};
                if constexpr (RT) {
                    const double t = (double)Ci[k] + (A.cm ? A.cm[j] : 0.0);
                    cell = ifit_rt_prep(sa[A.ld + j], sa[3 * J + j], sa[2 * J + j] - t, MT.rho ? qr[j] : 0.0, ms.P, w.v);
                }
                for (int q = s; q < Q; q += MARG_LANES) {
                    const double wt = wq[q], th = w.mu + w.sd * marg_node(q, h);
                    double e, r2, c, z2;
                    ifit_resp(a * (th - b), y, e, r2, c, z2);
                    acc[IFIT_E] += wt * e; acc[IFIT_R2] += wt * r2; acc[IFIT_C] += wt * c; acc[IFIT_Z2] += wt * z2;
                    if constexpr (RT) {
                        const double d = ifit_rt_d(cell, w.v, ms.R0 - th * (MT.rho ? ms.R1 : 0.0), w.m0 + w.m1 * th, th);
                        acc[IFIT_D] += wt * d; acc[IFIT_D2] += wt * (d * d);
                    }
                }
            }
            for (int m = 1; m < MARG_LANES; m <<= 1) {
#pragma unroll
                for (int c = 0; c < VALS; ++c) acc[c] += __shfl_xor(acc[c], m, 64);
            }
            double mine_v = acc[0];
#pragma unroll
            for (int c = 1; c < VALS; ++c) mine_v = s == c ? acc[c] : mine_v;
            if (ok && mine && s < VALS) wi[(size_t)j * IFIT_VALS + s] += mine_v;
        }
        __syncthreads();                                  // the next row is staged; this row's half is free for the one after
    }
    if (ok && s == 0 && A.coarse) A.coarse[i] = coarse ? 1u : 0u;
}

// stage A.  grid (blocks of the chunk, items); ws: the chunk's workspace [nc][J][IFIT_VALS]; off / idx: the chunk's observed lists (off[il] .. off[il + 1] of idx,
// rising in the item) or NULL for complete data; blk: [blocks of the chunk][J][IFIT_SUMS], the chunk's part of the table of block sums
__global__ void __launch_bounds__(IFIT_BLOCK) item_fit_block_kernel(const double* __restrict__ ws, long long nc, int J, const long long* __restrict__ off,
                                                                     const unsigned short* __restrict__ idx, double* __restrict__ blk)
{
    __shared__ double sh[IFIT_SUMS][IFIT_BLOCK];
    const int t = (int)threadIdx.x, j = (int)blockIdx.y;
    const long long b = blockIdx.x, il = b * IFIT_BLOCK + t;
    double v[IFIT_SUMS] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (il < nc) {
        bool seen = true;
        if (off) {                                        // is j on the subject's list?  a bisection over its rising items
            long long lo = off[il], hi = off[il + 1];
            while (lo < hi) { const long long mid = lo + ((hi - lo) >> 1); if ((int)idx[mid] < j) lo = mid + 1; else hi = mid; }
            seen = lo < off[il + 1] && (int)idx[lo] == j;
        }
        if (seen) {
            const double* cell = ws + ((size_t)il * J + j) * IFIT_VALS;
#pragma unroll
            for (int c = 0; c < IFIT_VALS; ++c) v[c] = cell[c];
            v[IFIT_VALS] = 1.0;
        }
    }
#pragma unroll
    for (int c = 0; c < IFIT_SUMS; ++c) sh[c][t] = v[c];
    __syncthreads();
    for (int w = IFIT_BLOCK / 2; w > 0; w >>= 1) {        // ifit_tree_sum
        if (t < w) {
#pragma unroll
            for (int c = 0; c < IFIT_SUMS; ++c) sh[c][t] += sh[c][t + w];
        }
        __syncthreads();
    }
    if (t < IFIT_SUMS) blk[((size_t)b * J + j) * IFIT_SUMS + t] = sh[t][0];
}

// stage B.  One thread per item: the block sums in rising block order, the rows' equal weights, ifit_finish; fit: column-major [J][IFIT_COLS]
__global__ void __launch_bounds__(256) item_fit_finish_kernel(const double* __restrict__ blk, long long n_blocks, int J, long long n_rows, int has_rt, double* __restrict__ fit)
{
    const int j = (int)(blockIdx.x * 256 + threadIdx.x);
    if (j >= J) return;
    double s[IFIT_SUMS] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (long long b = 0; b < n_blocks; ++b) {
        const double* p = blk + ((size_t)b * J + j) * IFIT_SUMS;
#pragma unroll
        for (int c = 0; c < IFIT_SUMS; ++c) s[c] += p[c];
    }
#pragma unroll
    for (int c = 0; c < IFIT_VALS; ++c) s[c] /= (double)n_rows;
    double out[IFIT_COLS];
    ifit_finish(s, has_rt != 0, out);
#pragma unroll
    for (int c = 0; c < IFIT_COLS; ++c) fit[(size_t)c * J + j] = out[c];
}

}  // namespace erm

// erm_marginal_kernels.hpp -- marginal WAIC on the device: every subject's log-likelihood with theta_i and zeta_i integrated out (erm_marginal.hpp),
// at every row of a table of item-trace rows, streamed through the WAIC accumulators of erm_pointwise.hpp.  Include after erm_kernels.hpp (PMAX, the model families).
//
// marginal_kernel<MODEL, real> runs AFTER the sweeps, from resident state: the rows are item-trace rows (a b lambda sig2t | small part of qr, fp64), the data set is
// the engine's (Y u8, logT centred by its column means and X in the engine's cell type, row-major) or a caller's (fp64, cm = nullptr).
// Geometry.  MARG_LANES = 8 lanes share a subject -- a constant, so that a subject's result depends on its own data, the rows and Q only: not on N, the other
// subjects, the grid or the device.  A workgroup of 256 threads takes ONE tile of 32 subjects through the whole row loop; the rows are never split across workgroups.
// Per row:
//   1. staging     the row after this one is copied into the other half of an LDS double buffer (with g_j = 1 / sig2t_j and log sig2t_j beside it) before this
//                  row's arithmetic starts; one barrier per row.  Every lane of the workgroup reads the same a_j, b_j: LDS broadcasts.
//   2. item sums   lane s of a subject adds its items s, s + 8, ... in order into the sums of marg_T and the two sums of the response part
//                  A1 = sum y_j a_j, A0 = sum y_j a_j b_j; a fixed butterfly adds the eight lanes.  B(theta) = theta A1 - A0 - sum_j log(1 + e^eta_j).
//                  Y and logT are read from global memory here, once per (cell, row): 9 or 5 bytes against Q evaluations of log(1 + e^eta) -- a tile's 32 J cells
//                  stay in L2 across the rows -- so the data set is not copied into LDS (at 896 items a tile's logT alone would take 229 KB).
//   3. nodes       lane s takes nodes s, s + 8, ... in chunks of MARG_CHUNK = 8: eight independent chains of marg_log1pexp per item, items in order.
//                  Each node's e_q enters the lane's (M, S); a fixed butterfly of marg_ms_merge joins the eight lanes.
//   4. accumulate  l = M + log S goes through pw_update into the subject's PwAcc, which lives in registers from the first row to the last and is stored once.
// The covariates of the subject stay in registers across the rows.  Plain vector loads and stores, no atomics: every output word has one writer.
// Steps 1 to 3 are __device__ helpers (marg_stage, marg_load_x, marg_stage_law, marg_item_sums, marg_lane_nodes) that score_kernel (erm_score_kernels.hpp) and
// pv_kernel (erm_pv_kernels.hpp) call too.
// MODEL = LATENTQR is the same kernel with the quantile weight nu_i integrated out as well: Latent's law with v read as the scale of zeta's asymmetric
// Laplace law, and qmarg_T (erm_qmarginal.hpp) at the level MargArgs::q in the place of marg_T.  marginal_kernel alone is instantiated for it.
#pragma once
#include <type_traits>
#include "erm_marginal.hpp"
#include "erm_qmarginal.hpp"
#include "erm_pointwise.hpp"

namespace erm {

constexpr int MARG_LANES = 8, MARG_LOG_LANES = 3, MARG_TILE = 256 / MARG_LANES, MARG_CHUNK = 8, MARG_MAXF = PMAX - 2;

struct MargArgs {
    const uint8_t* Y; const void* C; const void* X;       // row-major [N][J], [N][J], [N][F]; C, X of the kernel's `real`
    const double* cm;                                     // column means added back to C [J], or nullptr
    const double* rows; long long n_rows, ld;             // the table: row r at rows + r * ld
    long long N; int J, F, Q;                             // F = covariate columns the kernels see
    double* l_out;                                        // [n_rows][N] (the caller's column-major [N][n_rows]) or nullptr
    double2* acc_ms; double2* acc_w;                      // [N] or nullptr
    unsigned int* coarse;                                 // [N]: 1 if S < MARG_COARSE_S at any row; or nullptr
    double q;                                             // LatentQr: the quantile level q_rt of qmarg_T (erm_qmarginal.hpp); unread otherwise
    // the MASKED instantiations (erm_obs.hpp's compacted cell lists), unread otherwise: subject i's list is the positions off[i] .. off[i + 1] of
    // idx (the item), Y (the response) and C (the log-time, fp64), rising in the item
    const unsigned short* idx; const long long* off;
};
// where subject i's cells start in Y / C (and idx), and how many there are: the row i of [N][J], or the list of erm_obs.hpp
template <bool MASKED>
__device__ __forceinline__ size_t marg_cells(const MargArgs& A, long long i, int& n)
{
    if constexpr (MASKED) { const long long o = A.off[i]; n = (int)(A.off[i + 1] - o); return (size_t)o; }
    else { n = A.J; return (size_t)i * A.J; }
}
// doubles of LDS per half of the row buffer: the row | g [J] | log sig2t [J]
__host__ __device__ constexpr long long marg_row_lds(long long ld, int J) { return ld + 2 * (long long)J; }

// ---- the parts of a row that marginal_kernel and score_kernel (erm_score_kernels.hpp) share: one copy of the staging, the law, the item sums and the node loop
// the subject's covariates, widened
template <int MODEL, typename real>
__device__ __forceinline__ void marg_load_x(const MargArgs& A, long long i, double (&x)[MARG_MAXF])
{
    constexpr ModelTraits MT = model_traits(MODEL);
#pragma unroll
    for (int f = 0; f < MARG_MAXF; ++f) x[f] = (MT.sees_x && f < A.F) ? (double)reinterpret_cast<const real*>(A.X)[(size_t)i * A.F + f] : 0.0;
}
// staging: a row into one half of the LDS buffer, g_j and log sig2t_j beside it
template <int MODEL>
__device__ __forceinline__ void marg_stage(const MargArgs& A, long long row, double* dst, int tid)
{
    const double* src = A.rows + row * A.ld;
    for (long long e = tid; e < A.ld; e += 256) dst[e] = src[e];
    if constexpr (MODEL != MLIRT) for (int j = tid; j < A.J; j += 256) { const double v = src[3 * A.J + j]; dst[A.ld + j] = 1.0 / v; dst[A.ld + A.J + j] = log(v); }
}
// the population law at the staged row sa (v clamped at 0)
template <int MODEL>
__device__ __forceinline__ MargLaw marg_stage_law(const double* sa, int J, int F, const double (&x)[MARG_MAXF])
{
    constexpr ModelTraits MT = model_traits(MODEL);
    const double* q = sa + 4 * J;
    double xb0 = 0.0, xb1 = 0.0, bth = 0.0;
    if constexpr (MT.beta == BETA_VEC || MT.beta == BETA_LATENT || MT.beta == BETA_PAIR) {
        xb0 = q[0];
#pragma unroll
        for (int f = 0; f < MARG_MAXF; ++f) if (f < F) xb0 += x[f] * q[1 + f];
    }
    if constexpr (MT.beta == BETA_PAIR) {
        xb1 = q[F + 1];
#pragma unroll
        for (int f = 0; f < MARG_MAXF; ++f) if (f < F) xb1 += x[f] * q[F + 2 + f];
    }
    if constexpr (MT.beta == BETA_LATENT) bth = q[F + 1];
    const double S1[4] = {1.0, 0.0, 0.0, 1.0};
    MargLaw w = marg_law(MODEL, xb0, xb1, bth, MODEL != MLIRT ? q + qr_sigp_off(MODEL, J, F) : S1);
    w.v = fmax(w.v, 0.0);
    return w;
}
// item sums: lane s, items s, s + 8, ... in order; then the butterfly.  MASKED: lane s, the list positions s, s + 8, ... of the subject's n observed cells (Yi, Ci
// and Ii are the list's); the trip count is the subject's own, the butterfly stands after the loop and every lane reaches it
template <int MODEL, typename real, bool MASKED = false>
__device__ __forceinline__ void marg_item_sums(const MargArgs& A, const double* sa, const uint8_t* Yi, const real* Ci, int s, MargSums& ms, double& A1, double& A0,
                                               const unsigned short* Ii = nullptr, int n = 0)
{
    constexpr bool RT = MODEL != MLIRT;
    constexpr ModelTraits MT = model_traits(MODEL);
    const int J = A.J;
    const double* q = sa + 4 * J;
    ms = MargSums{0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    A1 = 0.0; A0 = 0.0;
    if constexpr (MASKED) {
        for (int k = s; k < n; k += MARG_LANES) {
            const int j = Ii[k];
            if (Yi[k] != 0) { const double a = sa[j]; A1 += a; A0 += a * sa[J + j]; }
            if constexpr (RT) {
                const double t = (double)Ci[k] + (A.cm ? A.cm[j] : 0.0);
                marg_sums_add(ms, sa[A.ld + j], sa[A.ld + J + j], sa[2 * J + j] - t, MT.rho ? q[j] : 0.0);
            }
        }
    } else
    for (int j = s; j < J; j += MARG_LANES) {
        if (Yi[j] != 0) { const double a = sa[j]; A1 += a; A0 += a * sa[J + j]; }
        if constexpr (RT) {
            const double t = (double)Ci[j] + (A.cm ? A.cm[j] : 0.0);
            marg_sums_add(ms, sa[A.ld + j], sa[A.ld + J + j], sa[2 * J + j] - t, MT.rho ? q[j] : 0.0);
        }
    }
    for (int m = 1; m < MARG_LANES; m <<= 1) {
        A1 += __shfl_xor(A1, m, 64); A0 += __shfl_xor(A0, m, 64);
        if constexpr (RT) {
            ms.P += __shfl_xor(ms.P, m, 64); ms.R0 += __shfl_xor(ms.R0, m, 64); ms.D0 += __shfl_xor(ms.D0, m, 64); ms.L += __shfl_xor(ms.L, m, 64);
            if constexpr (MT.rho) { ms.R1 += __shfl_xor(ms.R1, m, 64); ms.D1 += __shfl_xor(ms.D1, m, 64); ms.D2 += __shfl_xor(ms.D2, m, 64); }
        }
    }
}
// nodes: lane s, nodes s, s + 8, ... in chunks of MARG_CHUNK; sink(e_q, z_q) -- or sink(e_q, z_q, q) if it takes the node's index too -- receives the lane's nodes in order.
// LatentQr takes qmarg_T at the level q_rt for marg_T: two logPhi per node beside the J evaluations of log(1 + e^eta)
// MASKED (Ii: the subject's list of n items, rising): every node's chain runs over the list in order -- the eight lanes of a subject read the same Ii[k], a broadcast,
// once per MARG_CHUNK chains -- and n stands for J in T.  The trip count is the subject's own; nothing inside the loop crosses lanes.
template <int MODEL, bool MASKED = false, typename Sink>
__device__ __forceinline__ void marg_lane_nodes(const double* sa, int J, int Q, int s, double h, double log_h, const MargLaw& w, const MargSums& ms, double A1, double A0, Sink&& sink,
                                                double q_rt = 0.0, const unsigned short* Ii = nullptr, int n = 0)
{
    for (int q0 = s; q0 < Q; q0 += MARG_LANES * MARG_CHUNK) {
        double th[MARG_CHUNK], lse[MARG_CHUNK];
#pragma unroll
        for (int c = 0; c < MARG_CHUNK; ++c) {
            const int qq = q0 + c * MARG_LANES;
            th[c] = w.mu + w.sd * marg_node(qq < Q ? qq : Q - 1, h);      // (a slot past the last node repeats it and is dropped below)
            lse[c] = 0.0;
        }
        if constexpr (MASKED) {
            for (int k = 0; k < n; ++k) {
                const int j = Ii[k];
                const double a = sa[j], b = sa[J + j];
#pragma unroll
                for (int c = 0; c < MARG_CHUNK; ++c) lse[c] += marg_log1pexp(a * (th[c] - b));
            }
        } else
        for (int j = 0; j < J; ++j) {
            const double a = sa[j], b = sa[J + j];
#pragma unroll
            for (int c = 0; c < MARG_CHUNK; ++c) lse[c] += marg_log1pexp(a * (th[c] - b));
        }
#pragma unroll
        for (int c = 0; c < MARG_CHUNK; ++c) {
            const int qq = q0 + c * MARG_LANES;
            if (qq < Q) {
                const double z = marg_node(qq, h);
                double e = marg_log_weight(z, log_h) + (th[c] * A1 - A0 - lse[c]);
                if constexpr (MODEL == LATENTQR) e += qmarg_T(ms, J, w, th[c], q_rt);
                else if constexpr (MODEL != MLIRT) e += marg_T(ms, MASKED ? n : J, w, th[c]);
                if constexpr (std::is_invocable_v<Sink, double, double, int>) sink(e, z, qq);
                else sink(e, z);
            }
        }
    }
}

// MASKED: the same kernel over incomplete response patterns.  A subject's cells are its list (marg_cells); the item sums and the node chains run
// over the list, so the work is proportional to the observed cells.  The subjects of a wave have different trip counts: a finished subject's lanes idle until the
// wave's longest is done, and every butterfly and barrier stands outside those loops.  n = 0 is an ordinary case: every sum is empty and T = 0.
template <int MODEL, typename real, bool MASKED = false>
__global__ void __launch_bounds__(256) marginal_kernel(const MargArgs A)
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
    PwAcc acc{0.0, 0.0, 0.0, 0.0};
    bool coarse = false;
    for (long long row = 0; row < A.n_rows; ++row) {
        const double* sa = sh + (row & 1) * half;
        if (row + 1 < A.n_rows) marg_stage<MODEL>(A, row + 1, sh + ((row + 1) & 1) * half, tid);
        const MargLaw w = marg_stage_law<MODEL>(sa, J, F, x);
        MargSums ms;
        double A1, A0;
        marg_item_sums<MODEL, real, MASKED>(A, sa, Yi, Ci, s, ms, A1, A0, Ii, n);
        MargMS part{0.0, 0.0};
        marg_lane_nodes<MODEL, MASKED>(sa, J, Q, s, h, log_h, w, ms, A1, A0, [&](double e, double) { marg_ms_add(part, e); }, A.q, Ii, n);
        for (int m = 1; m < MARG_LANES; m <<= 1) {
            const MargMS o{__shfl_xor(part.M, m, 64), __shfl_xor(part.S, m, 64)};
            part = marg_ms_merge(part, o);
        }
        const double l = marg_ms_log(part);
        coarse = coarse || part.S < MARG_COARSE_S;
        pw_update(acc, l, row + 1);
        if (ok && s == 0 && A.l_out) A.l_out[(size_t)row * A.N + i] = l;
        __syncthreads();                                  // the next row is staged; this row's half is free for the one after
    }
    if (ok && s == 0) {
        if (A.acc_ms) { A.acc_ms[i] = make_double2(acc.m, acc.s); A.acc_w[i] = make_double2(acc.mean, acc.m2); }
        if (A.coarse) A.coarse[i] = coarse ? 1u : 0u;
    }
}

// the number of flagged subjects: thread t adds its entries in order, then a fixed tree (one workgroup)
__global__ void __launch_bounds__(256) marginal_count_kernel(const unsigned int* flag, long long n, unsigned long long* out)
{
    __shared__ unsigned long long sh[256];
    unsigned long long t = 0;
    for (long long k = threadIdx.x; k < n; k += 256) t += flag[k];
    sh[threadIdx.x] = t;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) { if ((int)threadIdx.x < w) sh[threadIdx.x] += sh[threadIdx.x + w]; __syncthreads(); }
    if (threadIdx.x == 0) *out = sh[0];
}

}  // namespace erm

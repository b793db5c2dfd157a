// erm_waic_kernels.hpp -- WAIC on the device: the pointwise log-likelihood of every unit, accumulated once per post-burn-in sweep.
// Included by erm_kernels.hpp (uses its Ctl, log1pexp_r and the model families of erm_layout.hpp).  CellArgs, the head of this pass's kernel arguments, is shared
// with the replicate pass (erm_predictive_kernels.hpp); the cell arithmetic of the two is not (log1pexp_r here, exp(-|eta|) / log1p there, each pinned to its twin).
//
// pointwise_kernel<MODEL, real, UNIT> is ONE streaming pass over the resident data set, launched behind every sweep's own kernels (on the stream and inside
// every captured graph): at that point theta_t, zeta_t, the item parameters of sweep t and the counters of trace row t are all resident.  It reads the
// counters itself and returns at once for a burn-in row, so the launch is the same for every sweep.  The cell term is the cell term of loglik_kernel
// (getLogLikelihood*'s), in fp64 with libm's exp / log1p / log from the stored state whatever the engine's precision:
//     l_ij = y eta - log(1 + e^eta), eta = a_j (theta_i - b_j)            [+ log N(logT_ij; mu_ij, var_ij) for every model but GibbsMlIrt]
//     mu_ij = lambda_j - zeta_i [- theta_i rho_j + k1 nu_ij],  var_ij = sig2t_j [k2 nu_ij]      (brackets: Cross family; nu == 1, k1 = 0, k2 = 1 without weights)
// GibbsRtIrtCrossQr's nu_t is read from the snapshot the engine takes ahead of pass B (which overwrites nu_t with nu_{t+1}).
// Accumulators (erm_pointwise.hpp): two double2 arrays, {m, s}[unit] and {mean, m2}[unit] -- every access is 16 bytes, and consecutive lanes of the cell
// unit touch consecutive units (device order: row-major [nSubj][nItem], any nItem), so a wave's read-modify-write covers whole cache lines.
// Plain vector loads and stores, no atomics: every unit has exactly one writer, and a subject's lanes combine their partial sums by a fixed butterfly.
#pragma once
#include "erm_pointwise.hpp"

namespace erm {

// A resident cell as every pass behind a sweep reads it (this one and erm_predictive_kernels.hpp): filled in one place, Engine::cell_args
struct CellArgs {
    const uint8_t* Y; const void* C; const void* nu;      // resident data set (row-major [N][J]); nu: CrossQr's snapshot of nu_t, else nullptr
    const void* theta; const void* zeta;                  // [N], the engine's cell type
    const double* par;                                    // the parameter block of the sweep just drawn
    const double* cm;                                     // column means of logT [J]
    const Ctl* ctl;                                       // the counters that sweep published: sweep, row, burn_rows
    long long N; int J; int logW;                         // W = 2^logW lanes share a subject (pass_geom, erm_geometry.hpp)
    double k1, k2;
};

struct PwArgs {
    CellArgs cell;
    double2* acc_ms; double2* acc_w;                      // [units]
};

template <int MODEL>
__device__ __forceinline__ double pw_cell(bool y, double th, double ze, double c, double nu, int j, const double* sa, int J, double k1, double k2)
{
    const double eta = sa[j] * (th - sa[J + j]);
    double l = (y ? eta : 0.0) - log1pexp_r(eta);
    if constexpr (MODEL != MLIRT) {
        const double lt = c + sa[5 * J + j];
        double mu = sa[2 * J + j] - ze, var = sa[3 * J + j];
        if constexpr (fam_cq(MODEL)) { mu += -th * sa[4 * J + j] + k1 * nu; var *= k2 * nu; }
        const double er = lt - mu;
        // (the logarithm of the variance is per item unless the cell carries a quantile weight: staged in sa[6 J + j])
        l += (MODEL == CROSSQR ? -0.5 * LOG_2PI - 0.5 * log(var) : sa[6 * J + j]) - 0.5 * er * er / var;
    }
    return l;
}

template <int MODEL, typename real, int UNIT>
__global__ void __launch_bounds__(256) pointwise_kernel(const PwArgs A)
{
    const uint32_t row = A.cell.ctl->row, burn = A.cell.ctl->burn_rows;
    if (row < burn) return;                               // burn-in rows do not enter S (uniform: every thread reads the same word)
    const long long k = (long long)(row - burn) + 1;      // this is the k-th post-burn-in row
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    double* sa = reinterpret_cast<double*>(smem);         // a b lambda sig2t rho [5][J] | column means [J] | -1/2 (log 2 pi + log var_j) [J]
    const int J = A.cell.J, tid = (int)threadIdx.x;
    for (int e = tid; e < 5 * J; e += 256) sa[e] = A.cell.par[e];
    for (int j = tid; j < J; j += 256) {
        sa[5 * J + j] = (MODEL != MLIRT) ? A.cell.cm[j] : 0.0;
        double var = A.cell.par[3 * J + j];
        if (fam_cq(MODEL)) var *= A.cell.k2;                   // GibbsRtIrtCross: k2 = 1, nu = 1
        sa[6 * J + j] = (MODEL != MLIRT) ? -0.5 * LOG_2PI - 0.5 * log(var) : 0.0;
    }
    __syncthreads();
    const real* C = reinterpret_cast<const real*>(A.cell.C);
    const real* NU = reinterpret_cast<const real*>(A.cell.nu);
    const real* TH = reinterpret_cast<const real*>(A.cell.theta);
    const real* ZE = reinterpret_cast<const real*>(A.cell.zeta);
    if constexpr (UNIT == PW_SUBJECT) {
        const int W = 1 << A.cell.logW, R = 256 >> A.cell.logW;     // a workgroup takes R subjects at a time, W lanes each (W divides the wave)
        const int s = tid & (W - 1), r = tid >> A.cell.logW;
        for (long long i0 = (long long)blockIdx.x * R; i0 < A.cell.N; i0 += (long long)gridDim.x * R) {
            const bool ok = i0 + r < A.cell.N;
            const long long i = ok ? i0 + r : A.cell.N - 1;    // idle lanes repeat the last subject: every lane takes part in the butterfly
            const double th = (double)TH[i], ze = (MODEL != MLIRT) ? (double)ZE[i] : 0.0;
            const size_t e0 = (size_t)i * J;
            double t = 0.0;
            for (int j = s; j < J; j += W) {              // lane s: items s, s + W, ... in order
                const double c = (MODEL != MLIRT) ? (double)C[e0 + j] : 0.0;
                const double nu = (MODEL == CROSSQR) ? (double)NU[e0 + j] : 1.0;
                t += pw_cell<MODEL>(A.cell.Y[e0 + j] != 0, th, ze, c, nu, j, sa, J, A.cell.k1, A.cell.k2);
            }
            for (int m = 1; m < W; m <<= 1) t += __shfl_xor(t, m, 64);     // fixed-order butterfly over the subject's lanes
            if (ok && s == 0) {
                const double2 ms = A.acc_ms[i], w = A.acc_w[i];
                PwAcc a{ms.x, ms.y, w.x, w.y};
                pw_update(a, t, k);
                A.acc_ms[i] = make_double2(a.m, a.s); A.acc_w[i] = make_double2(a.mean, a.m2);
            }
        }
    } else {
        const long long NJ = A.cell.N * (long long)J;
        for (long long e = (long long)blockIdx.x * 256 + tid; e < NJ; e += (long long)gridDim.x * 256) {
            const long long i = e / J;
            const int j = (int)(e - i * J);
            const double th = (double)TH[i], ze = (MODEL != MLIRT) ? (double)ZE[i] : 0.0;
            const double c = (MODEL != MLIRT) ? (double)C[e] : 0.0;
            const double nu = (MODEL == CROSSQR) ? (double)NU[e] : 1.0;
            const double l = pw_cell<MODEL>(A.cell.Y[e] != 0, th, ze, c, nu, j, sa, J, A.cell.k1, A.cell.k2);
            const double2 ms = A.acc_ms[e], w = A.acc_w[e];
            PwAcc a{ms.x, ms.y, w.x, w.y};
            pw_update(a, l, k);
            A.acc_ms[e] = make_double2(a.m, a.s); A.acc_w[e] = make_double2(a.mean, a.m2);
        }
    }
}

// The per-unit finish and the totals: lppd_u, p_u (optionally stored, device order) and per-workgroup partial sums
//   part[b][0..4] = sum lppd_u, sum p_u, sum elpd_u, sum (elpd_u - center)^2, number of units with p_u > PW_VAR_WARN
// Thread t adds its units t, t + T, ... in order, a workgroup's threads are summed by a fixed tree, the host adds the rows in order (as erm_get_dic does).
// The host calls it twice: with center = 0 for the sums, then with center = mean(elpd_u) for the variance over the units.
struct PwFinArgs {
    const double2* acc_ms; const double2* acc_w; long long U; long long n; double center;
    double* lppd_out; double* p_out; double* part;
};
constexpr int PW_FIN_COLS = 5;
__global__ void __launch_bounds__(256) pointwise_finish_kernel(const PwFinArgs A)
{
    __shared__ double red[PW_FIN_COLS][256];
    const int tid = (int)threadIdx.x;
    double t[PW_FIN_COLS] = {0.0, 0.0, 0.0, 0.0, 0.0};
    for (long long u = (long long)blockIdx.x * 256 + tid; u < A.U; u += (long long)gridDim.x * 256) {
        const double2 ms = A.acc_ms[u], w = A.acc_w[u];
        const PwAcc a{ms.x, ms.y, w.x, w.y};
        const double lppd = pw_lppd(a, A.n), p = pw_var(a, A.n), el = lppd - p, d = el - A.center;
        t[0] += lppd; t[1] += p; t[2] += el; t[3] += d * d; t[4] += (p > PW_VAR_WARN) ? 1.0 : 0.0;
        if (A.lppd_out) A.lppd_out[u] = lppd;
        if (A.p_out) A.p_out[u] = p;
    }
    for (int q = 0; q < PW_FIN_COLS; ++q) red[q][tid] = t[q];
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (tid < w) for (int q = 0; q < PW_FIN_COLS; ++q) red[q][tid] += red[q][tid + w];
        __syncthreads();
    }
    if (tid < PW_FIN_COLS) A.part[(size_t)blockIdx.x * PW_FIN_COLS + tid] = red[tid][0];
}

}  // namespace erm

// erm_predictive_kernels.hpp -- posterior predictive checks on the device: at every replicate row the data set is drawn again from the model at
// the values of that row and three discrepancies of the replicate are compared with the same discrepancies of the observed data.
// Included by ertirt.hip behind erm_kernels.hpp (uses its Ctl, the Philox block of erm_rng.hpp and the model families of erm_layout.hpp).
//
// Specification (restated independently by the numpy twin, gibbs.py::getPpcHost).  Post-burn-in row number k = 1, 2, ... (row >= burn_rows) is a replicate row
// when (k - 1) mod thin = 0.  Per cell (i, j), from the stored state in fp64 whatever the engine's precision:
//     eta = a_j (theta_i - b_j),  p = 1 / (1 + e^-eta),  l = y eta - log(1 + e^eta)
//     mu = lambda_j - zeta_i [- theta_i rho_j + k1 nu_ij],  var = sig2t_j [k2 nu_ij]      (brackets: Cross family; nu == 1, k1 = 0, k2 = 1 without weights)
//     (w0, w1, w2, w3) = Philox4x32-10(key = seed; ctr = {i + row_base, j, Ctl.sweep, SITE_PRED << 24 | chain << 16})       -- ONE block per cell
//     y_rep = [u(w0) < p],  z = sqrt(-2 log u(w1)) cos(2 pi u(w2)),  logT_rep = mu + sqrt(var) z,      u(w) = (w + 1/2) 2^-32
//   responses (deviance):     D_obs = -2 sum l,  D_rep = D_obs + 2 Delta,  Delta = sum (y - y_rep) eta      (a cell with y_rep = y adds an exact zero: a unit
//                             whose replicate equals its data ties exactly in any arithmetic, which is why both >= and > are counted)
//   response times (chi^2):   D_obs = sum (logT - mu)^2 / var,  D_rep = sum z^2                              (every model but GibbsMlIrt)
//   item score:               T_obs = sum_i y_ij,  T_rep = sum_i y_rep,ij                                    (items only)
// Units: every subject (over its items), every item (over all subjects), the data set.  Per unit and component four doubles, updated once per replicate row in
// trace order: { #(rep >= obs), #(rep > obs), running mean of obs, running mean of rep }.
//
// predictive_kernel<MODEL, real> is ONE streaming pass over Y, C, (CrossQr's snapshot of nu_t), theta, zeta, launched behind every sweep like the WAIC pass: it reads
// the counters itself and returns at once on a row that is no replicate row, so the launch is the same for every sweep and sits inside the captured graphs.
// W = 2^logW lanes share a subject (lane s: items s, s + W, ... in order; consecutive lanes read consecutive cells); the subject's four partial sums are combined by a
// fixed butterfly and lane 0 updates the subject's 64 bytes with plain vector stores.  The item sums live in LDS, one private copy [NQ][J] per subject slot of the
// workgroup: entry (slot r, item j) is written by lane j mod W of slot r only, subjects in order, so there is no atomic and no race; at the end the slots are
// added in order and the workgroup writes ONE slab row [NQ][J].  predictive_items_kernel (one workgroup) adds the slab rows in workgroup order, updates the item and
// total accumulators and counts the replicate.  No floating-point atomics: the launch geometry is a function of (nSubj, nItem) alone, so the accumulators are
// bit-reproducible run to run and do not depend on the sweep kernels' geometry or schedule.
#pragma once
#include "erm_kernels.hpp"
#include "erm_geometry.hpp"      // the pass's launch geometry, slab columns and LDS request: pass_geom, pred_nq, pass_log_lanes, pred_lds_bytes

namespace erm {

constexpr uint32_t SITE_PRED = 14;                         // the replicate draws' stream site (free in erm_rng.hpp's Site)
constexpr int PRED_SUBJ = 8, PRED_ITEM = 12, PRED_TOT = 8; // doubles per subject [RA, RT][4], per item [RA, RT, SCORE][4], of the data set [RA, RT][4]

struct PredArgs {
    CellArgs cell;                                        // erm_waic_kernels.hpp
    double* subj;                                         // [N][PRED_SUBJ]
    double* slab;                                         // [gridDim.x][NQ][J]
    uint32_t thin;
    uint64_t seed; uint32_t chain; uint32_t row_base;
};

// {n_ge, n_gt} and {mean_obs, mean_rep} of one unit and component after replicate number rk (the accumulators start from zero)
__device__ __forceinline__ void pred_update(double2& cnt, double2& mean, double obs, double rep, bool ge, bool gt, double rk)
{
    cnt.x += ge ? 1.0 : 0.0; cnt.y += gt ? 1.0 : 0.0;
    mean.x += (obs - mean.x) / rk; mean.y += (rep - mean.y) / rk;
}

template <int MODEL, typename real>
__global__ void __launch_bounds__(256) predictive_kernel(const PredArgs A)
{
    const uint32_t row = A.cell.ctl->row, burn = A.cell.ctl->burn_rows;
    if (row < burn) return;                               // (uniform: every thread reads the same words)
    const uint32_t kpost = row - burn;                    // k - 1
    if (kpost % A.thin != 0u) return;
    const double rk = (double)(kpost / A.thin + 1u);      // this is replicate number rk
    const uint32_t sweep = A.cell.ctl->sweep;
    constexpr int NQ = pred_nq(MODEL);
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    double* sa = reinterpret_cast<double*>(smem);         // a b lambda sig2t rho [5][J] | column means [J]
    const int J = A.cell.J, tid = (int)threadIdx.x, T = (int)blockDim.x;
    const int W = 1 << A.cell.logW, R = T >> A.cell.logW;           // a workgroup takes R subjects at a time, W lanes each (W divides the wave)
    double* acc = sa + 6 * J;                             // [R][NQ][J]
    for (int e = tid; e < 5 * J; e += T) sa[e] = A.cell.par[e];
    for (int j = tid; j < J; j += T) sa[5 * J + j] = (MODEL != MLIRT) ? A.cell.cm[j] : 0.0;
    for (int e = tid; e < R * NQ * J; e += T) acc[e] = 0.0;
    __syncthreads();
    const real* C = reinterpret_cast<const real*>(A.cell.C);
    const real* NU = reinterpret_cast<const real*>(A.cell.nu);
    const real* TH = reinterpret_cast<const real*>(A.cell.theta);
    const real* ZE = reinterpret_cast<const real*>(A.cell.zeta);
    const int s = tid & (W - 1), r = tid >> A.cell.logW;
    double* my = acc + (size_t)r * NQ * J;
    const uint32_t k0 = (uint32_t)A.seed, k1 = (uint32_t)(A.seed >> 32), c3 = (SITE_PRED << 24) | ((A.chain & 0xFFu) << 16);
    for (long long i0 = (long long)blockIdx.x * R; i0 < A.cell.N; i0 += (long long)gridDim.x * R) {
        const bool ok = i0 + r < A.cell.N;
        const long long i = ok ? i0 + r : A.cell.N - 1;        // idle lanes repeat the last subject (every lane takes part in the butterfly) and add nothing to the items
        const double th = (double)TH[i], ze = (MODEL != MLIRT) ? (double)ZE[i] : 0.0;
        const size_t e0 = (size_t)i * J;
        const uint32_t ig = (uint32_t)i + A.row_base;
        double sd = 0.0, sl = 0.0, so = 0.0, sr = 0.0;
        for (int j = s; j < J; j += W) {                  // lane s: items s, s + W, ... in order
            const bool y = A.cell.Y[e0 + j] != 0;
            const double eta = sa[j] * (th - sa[J + j]);
            const double en = exp(-fabs(eta)), l1p = log1p(en);
            const double l = (y ? eta : 0.0) - (eta > 0.0 ? eta + l1p : l1p);
            const double p = eta >= 0.0 ? 1.0 / (1.0 + en) : en / (1.0 + en);
            uint32_t w0, w1, w2, w3;
            uint32_t q0 = k0, q1 = k1;
            asm volatile("" : "+s"(q0), "+s"(q1));         // opaque per cell: the twenty round keys are re-derived by scalar adds instead of living in 18 more SGPRs
            philox4x32_10(ig, (uint32_t)j, sweep, c3, q0, q1, w0, w1, w2, w3);
            const bool yr = word_to_unif<double>(w0) < p;
            const double d = ((y ? 1.0 : 0.0) - (yr ? 1.0 : 0.0)) * eta;      // an exact zero when the replicate repeats the datum
            sd += d; sl += l;
            double dobs = 0.0, drep = 0.0;
            if constexpr (MODEL != MLIRT) {
                const double lt = (double)C[e0 + j] + sa[5 * J + j];
                double mu = sa[2 * J + j] - ze, var = sa[3 * J + j];
                if constexpr (fam_cq(MODEL)) {
                    const double nu = (MODEL == CROSSQR) ? (double)NU[e0 + j] : 1.0;
                    mu += -th * sa[4 * J + j] + A.cell.k1 * nu; var *= A.cell.k2 * nu;
                }
                const double er = lt - mu, c = fm::cos2pi(word_to_unif<double>(w2));
                dobs = er * er / var;
                drep = -2.0 * fm::log(word_to_unif<double>(w1)) * (c * c);    // z^2
                so += dobs; sr += drep;
            }
            if (ok) {
                my[j] += d; my[J + j] += l;
                if constexpr (MODEL != MLIRT) { my[2 * J + j] += dobs; my[3 * J + j] += drep; }
                my[(NQ - 1) * J + j] += yr ? 1.0 : 0.0;
            }
        }
        for (int m = 1; m < W; m <<= 1) {                 // fixed-order butterfly over the subject's lanes
            sd += __shfl_xor(sd, m, 64); sl += __shfl_xor(sl, m, 64);
            if constexpr (MODEL != MLIRT) { so += __shfl_xor(so, m, 64); sr += __shfl_xor(sr, m, 64); }
        }
        if (ok && s == 0) {
            double2* P = reinterpret_cast<double2*>(A.subj + (size_t)i * PRED_SUBJ);
            double2 cnt = P[0], mean = P[1];
            const double Dobs = -2.0 * sl;
            pred_update(cnt, mean, Dobs, Dobs + 2.0 * sd, sd >= 0.0, sd > 0.0, rk);
            P[0] = cnt; P[1] = mean;
            if constexpr (MODEL != MLIRT) {
                cnt = P[2]; mean = P[3];
                pred_update(cnt, mean, so, sr, sr >= so, sr > so, rk);
                P[2] = cnt; P[3] = mean;
            }
        }
    }
    __syncthreads();
    double* out = A.slab + (size_t)blockIdx.x * NQ * J;
    for (int e = tid; e < NQ * J; e += T) {               // the workgroup's subject slots, added in order
        double t = 0.0;
        for (int q = 0; q < R; ++q) t += acc[(size_t)q * NQ * J + e];
        out[e] = t;
    }
}

// The slab rows summed in workgroup order, the item and total accumulators, the replicate counter.  ONE workgroup: lane l of part p adds the rows of part p (a
// contiguous range of workgroups, in order) for item j0 + l, the parts are added in order, the totals add the items in order.
struct PredItemArgs {
    const double* slab; int nb; int nq; int J; double N;
    const double* k0;                                     // the data constants' K0_j = sum_i (y_ij - 1/2): T_obs = K0_j + N / 2, exactly
    const Ctl* ctl; uint32_t thin;
    double* item;                                         // [J][PRED_ITEM]
    double* tot;                                          // [PRED_TOT], then the replicate counter (one unsigned long long)
};
__global__ void __launch_bounds__(PRED_IT_THREADS) predictive_items_kernel(const PredItemArgs A)
{
    const uint32_t row = A.ctl->row, burn = A.ctl->burn_rows;
    if (row < burn) return;
    const uint32_t kpost = row - burn;
    if (kpost % A.thin != 0u) return;
    const double rk = (double)(kpost / A.thin + 1u);
    __shared__ double red[PRED_IT_PARTS][PRED_NQ_RT][64];
    __shared__ double tl[4][64];
    const int tid = (int)threadIdx.x, lane = tid & 63, part = tid >> 6, J = A.J, nq = A.nq;
    const bool rt = nq == PRED_NQ_RT;
    const int per = (A.nb + PRED_IT_PARTS - 1) / PRED_IT_PARTS;
    const int b0 = part * per, b1 = min(A.nb, b0 + per);
    double tsum[4] = {0.0, 0.0, 0.0, 0.0};                // this lane's items so far: Delta, sum l, D^T_obs, D^T_rep
    for (int j0 = 0; j0 < J; j0 += 64) {
        const int j = j0 + lane;
        double t[PRED_NQ_RT] = {0.0, 0.0, 0.0, 0.0, 0.0};
        if (j < J) for (int b = b0; b < b1; ++b) for (int q = 0; q < nq; ++q) t[q] += A.slab[((size_t)b * nq + q) * J + j];
        for (int q = 0; q < PRED_NQ_RT; ++q) red[part][q][lane] = t[q];
        __syncthreads();
        if (part == 0 && j < J) {
            for (int q = 0; q < nq; ++q) { double v = 0.0; for (int p = 0; p < PRED_IT_PARTS; ++p) v += red[p][q][lane]; t[q] = v; }
            double2* P = reinterpret_cast<double2*>(A.item + (size_t)j * PRED_ITEM);
            double2 cnt = P[0], mean = P[1];
            const double Dobs = -2.0 * t[1];
            pred_update(cnt, mean, Dobs, Dobs + 2.0 * t[0], t[0] >= 0.0, t[0] > 0.0, rk);
            P[0] = cnt; P[1] = mean;
            tsum[0] += t[0]; tsum[1] += t[1];
            if (rt) {
                cnt = P[2]; mean = P[3];
                pred_update(cnt, mean, t[2], t[3], t[3] >= t[2], t[3] > t[2], rk);
                P[2] = cnt; P[3] = mean;
                tsum[2] += t[2]; tsum[3] += t[3];
            }
            const double Tobs = A.k0[j] + 0.5 * A.N, Trep = t[nq - 1];
            cnt = P[4]; mean = P[5];
            pred_update(cnt, mean, Tobs, Trep, Trep >= Tobs, Trep > Tobs, rk);
            P[4] = cnt; P[5] = mean;
        }
        __syncthreads();
    }
    if (part == 0) for (int q = 0; q < 4; ++q) tl[q][lane] = tsum[q];
    __syncthreads();
    if (tid == 0) {
        double v[4];
        for (int q = 0; q < 4; ++q) { double u = 0.0; for (int l = 0; l < 64; ++l) u += tl[q][l]; v[q] = u; }
        double2* P = reinterpret_cast<double2*>(A.tot);
        double2 cnt = P[0], mean = P[1];
        const double Dobs = -2.0 * v[1];
        pred_update(cnt, mean, Dobs, Dobs + 2.0 * v[0], v[0] >= 0.0, v[0] > 0.0, rk);
        P[0] = cnt; P[1] = mean;
        if (rt) {
            cnt = P[2]; mean = P[3];
            pred_update(cnt, mean, v[2], v[3], v[3] >= v[2], v[3] > v[2], rk);
            P[2] = cnt; P[3] = mean;
        }
        unsigned long long* reps = reinterpret_cast<unsigned long long*>(A.tot + PRED_TOT);
        *reps = *reps + 1ull;
    }
}

}  // namespace erm

// erm_ifit.hpp -- item fit and drift from the item trace (include/ertirt.h: erm_get_item_fit): whether the saved item parameters still hold for a
// sample, as PURE functions usable from host and device, beside erm_fit.hpp whose law, item sums, node rule and weights w_q = exp(e_q - M) / S they share.
//
// For an observed cell (i, j) at node theta_q:
//     responses        eta = a_j (theta_q - b_j), t = e^-min(|eta|, 700), "agree" = (y = 1) <=> (eta >= 0)                                          (ifit_resp)
//                      r = t / (1 + t) if agree, else 1 / (1 + t) = |y - p|;  c = t / (1 + t)^2 = p (1 - p);  z^2 = t if agree, else 1 / t = r^2 / c without
//                      the cancellation (the clamp keeps every term finite; below it t is e^-|eta| itself);  e = (2 y - 1) r.  ONE exp per cell-node.
//     response times   u = lambda_j - rho_j theta_q - logT_ij, g = 1 / sig2t_j, R = R0 - theta_q R1, m = m0 + m1 theta_q: the leave-one-item-out prediction given
//                      theta and the subject's OTHER observed times, zeta integrated out:  Pi = 1 + v (P - g),  m_ = (m + v (R - g u)) / Pi,  v_ = v / Pi,
//                      d = -(u - m_) / sqrt(sig2t_j + v_): positive means slower than predicted, d^2 is chi^2_1 given theta.  No 1 / v: v = 0 is an ordinary case.
//                      Pi and the square root do not depend on the node: ifit_rt_prep lays them down once per cell, ifit_rt_d is the node's part.
//     per cell         the six means E[e], E[r^2], E[c], E[z^2], E[d], E[d^2] under w_q, averaged over the rows with equal weights, in trace order.
//     per item         their sums over the subjects that observed the item, n_j their count, and the six columns of ifit_finish.
// The sums over the subjects have ONE order whatever the chunking: blocks of IFIT_BLOCK = 256 consecutive subjects by global index, each summed by the fixed binary
// tree of ifit_tree_sum (absent subjects count 0), then the block sums added in rising block order (ifit_reduce).  ifit_chunk gives chunks of whole blocks.
// The same header is compiled by g++ with -fsanitize=undefined -ftrapv into tests/ifit_check (tests/test_ifit_host.py).  No HIP, no allocation, no environment.
#pragma once
#include <cstdint>
#include "erm_fit.hpp"

namespace erm {

constexpr int IFIT_INFIT = 0, IFIT_OUTFIT = 1, IFIT_RESP_Z = 2, IFIT_RT_MSQ = 3, IFIT_RT_Z = 4, IFIT_N_OBS = 5, IFIT_COLS = 6;
// the six values of a cell, in the order of the workspace's words; the block sums carry the count of observing subjects as a seventh
constexpr int IFIT_E = 0, IFIT_R2 = 1, IFIT_C = 2, IFIT_Z2 = 3, IFIT_D = 4, IFIT_D2 = 5, IFIT_VALS = 6, IFIT_SUMS = 7;
constexpr int IFIT_BLOCK = 256;
constexpr double IFIT_ETA_MAX = 700.0;

// the four response values of a cell at one node, from ONE exp
ERM_MG_FN void ifit_resp(double eta, bool y, double& e, double& r2, double& c, double& z2)
{
    const double t = exp(-fmin(fabs(eta), IFIT_ETA_MAX)), inv = 1.0 / (1.0 + t), small = t * inv;      // small <= 1/2 <= inv: the two probabilities of the cell
    const bool agree = y == (eta >= 0.0);
    const double r = agree ? small : inv;
    e = y ? r : -r;
    r2 = r * r;
    c = small * inv;
    z2 = agree ? t : 1.0 / t;
}

// what a cell's response-time residual keeps across the nodes: g, d0 = lambda_j - logT_ij, rho_j, 1 / Pi and 1 / sqrt(sig2t_j + v / Pi)
struct IfitRt { double g, d0, rho, ipi, isd; };
ERM_MG_FN IfitRt ifit_rt_prep(double g, double sig2t, double d0, double rho, double P, double v)
{
    const double ipi = 1.0 / (1.0 + v * (P - g));
    return {g, d0, rho, ipi, 1.0 / sqrt(sig2t + v * ipi)};
}
// d at theta: R = R0 - theta R1 and m = m0 + m1 theta are the node's
ERM_MG_FN double ifit_rt_d(const IfitRt& k, double v, double R, double m, double theta)
{
    const double u = k.d0 - k.rho * theta;
    return ((m + v * (R - k.g * u)) * k.ipi - u) * k.isd;
}

// an item's row from its seven sums over the subjects (the six values as sums of per-cell means, and n_j): out[IFIT_COLS].  A model without response times gets
// NaN in RT_MSQ and RT_Z, an item nobody observed (n = 0) in all five statistics.
ERM_MG_FN void ifit_finish(const double* s, bool has_rt, double* out)
{
    const double nan = NAN, n = s[IFIT_VALS];
    const bool any = n > 0.0;
    out[IFIT_INFIT] = any ? s[IFIT_R2] / s[IFIT_C] : nan;
    out[IFIT_OUTFIT] = any ? s[IFIT_Z2] / n : nan;
    out[IFIT_RESP_Z] = any ? s[IFIT_E] / sqrt(s[IFIT_C]) : nan;
    out[IFIT_RT_MSQ] = has_rt && any ? s[IFIT_D2] / n : nan;
    out[IFIT_RT_Z] = has_rt && any ? s[IFIT_D] / sqrt(n) : nan;
    out[IFIT_N_OBS] = n;
}

// ---- the order of the sums over the subjects
// the subjects of a chunk: whole blocks.  budget = the subjects whose per-chunk buffers fit the pass's memory (item_pass_chunk), rounded down to a multiple of
// IFIT_BLOCK but at least one block; cap > 0 (ERM_IFIT_CHUNK, for the tests): no more than cap rounded UP to a multiple of IFIT_BLOCK
ERM_MG_FN int64_t ifit_chunk(int64_t budget, int64_t cap)
{
    int64_t chunk = budget / IFIT_BLOCK * IFIT_BLOCK;
    if (chunk < IFIT_BLOCK) chunk = IFIT_BLOCK;
    if (cap > 0) {
        const int64_t up = (cap + IFIT_BLOCK - 1) / IFIT_BLOCK * IFIT_BLOCK;
        if (up < chunk) chunk = up;
    }
    return chunk;
}
ERM_MG_FN int64_t ifit_blocks(int64_t N) { return (N + IFIT_BLOCK - 1) / IFIT_BLOCK; }
// the fixed binary tree over the IFIT_BLOCK slots of a block, as the workgroup runs it: at width w = 128, 64, ..., 1 slot t < w takes slot t + w
ERM_MG_FN double ifit_tree_sum(double* slot)
{
    for (int w = IFIT_BLOCK / 2; w > 0; w >>= 1)
        for (int t = 0; t < w; ++t) slot[t] += slot[t + w];
    return slot[0];
}
// The whole reduction of one (item, value) on the host, chunk by chunk as the device goes: value(i) of subject i < N (0 where the subject did not observe the item).
// seen[i], if given, is raised once for every subject a chunk's block takes in: the partition the tests check.  The result does not depend on `chunk`.
template <typename Value>
inline double ifit_reduce(int64_t N, int64_t chunk, Value&& value, int* seen = nullptr)
{
    double total = 0.0;
    for (int64_t c0 = 0; c0 < N; c0 += chunk) {
        const int64_t nc = N - c0 < chunk ? N - c0 : chunk;
        for (int64_t b = 0; b < ifit_blocks(nc); ++b) {               // (c0 is a multiple of IFIT_BLOCK: the chunk's blocks are global blocks)
            double slot[IFIT_BLOCK];
            for (int t = 0; t < IFIT_BLOCK; ++t) {
                const int64_t il = b * IFIT_BLOCK + t;
                slot[t] = il < nc ? value(c0 + il) : 0.0;
                if (il < nc && seen) seen[c0 + il] += 1;
            }
            total += ifit_tree_sum(slot);                             // the block sums in rising block order
        }
    }
    return total;
}

}  // namespace erm

// erm_pv.hpp -- plausible values (include/ertirt.h: erm_get_plausible_values): draws of (theta_i, zeta_i) from each subject's posterior, read off the item
// trace, as PURE functions usable from host and device, beside erm_score.hpp whose row moments and zeta conditional they use.
//
// Draw k = 0..K-1 of subject i uses one row of the table of n_rows item-trace rows and two Philox4x32-10 sites of stream 16:
//     row      r_k = ((2 k + 1) n_rows) / (2 K) in 64-bit integers: evenly spaced, rising with k, distinct when K <= n_rows, each row m times when K = m n_rows   (pv_row)
//     node     Gumbel-max over the rule's nodes: key_q = e_q + g_q, g_q = -log(-log u(w)), u(w) = (w + 1/2) 2^-32, w = word 0 of the block at ctr = {i, k, q, 16 << 24};
//              the largest key wins, of equal keys the smaller q (PvBest, pv_best_add, pv_best_merge): q is chosen with probability w_q = exp(e_q - M) / S.
//              The maximum is associative and the merge symmetric, so the choice does not depend on how the nodes are dealt to lanes.  g lies in [-3.13, 22.87]
//              (the 32-bit uniform), so a node whose weight is below e^-26 of the largest can never be chosen.
//     theta    theta* = theta_q* + sd h (u(w0) - 1/2), uniform within the node's cell; that adds sd^2 h^2 / 12 to the row's variance V, so it is taken out again:
//              c = sqrt(V / (V + sd^2 h^2 / 12)) (0 when V = 0), theta = E + c (theta* - E): mean E and variance V of score_row exactly, the rule's shape.
//     zeta     zeta = c0 + c1 theta + sqrt(u) n, n = sqrt(-2 log u(w1)) cos(2 pi u(w2)), with (c0, c1, u) of score_zeta; w0, w1, w2 = words 0..2 of the block at
//              ctr = {i, k, 0xFFFFFFFF, 16 << 24} (pv_finish).  A model without zeta gets NaN.
// The same header is compiled by g++ with -fsanitize=undefined into tests/pv_check (tests/test_pv_host.py).  No HIP, no allocation, no environment.
#pragma once
#include <cstdint>
#include "erm_score.hpp"

namespace erm {

constexpr int PV_DRAWS_MIN = 1, PV_DRAWS_MAX = 4096, PV_DRAWS_DEFAULT = 5;
constexpr uint32_t PV_SITE = 16;                      // the stream site of the draws (erm_rng.hpp's Site ends at 15, the replicate draws use 14)
constexpr uint32_t PV_FINISH_CTR = 0xFFFFFFFFu;       // the node slot of the block that finishes a draw: no node has this index
constexpr double PV_TWO_PI = 6.283185307179586476925;
constexpr bool pv_draws_ok(long long K) { return K >= PV_DRAWS_MIN && K <= PV_DRAWS_MAX; }

// the row of draw k
ERM_MG_FN long long pv_row(long long k, long long K, long long n_rows) { return ((2 * k + 1) * n_rows) / (2 * K); }

// u(w) in (0, 1), and the Gumbel variate of a word
ERM_MG_FN double pv_uniform(uint32_t w) { return ((double)w + 0.5) * 0x1p-32; }
ERM_MG_FN double pv_gumbel(uint32_t w) { return -log(-log(pv_uniform(w))); }

// the best (key, q) so far; q < 0 is the empty pair (key is then not read)
struct PvBest { double key; int q; };
ERM_MG_FN bool pv_best_before(const PvBest& a, const PvBest& b) { return a.key > b.key || (a.key == b.key && a.q < b.q); }
// two partial maxima; symmetric in its arguments bit for bit (two distinct nodes never share q), so both partners of a butterfly step hold the same pair afterwards.
// (member by member: a choice between whole pairs would be made through their addresses, and on the device that puts them in scratch memory)
ERM_MG_FN PvBest pv_best_merge(const PvBest& a, const PvBest& b)
{
    const bool take_b = b.q >= 0 && (a.q < 0 || pv_best_before(b, a));
    return {take_b ? b.key : a.key, take_b ? b.q : a.q};
}
ERM_MG_FN void pv_best_add(PvBest& a, double key, int q) { a = pv_best_merge(a, PvBest{key, q}); }

// the finish of a draw at node q of the row with moments r (score_row), law w and zeta conditional k (score_zeta); w0, w1, w2: the finishing block's words
struct PvDraw { double theta, zeta; };
ERM_MG_FN PvDraw pv_finish(const ScoreRow& r, const MargLaw& w, const ScoreZeta& k, int q, double h, bool has_zeta, uint32_t w0, uint32_t w1, uint32_t w2)
{
    const double cell = w.sd * h;
    const double star = (w.mu + w.sd * marg_node(q, h)) + cell * (pv_uniform(w0) - 0.5);
    const double c = r.V > 0.0 ? sqrt(r.V / (r.V + cell * cell / 12.0)) : 0.0;
    const double theta = r.E + c * (star - r.E);
    if (!has_zeta) return {theta, NAN};
    const double n = sqrt(-2.0 * log(pv_uniform(w1))) * cos(PV_TWO_PI * pv_uniform(w2));
    return {theta, (k.c0 + k.c1 * theta) + sqrt(k.u) * n};
}

}  // namespace erm

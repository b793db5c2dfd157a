// erm_rank_diag_kernels.hpp -- rank-normalised convergence diagnostics on the device-resident traces: bulk-ESS, tail-ESS and rank-normalised split-R-hat
// (Vehtari, Gelman, Simpson, Carpenter and Buerkner 2021; what MCMCChains 6 / MCMCDiagnosticTools 0.3 report from `ess_rhat`, which the reference's
// checkConvergence, src/SimTools.jl:419-443, pipes Post.ra / rt / qr into).  Included by ertirt.hip behind erm_kernels.hpp (uses the fp64 ndtri of erm_rng.hpp).
//
// The used draws of a column are diag_kernel's: with Tn = nIter - nBurnin and n = floor(Tn / 2) the first n and the last n post-burn-in draws of every chain,
// M = 2 nChain sequences, S = M n pooled draws (always even).  E(.) and R(.) are diag_kernel's ESS and split-R-hat (erm_service_kernels.hpp) of a transformed column:
//   1. r_i   = average rank of x_i among the S pooled draws (ties share the mean of their positions)
//   2. z_i   = ndtri((r_i - 3/8) / (S + 1/4)), fp64 whatever the engine's precision
//   3. ess_bulk = E(z)
//   4. med = (x_(S/2) + x_(S/2+1)) / 2 (order statistics), f_i = |x_i - med|, z' = the normal scores of f
//   5. rhat_rank = max(R(z), R(z')) over those of the two that are defined (f constant: R(z') undefined)
//   6. k = ceil(S / 20); L_i = [x_i <= x_(k)], U_i = [x_i >= x_(S+1-k)]; ess_tail = min(E(L), E(U)), NaN if either indicator column is constant
//   7. a column that never moves: NaN, NaN, NaN
// Two kernels:
//   rank_stage_kernel  the used draws of a chunk of columns, gathered from the trace ([row = m nChain + l][column]: one column is a stride-ld walk) into
//                      a [column][S] scratch of doubles in sequence order (index c n + i), 32 x 32 tiles through LDS: reads coalesced along the columns, writes
//                      along the draws (trace_transpose_kernel's pattern)
//   rank_diag_kernel   ONE WORKGROUP PER COLUMN, the column's work resident in LDS: the (key, position) pairs of a bitonic sorting network padded to a power of
//                      two, the tie runs by a max- / min-scan of the run boundaries, the average ranks scattered back to position order, the normal scores, and
//                      the estimator on z, L, U and z' with the lag sums reduced over the lanes in a FIXED order (lane-strided partial sums, a shuffle tree in
//                      the wave, the waves' sums added in wave order): no atomics, bit-reproducible, independent of the grid and of the other columns.
// LDS: 8 P (keys) + 8 S (series) + 2 P (positions) bytes with P = S rounded up to a power of two -- 144 KB at S = RK_MAX_DRAWS = 8192 (erm_rankdiag.hpp).
#pragma once
#include "erm_kernels.hpp"
#include "erm_rankdiag.hpp"

namespace erm {

constexpr int RK_THREADS = 256, RK_WAVES = RK_THREADS / 64;

// draw s = c n + i of the pooled used draws -> its trace row
__device__ __forceinline__ long long rk_row(int s, int n, int Tn, int nBurnin, int nChain)
{
    const int c = s / n, i = s - c * n;
    return (long long)(nBurnin + ((c & 1) ? Tn - n : 0) + i) * nChain + (c >> 1);
}
template <typename T>
__global__ void __launch_bounds__(256) rank_stage_kernel(const T* tr, long long ld, long long ncol, int nChain, int nBurnin, int Tn, int n, int S, double* dst)
{
    __shared__ double tile[32][33];
    const long long k0 = (long long)blockIdx.x * 32;
    const int s0 = (int)blockIdx.y * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;       // 32 x 8
    for (int r = ty; r < 32; r += 8) {
        const int s = s0 + r; const long long k = k0 + tx;
        if (s < S && k < ncol) tile[r][tx] = (double)tr[rk_row(s, n, Tn, nBurnin, nChain) * ld + k];
    }
    __syncthreads();
    for (int r = ty; r < 32; r += 8) {
        const long long k = k0 + r; const int s = s0 + tx;
        if (k < ncol && s < S) dst[k * S + s] = tile[tx][r];
    }
}

struct RkShared {
    double red[2][RK_WAVES][2];      // block sums: two slots, so that one barrier per sum is enough
    double mu[32];                   // the sequences' means
    int scan[RK_THREADS];
};

__device__ __forceinline__ double rk_wave_sum(double v)
{
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;                        // lane 0 holds the sum
}
// the sums of a and b over the workgroup, in every thread: the wave's shuffle tree, then the waves in order
__device__ __forceinline__ void rk_block_sum2(double& a, double& b, RkShared& sh, int& slot)
{
    a = rk_wave_sum(a); b = rk_wave_sum(b);
    const int lane = (int)threadIdx.x & 63, w = (int)threadIdx.x >> 6;
    if (lane == 0) { sh.red[slot][w][0] = a; sh.red[slot][w][1] = b; }
    __syncthreads();
    a = sh.red[slot][0][0]; b = sh.red[slot][0][1];
    for (int q = 1; q < RK_WAVES; ++q) { a += sh.red[slot][q][0]; b += sh.red[slot][q][1]; }
    slot ^= 1;
}

// bitonic network on the P (key, position) pairs, ascending by (key, position): the position breaks ties, so the padding (key ~0, positions >= S) stays behind
// every draw whatever its key.  THREADS threads, numbered tid = 0 .. THREADS - 1, share the P pairs; the barriers are the workgroup's, so every thread of the
// workgroup calls it with the same P (psis_kernel, erm_psis_kernels.hpp: several groups of a workgroup, each on its own pairs)
template <int THREADS>
__device__ inline void rk_sort_n(uint64_t* key, uint16_t* pos, int P, int tid)
{
    for (int k = 2; k <= P; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
#pragma unroll 1
            for (int t = tid; t < (P >> 1); t += THREADS) {
                const int lo = ((t & ~(j - 1)) << 1) | (t & (j - 1)), hi = lo | j;
                const uint64_t ka = key[lo], kb = key[hi];
                const uint16_t pa = pos[lo], pb = pos[hi];
                const bool gt = ka > kb || (ka == kb && pa > pb);
                if (gt == ((lo & k) == 0)) { key[lo] = kb; key[hi] = ka; pos[lo] = pb; pos[hi] = pa; }
            }
            __syncthreads();
        }
    }
}
__device__ inline void rk_sort(uint64_t* key, uint16_t* pos, int P) { rk_sort_n<RK_THREADS>(key, pos, P, (int)threadIdx.x); }

// the normal score of an average rank, as a REAL call: inlined, the 48 fp64 coefficients of AS 241 are hoisted out of the loop over the draws and held in
// registers across it
__device__ __attribute__((noinline)) double rk_normal_score(double rank, int S) { return ndtri(rk_prob(rank, S)); }

// the sorted (key, position) pairs -> v[position] = the normal score of the draw's average rank.  Tie runs: a thread walks a contiguous piece of the sorted order,
// the last run start before the piece (the first run end behind it) comes from a max- (min-) scan over the threads.
__device__ inline void rk_scores(const uint64_t* key, const uint16_t* pos, double* v, int S, RkShared& sh)
{
    const int tid = (int)threadIdx.x, piece = (S + RK_THREADS - 1) / RK_THREADS;
    const int p0 = min(tid * piece, S), p1 = min(p0 + piece, S);
    int last = -1;
    for (int p = p0; p < p1; ++p) if (p == 0 || key[p] != key[p - 1]) last = p;
    sh.scan[tid] = last;
    for (int off = 1; off < RK_THREADS; off <<= 1) {
        __syncthreads();
        const int o = tid >= off ? sh.scan[tid - off] : -1;
        __syncthreads();
        sh.scan[tid] = max(sh.scan[tid], o);
    }
    __syncthreads();
    int cur = tid > 0 ? sh.scan[tid - 1] : -1;
    for (int p = p0; p < p1; ++p) {
        if (p == 0 || key[p] != key[p - 1]) cur = p;
        v[pos[p]] = (double)cur;                                   // the run's first sorted position; the same thread completes it below
    }
    __syncthreads();
    int first = 0x7fffffff;
    for (int p = p1 - 1; p >= p0; --p) if (p == S - 1 || key[p + 1] != key[p]) first = p;
    sh.scan[tid] = first;
    for (int off = 1; off < RK_THREADS; off <<= 1) {
        __syncthreads();
        const int o = tid + off < RK_THREADS ? sh.scan[tid + off] : 0x7fffffff;
        __syncthreads();
        sh.scan[tid] = min(sh.scan[tid], o);
    }
    __syncthreads();
    cur = tid + 1 < RK_THREADS ? sh.scan[tid + 1] : 0x7fffffff;
#pragma unroll 1
    for (int p = p1 - 1; p >= p0; --p) {
        if (p == S - 1 || key[p + 1] != key[p]) cur = p;
        const int at = pos[p];
        v[at] = rk_normal_score(rk_avg_rank((long long)v[at], cur), S);
    }
    __syncthreads();
}

// diag_kernel's estimator on the series v[c n + i] (centred in place): ess / rhat in every thread, NaN for a series that never moves
__device__ inline void rk_estimate(double* v, int M, int n, bool want_ess, RkShared& sh, int& slot, double& ess, double& rhat)
{
    const int tid = (int)threadIdx.x, lane = tid & 63, w = tid >> 6, S = M * n;
    const double v0 = v[0];
    int differs = 0;
    for (int j = tid; j < S; j += RK_THREADS) differs |= (v[j] != v0) ? 1 : 0;
    if (!__syncthreads_or(differs)) { ess = __builtin_nan(""); rhat = __builtin_nan(""); return; }
    for (int c = w; c < M; c += RK_WAVES) {
        double s = 0.0;
        for (int i = lane; i < n; i += 64) s += v[c * n + i];
        s = rk_wave_sum(s);
        if (lane == 0) sh.mu[c] = s / n;
    }
    __syncthreads();
    double sq = 0.0, unused = 0.0;
    for (int j = tid; j < S; j += RK_THREADS) { const double d = v[j] - sh.mu[j / n]; v[j] = d; sq += d * d; }
    rk_block_sum2(sq, unused, sh, slot);                           // (its barrier also publishes the centred series)
    const double W = sq / (n - 1) / M;
    double mbar = 0.0;
    for (int c = 0; c < M; ++c) mbar += sh.mu[c];
    mbar /= M;
    double Bn = 0.0;
    for (int c = 0; c < M; ++c) Bn += (sh.mu[c] - mbar) * (sh.mu[c] - mbar);
    Bn /= (M - 1);
    const double varp = W * (n - 1) / n + Bn;
    rhat = sqrt(varp / W);
    ess = 0.0;
    if (!want_ess) return;
    double sum = 0.0, prev = 1e300;
    for (int t = 0; t + 1 < n; t += 2) {
        // the lag sums of t and t + 1 over all sequences in one pass: element e = c (n - t) + i pairs draw i of sequence c with draws i + t and i + t + 1
        const int len = n - t, cnt = M * len;
        double a0 = 0.0, a1 = 0.0;
#pragma unroll 2
        for (int e = tid; e < cnt; e += RK_THREADS) {
            const int c = e / len, i = e - c * len;
            const double* d = v + c * n + i;
            const double di = d[0];
            if (t > 0) a0 += di * d[t];
            if (i + 1 < len) a1 += di * d[t + 1];
        }
        rk_block_sum2(a0, a1, sh, slot);
        const double r0 = t == 0 ? 1.0 - (W - W * (n - 1) / n) / varp : 1.0 - (W - a0 / n / M) / varp;
        const double r1 = 1.0 - (W - a1 / n / M) / varp;
        double P = r0 + r1;
        if (!(P > 0.0)) break;
        if (P > prev) P = prev;
        prev = P;
        sum += P;
    }
    ess = (double)M * n / (-1.0 + 2.0 * sum);
}

// xs: [column][S] staged draws (rank_stage_kernel); one workgroup of RK_THREADS per column; dynamic LDS 8 P + 8 S + 2 P bytes
__global__ void __launch_bounds__(RK_THREADS) rank_diag_kernel(const double* xs, int M, int n, int P, double* ess_bulk, double* ess_tail, double* rhat_rank)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char rk_smem[];
    __shared__ RkShared sh;
    const int S = M * n, tid = (int)threadIdx.x;
    uint64_t* key = reinterpret_cast<uint64_t*>(rk_smem);
    double* v = reinterpret_cast<double*>(rk_smem + (size_t)P * 8);
    uint16_t* pos = reinterpret_cast<uint16_t*>(rk_smem + (size_t)P * 8 + (size_t)S * 8);
    const long long col = blockIdx.x;
    const double* x = xs + col * S;
    int slot = 0;

    // four series through one estimator: 0 the normal scores z of x, 1 the lower-tail indicator L, 2 the upper-tail indicator U, 3 the normal scores z' of f
    const int k = (int)rk_tail_k(S);
    double lo = 0.0, hi = 0.0, med = 0.0, bulk = 0.0, el = 0.0, eu = 0.0, rz = 0.0, rf = 0.0;
#pragma unroll 1
    for (int pass = 0; pass < 4; ++pass) {
        if (pass == 0 || pass == 3) {
            for (int p = tid; p < P; p += RK_THREADS) { key[p] = p < S ? rk_key(pass == 0 ? x[p] : fabs(x[p] - med)) : ~0ull; pos[p] = (uint16_t)p; }
            __syncthreads();
            rk_sort(key, pos, P);
            if (pass == 0) { lo = x[pos[k - 1]]; hi = x[pos[S - k]]; med = 0.5 * (x[pos[S / 2 - 1]] + x[pos[S / 2]]); }
            rk_scores(key, pos, v, S, sh);
        } else {
            for (int j = tid; j < S; j += RK_THREADS) v[j] = (pass == 1 ? x[j] <= lo : x[j] >= hi) ? 1.0 : 0.0;
            __syncthreads();
        }
        double e, r;
        rk_estimate(v, M, n, pass < 3, sh, slot, e, r);
        if (pass == 0) { bulk = e; rz = r; } else if (pass == 1) el = e; else if (pass == 2) eu = e; else rf = r;
        __syncthreads();
    }
    if (tid == 0) {
        ess_bulk[col] = bulk;
        ess_tail[col] = (el == el && eu == eu) ? (el < eu ? el : eu) : __builtin_nan("");
        rhat_rank[col] = (rf == rf && rf > rz) ? rf : rz;          // rz is NaN only for a column that never moves, and then so is rf
    }
}

}  // namespace erm

// erm_psis_kernels.hpp -- marginal PSIS-LOO on the device (include/ertirt.h: erm_get_marginal_loo): Pareto-smoothed leave-one-subject-out from the
// subjects' marginal log-likelihoods l_i^(s) that marginal_kernel writes (MargArgs::l_out).  Include after erm_rank_diag_kernels.hpp (rk_sort_n, rk_wave_sum) and
// erm_marginal_kernels.hpp.  The scalar parts -- the tail length, the grid, the fit, the quantile -- are erm_psis.hpp's.
// Three kernels:
//   psis_transpose_kernel  [rows][cols] -> [cols][rows] of doubles through 32 x 33 LDS tiles (trace_transpose_kernel's pattern): marginal_kernel writes l as
//                          [row][subject], the subject fastest, so a subject's column is a stride-N walk; staged, it is S contiguous doubles.  The same kernel
//                          takes the smoothed log-weights back to the caller's layout.
//   psis_kernel<TPS>       TPS = 64, 128 or 256 threads share a subject and a workgroup of 256 carries 256 / TPS subjects: one wave each while the padded length
//                          P = rk_pad(S) <= 2048, two waves up to 4096, the whole workgroup up to 8192 -- 10 P bytes of (key, position) pairs per subject, 80 KB
//                          per workgroup at each upper end, so two workgroups fit the 160 KB of a compute unit.  S is the same for every subject of a call, so every
//                          loop bound and every barrier is uniform over the workgroup; a slot past the last subject repeats it and stores nothing.
//                          Per subject: lw = -l - max(-l) -> keys -> rk_sort's bitonic network by (key, position) -> the M tail slots are overwritten in place by
//                          the exceedances -> lane j < G takes grid point j of the fit (its M log1p in order), every lane finishes the fit -> the tail slots receive
//                          the smoothed values, the others their lw -> four sums over the SORTED order -> elpd, p, k^, n_eff (and lw' - LSE(lw') to position order).
//   psis_totals_kernel     one workgroup: the sums and counts behind out12 over all units.
// SUMS.  A sum over the S sorted slots is taken as 256 lane-strided partial sums (slot p belongs to partial p mod 256, added in rising p), a shuffle tree over each
// run of 64 partials (rk_wave_sum), and the four runs added in order.  With TPS < 256 a thread carries 256 / TPS of the partials, so the order -- and every bit of the
// result -- is the same in the three geometries: the packing is a matter of occupancy only.  No atomics; a subject's result depends on its own column only.
#pragma once
#include "erm_psis.hpp"

namespace erm {

__global__ void __launch_bounds__(256) psis_transpose_kernel(const double* src, long long rows, long long cols, double* dst)
{
    __shared__ double tile[32][33];
    const long long c0 = (long long)blockIdx.x * 32, r0 = (long long)blockIdx.y * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;       // 32 x 8
    for (int r = ty; r < 32; r += 8) if (r0 + r < rows && c0 + tx < cols) tile[r][tx] = src[(r0 + r) * cols + c0 + tx];
    __syncthreads();
    for (int c = ty; c < 32; c += 8) if (c0 + c < cols && r0 + tx < rows) dst[(c0 + c) * rows + r0 + tx] = tile[tx][c];
}

constexpr int PSIS_PARTS = 256, PSIS_RUNS = PSIS_PARTS / 64, PSIS_NV = 4;
struct PsisShared {
    double red[2][4][PSIS_RUNS][PSIS_NV];          // [slot][subject of the workgroup][run of 64 partials][value]
    double L[4][PSIS_MAX_GRID], b[4][PSIS_MAX_GRID];
};

// part[q][v]: this thread's partial number t + TPS q of value v.  SUM: the order of the header; otherwise the maximum.  The result in every thread of the group.
template <int TPS, bool SUM>
__device__ __forceinline__ void psis_group_reduce(double (&part)[256 / TPS][PSIS_NV], double (&out)[PSIS_NV], PsisShared& sh, int& slot, int g, int t)
{
    constexpr int NPL = 256 / TPS, WPS = TPS / 64;
    const int lane = t & 63, wl = t >> 6;
#pragma unroll
    for (int q = 0; q < NPL; ++q)
#pragma unroll
        for (int v = 0; v < PSIS_NV; ++v) {
            double a = part[q][v];
            if constexpr (SUM) a = rk_wave_sum(a);
            else for (int off = 32; off > 0; off >>= 1) a = fmax(a, __shfl_down(a, off, 64));
            if (lane == 0) sh.red[slot][g][wl + WPS * q][v] = a;
        }
    __syncthreads();
#pragma unroll
    for (int v = 0; v < PSIS_NV; ++v) {
        double a = sh.red[slot][g][0][v];
        for (int r = 1; r < PSIS_RUNS; ++r) a = SUM ? a + sh.red[slot][g][r][v] : fmax(a, sh.red[slot][g][r][v]);
        out[v] = a;
    }
    slot ^= 1;
}

struct PsisArgs {
    double* xs;                    // [subject of the chunk][S]: the staged l; receives lw' - LSE(lw') in position order if want_lw
    long long n;                   // subjects of the chunk
    int S, P;                      // rows and the sort's padded length
    double* pw;                    // [PSIS_DEV_COLS][n_all] (column-major [n_all][PSIS_DEV_COLS]): this chunk's subjects start at pw + c0
    long long n_all, c0;
    int want_lw;
};
constexpr int PSIS_LPPD = PSIS_COLS, PSIS_DEV_COLS = PSIS_COLS + 1;      // the device table carries lppd_i beside the four public columns

// dynamic LDS: (256 / TPS) * 10 P bytes -- the keys of all the workgroup's subjects, then their positions
template <int TPS>
__global__ void __launch_bounds__(256) psis_kernel(const PsisArgs A)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char psis_smem[];
    __shared__ PsisShared sh;
    constexpr int NS = 256 / TPS, NPL = 256 / TPS;
    const int S = A.S, P = A.P, tid = (int)threadIdx.x, g = tid / TPS, t = tid - g * TPS;
    uint64_t* key = reinterpret_cast<uint64_t*>(psis_smem) + (size_t)g * P;
    double* val = reinterpret_cast<double*>(key);                                   // the same slots once they hold doubles
    uint16_t* pos = reinterpret_cast<uint16_t*>(psis_smem + (size_t)NS * P * 8) + (size_t)g * P;
    const long long i0 = (long long)blockIdx.x * NS + g;
    const bool live = i0 < A.n;
    const long long i = live ? i0 : A.n - 1;
    double* l = A.xs + i * S;
    int slot = 0;
    double part[NPL][PSIS_NV], r[PSIS_NV];
    const double ninf = -(double)INFINITY;

    // ---- max(-l) and max(l)
#pragma unroll
    for (int q = 0; q < NPL; ++q) {
        double a = ninf, b = ninf;
        for (int p = t + TPS * q; p < S; p += PSIS_PARTS) { const double v = l[p]; a = fmax(a, -v); b = fmax(b, v); }
        part[q][0] = a; part[q][1] = b; part[q][2] = ninf; part[q][3] = ninf;
    }
    psis_group_reduce<TPS, false>(part, r, sh, slot, g, t);
    const double mx = r[0], lmax = r[1];

    // ---- the log ratios in sorted order
    for (int p = t; p < P; p += TPS) { key[p] = p < S ? rk_key(-l[p] - mx) : ~0ull; pos[p] = (uint16_t)p; }
    __syncthreads();
    rk_sort_n<TPS>(key, pos, P, t);

    // ---- the tail: slots T0 .. S - 1; the exceedances take the keys' place
    const int M = psis_tail_len(S), G = psis_grid(M), T0 = S - M;
    const double c = psis_unkey(key[T0 - 1]), expc = exp(c);
    for (int p = T0 + t; p < S; p += TPS) val[p] = exp(psis_unkey(key[p])) - expc;
    __syncthreads();
    const double* x = val + T0;
    const bool fittable = psis_fittable(x, M);
    if (t < G) {
        double bj = 0.0, Lj = 0.0;
        if (fittable) { bj = psis_b(t + 1, G, x[M - 1], x[psis_xstar(M)]); Lj = psis_profile(bj, psis_mean_log1p(bj, x, M), M); }
        sh.b[g][t] = bj; sh.L[g][t] = Lj;
    }
    __syncthreads();
    const PsisFit fit = psis_finish(sh.L[g], sh.b[g], G, x, M);
    __syncthreads();                                               // every lane has read the exceedances

    // ---- every slot receives its final log-weight as a double
    for (int p = t; p < S; p += TPS) val[p] = p < T0 ? psis_unkey(key[p]) : (fit.ok ? psis_smooth(p - T0 + 1, M, expc, fit.khat, fit.sigma) : -l[pos[p]] - mx);
    __syncthreads();

    // ---- max(lw') and max(lw' + l), then the four sums, over the sorted slots
#pragma unroll
    for (int q = 0; q < NPL; ++q) {
        double a = ninf, b = ninf;
        for (int p = t + TPS * q; p < S; p += PSIS_PARTS) { const double w = val[p]; a = fmax(a, w); b = fmax(b, w + l[pos[p]]); }
        part[q][0] = a; part[q][1] = b; part[q][2] = ninf; part[q][3] = ninf;
    }
    psis_group_reduce<TPS, false>(part, r, sh, slot, g, t);
    const double m1 = r[0], m2 = r[1];
#pragma unroll
    for (int q = 0; q < NPL; ++q) {
        double s1 = 0.0, s1q = 0.0, s2 = 0.0, s3 = 0.0;
        for (int p = t + TPS * q; p < S; p += PSIS_PARTS) {
            const double w = val[p], lv = l[pos[p]], e = exp(w - m1);
            s1 += e; s1q += e * e; s2 += exp(w + lv - m2); s3 += exp(lv - lmax);
        }
        part[q][0] = s1; part[q][1] = s1q; part[q][2] = s2; part[q][3] = s3;
    }
    psis_group_reduce<TPS, true>(part, r, sh, slot, g, t);         // (its barrier: every read of l is done before lw' goes over it)
    const double lse1 = m1 + log(r[0]);
    const double elpd = (m2 + log(r[2])) - lse1, lppd = lmax + log(r[3] / (double)S);
    if (live && A.want_lw) for (int p = t; p < S; p += TPS) l[pos[p]] = val[p] - lse1;
    if (live && t == 0) {
        double* o = A.pw + A.c0 + i;
        o[PSIS_ELPD * A.n_all] = elpd; o[PSIS_P * A.n_all] = lppd - elpd; o[PSIS_KHAT * A.n_all] = fit.khat; o[PSIS_NEFF * A.n_all] = r[0] * r[0] / r[1];
        o[PSIS_LPPD * A.n_all] = lppd;
    }
}

// out8 = { sum elpd, sum p, sum lppd, sum (elpd_u - mean)^2, #(k^ > 0.7), #(k^ > k_thr), 0, 0 } over the n units of pw: thread t adds its units t, t + 256, ... in
// order, a shuffle tree adds the wave's lanes, the four waves are added in order (one workgroup)
__global__ void __launch_bounds__(256) psis_totals_kernel(const double* pw, long long n, double k_thr, double* out8)
{
    __shared__ double red[2][4][4];
    const int tid = (int)threadIdx.x, lane = tid & 63, w = tid >> 6;
    const double* el = pw + PSIS_ELPD * n; const double* pp = pw + PSIS_P * n; const double* kh = pw + PSIS_KHAT * n; const double* lp = pw + PSIS_LPPD * n;
    double a[4] = {0.0, 0.0, 0.0, 0.0}, c[4] = {0.0, 0.0, 0.0, 0.0};
    for (long long u = tid; u < n; u += 256) { a[0] += el[u]; a[1] += pp[u]; a[2] += lp[u]; c[1] += kh[u] > PSIS_K_BAD ? 1.0 : 0.0; c[2] += kh[u] > k_thr ? 1.0 : 0.0; }
    for (int v = 0; v < 4; ++v) { a[v] = rk_wave_sum(a[v]); if (lane == 0) red[0][w][v] = a[v]; }
    __syncthreads();
    for (int v = 0; v < 4; ++v) a[v] = ((red[0][0][v] + red[0][1][v]) + red[0][2][v]) + red[0][3][v];
    const double mean = a[0] / (double)n;
    for (long long u = tid; u < n; u += 256) { const double d = el[u] - mean; c[0] += d * d; }
    for (int v = 0; v < 4; ++v) { c[v] = rk_wave_sum(c[v]); if (lane == 0) red[1][w][v] = c[v]; }
    __syncthreads();
    for (int v = 0; v < 4; ++v) c[v] = ((red[1][0][v] + red[1][1][v]) + red[1][2][v]) + red[1][3][v];
    if (tid == 0) { out8[0] = a[0]; out8[1] = a[1]; out8[2] = a[2]; out8[3] = c[0]; out8[4] = c[1]; out8[5] = c[2]; out8[6] = 0.0; out8[7] = 0.0; }
}

}  // namespace erm

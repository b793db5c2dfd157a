// erm_service_kernels.hpp -- the kernels around the sweep: convergence diagnostics, data preparation, the data generator, run begin / end, DIC, the
// diagnostic counters and the debug samplers.  Included by erm_kernels.hpp behind the sweep (uses its Ctl, reduce_rows and the samplers of erm_rng.hpp).
#pragma once
#include "erm_kernels.hpp"

namespace erm {

// ---------------------------------------------------------------------------------------------------------------------
// Convergence diagnostics on the device-resident traces (the reference pulls Post.ra/rt/qr through MCMCChains'
// ess_rhat in checkConvergence, src/SimTools.jl:419-443): split-R-hat and the effective sample size by Geyer's initial monotone
// sequence over the split chains (Gelman et al., BDA3 sec. 11.4-11.5; the non-rank-normalised estimator), one thread per parameter.
//   draws: trace row (m * nChain + l), m >= nBurnin; each chain l is split into its first and last n = floor((nIter - nBurnin)/2)
//   draws  => M = 2 nChain sequences.  W = mean of the sequences' variances (n-1 denominator), B/n = variance of their means,
//   var+ = (n-1)/n W + B/n, rhat = sqrt(var+ / W), rho_t = 1 - (W - mean_c acov_c(t)) / var+ with acov_c(t) = 1/n sum_i (x_i - mu_c)
//   (x_{i+t} - mu_c); P_k = rho_{2k} + rho_{2k+1} summed while positive and made non-increasing; ess = M n / (-1 + 2 sum_k P_k).
// A parameter that never moves (beta[1] = 0, Sigma_p[1,1] = 1 ...) gets NaN, as MCMCChains reports it.  "Never moves" means that every used draw (the 2 n
// draws of every chain; an odd length leaves the middle one out) equals the first one: decided on the draws themselves, not by W > 0, because the rounded mean of n
// copies of a non-dyadic constant is not that constant and leaves a W of rounding noise (gibbs.ess_rhat carries the same rule).  The sampler's constant columns hold 0
// or 1, whose sums are exact, so on a device trace the two rules agree: the difference shows on host traces only.
// The sum over k stops BEFORE the first P_k that is not positive, P_0 included: a column whose first pair sum is not positive gets -M n (sum = 0, so the denominator
// is -1); x_i = (-1)^i is such a column.  More generally the value is negative whenever the pair sums add up to less than 1 / 2, which sampler traces with n = 4 .. 8
// draws per sequence do show.  The estimator is left as it is; a caller that counts "ESS defined" counts such a column too.
// ---------------------------------------------------------------------------------------------------------------------
constexpr int DIAG_MAXSEQ = 32;
// Subject-sharded chains: a device's reduced statistics (the nb group rows of a pass) summed into ONE row, the unit the devices
// all-gather before every tiny step; reduce_rows order, so the result does not depend on the launch geometry of this kernel
__global__ void __launch_bounds__(256) shard_pack_kernel(const double* gslab, int nb, int NS, double* out)
{
    reduce_rows(gslab, nb, NS, out, (int)threadIdx.x, (int)blockDim.x);
}

// erm_set_data on the device.  The caller's arrays are column-major (Julia): uploaded as they are, then
//   colstats_cm_kernel : one workgroup per column j: K0_j = sum_i (Y_ij - 1/2), sum_i logT_ij (fp64, fixed order), validity flags
//                        (bit 0: a Y that is not 0/1, bit 1: a non-finite logT);
//   to_rows_kernel     : 32 x 32 tiles through LDS, dst[i][j] = (T)(src[j][i] - shift[j]) -- Y bytes, logT centred by its column mean
//                        (subtracted in fp64 BEFORE the value is rounded to the engine's cell type), X;
//   colsq_kernel       : per-workgroup partial sums over rows of the squared centred values ([block][J]).
__global__ void __launch_bounds__(256) colstats_cm_kernel(const uint8_t* Y, const double* L, long long N, int has_l, double* out, int J, unsigned int* flags)
{
    const int j = blockIdx.x, tid = threadIdx.x;
    double sk = 0.0, sl = 0.0;
    unsigned int bad = 0u;
    for (long long i = tid; i < N; i += 256) {
        const uint8_t y = Y[(size_t)j * N + i];
        bad |= (y > 1) ? 1u : 0u;
        sk += (double)y - 0.5;
        if (has_l) { const double v = L[(size_t)j * N + i]; bad |= (fabs(v) < 1.79e308) ? 0u : 2u; sl += v; }
    }
    __shared__ double shk[256], shl[256];
    shk[tid] = sk; shl[tid] = sl;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) { if (tid < w) { shk[tid] += shk[tid + w]; shl[tid] += shl[tid + w]; } __syncthreads(); }
    if (tid == 0) { out[j] = shk[0]; out[J + j] = shl[0]; }
    if (bad) atomicOr(flags, bad);
}
template <typename S, typename T>
__global__ void __launch_bounds__(256) to_rows_kernel(const S* src, long long N, int J, const double* shift, T* dst)
{
    __shared__ double tile[32][33];
    const long long i0 = (long long)blockIdx.x * 32;
    const int j0 = (int)blockIdx.y * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    for (int r = ty; r < 32; r += 8) {
        const int j = j0 + r; const long long i = i0 + tx;
        if (j < J && i < N) tile[r][tx] = (double)src[(size_t)j * N + i] - (shift ? shift[j] : 0.0);
    }
    __syncthreads();
    for (int r = ty; r < 32; r += 8) {
        const long long i = i0 + r; const int j = j0 + tx;
        if (i < N && j < J) dst[(size_t)i * J + j] = (T)tile[tx][r];
    }
}
template <typename real>
__global__ void __launch_bounds__(128) colsq_kernel(const real* C, long long N, int J, double* part)
{
    const long long per = (N + gridDim.x - 1) / gridDim.x, r0 = (long long)blockIdx.x * per, r1 = (r0 + per < N) ? r0 + per : N;
    for (int j = threadIdx.x; j < J; j += blockDim.x) {
        double sq = 0.0;
        for (long long i = r0; i < r1; ++i) { const double c = (double)C[(size_t)i * J + j]; sq += c * c; }
        part[(size_t)blockIdx.x * J + j] = sq;
    }
}

// Post.ra / rt / qr in Julia layout: the device keeps a subject-level trace as [row = m * nChain + l][subject] (coalesced stores, one row per
// sweep); Julia's array is [nIter][width][nChain] with the iteration fastest.  dst[i * nIter + m] = (double) src[(m * nChain + l) * ld + i] for ONE
// chain l, 32 x 32 tiles through LDS so that both the reads (along subjects) and the writes (along iterations) are coalesced.
template <typename T>
__global__ void __launch_bounds__(256) trace_transpose_kernel(const T* src, long long ld, long long ncol, int nIter, int nChain, int l, double* dst)
{
    __shared__ double tile[32][33];
    const long long i0 = (long long)blockIdx.x * 32;
    const int m0 = (int)blockIdx.y * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;       // 32 x 8
    for (int r = ty; r < 32; r += 8) {
        const int m = m0 + r; const long long i = i0 + tx;
        if (m < nIter && i < ncol) tile[r][tx] = (double)src[((long long)m * nChain + l) * ld + i];
    }
    __syncthreads();
    for (int r = ty; r < 32; r += 8) {
        const long long i = i0 + r; const int m = m0 + tx;
        if (i < ncol && m < nIter) dst[i * nIter + m] = tile[tx][r];
    }
}

// dst[i] += src[i] (chain farms: post-burn-in sums of the chains that share a device, before the RCCL all-reduce over the devices)
__global__ void __launch_bounds__(256) acc_kernel(double* dst, const double* src, long long n)
{
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) dst[i] += src[i];
}

template <typename T>
__global__ void diag_kernel(const T* tr, long long ncol, long long ld, int nIter, int nChain, int nBurnin, double* ess, double* rhat)
{
    const long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= ncol) return;
    const int Tn = nIter - nBurnin, n = Tn / 2, M = 2 * nChain;
    auto at = [&](int c, int i) -> double {                      // draw i of split sequence c
        const int l = c >> 1, m0 = nBurnin + ((c & 1) ? Tn - n : 0);
        return (double)tr[((long long)(m0 + i) * nChain + l) * ld + k];
    };
    double mu[DIAG_MAXSEQ];
    double W = 0.0, mbar = 0.0;
    const double x0 = at(0, 0);
    bool moves = false;                                          // some used draw differs from the first one
    for (int c = 0; c < M; ++c) {
        double s1 = 0.0;
        for (int i = 0; i < n; ++i) { const double x = at(c, i); moves = moves || (x != x0); s1 += x; }
        mu[c] = s1 / n; mbar += mu[c];
        double s2 = 0.0;
        for (int i = 0; i < n; ++i) { const double d = at(c, i) - mu[c]; s2 += d * d; }
        W += s2 / (n - 1);
    }
    W /= M; mbar /= M;
    double Bn = 0.0;
    for (int c = 0; c < M; ++c) Bn += (mu[c] - mbar) * (mu[c] - mbar);
    Bn /= (M - 1);
    const double varp = W * (n - 1) / n + Bn;
    if (!moves) { ess[k] = __builtin_nan(""); rhat[k] = __builtin_nan(""); return; }
    rhat[k] = sqrt(varp / W);
    auto rho = [&](int t) -> double {
        double a = 0.0;
        for (int c = 0; c < M; ++c) {
            double s = 0.0;
            for (int i = 0; i + t < n; ++i) s += (at(c, i) - mu[c]) * (at(c, i + t) - mu[c]);
            a += s / n;
        }
        return 1.0 - (W - a / M) / varp;
    };
    double sum = 0.0, prev = 1e300;
    for (int t = 0; t + 1 < n; t += 2) {
        double P = (t == 0 ? 1.0 - (W - W * (n - 1) / n) / varp : rho(t)) + rho(t + 1);
        if (!(P > 0.0)) break;
        if (P > prev) P = prev;
        prev = P;
        sum += P;
    }
    ess[k] = (double)M * n / (-1.0 + 2.0 * sum);
}

// Chain farm, joint diagnostics: the post-burn-in rows of nc columns of ONE chain's trace block (src: the chunk's first column in row 0 of the
// block, rows ld apart) into slot l of the interleaved scratch the estimator kernels read as a trace of L chains without burn-in:
//   dst[((m - nBurnin) L + l) nc + k] = src[m ld + k],   m = nBurnin .. nBurnin + Tn - 1,  k = 0 .. nc - 1.
// With L = 1, l = 0 the same kernel compacts the rows into the slab [Tn][nc] that crosses to chain 0's device when the chain lives elsewhere.  Rows go over
// blockIdx.y, columns over blockIdx.x and the lanes (both grid-stride): reads and writes are coalesced along the columns, 16 bytes a lane where the chunk length,
// the row stride and both base addresses allow (a wave-uniform choice), one element a lane otherwise.  One writer per element, no atomics.
template <typename T>
__global__ void __launch_bounds__(256) farm_gather_kernel(const T* src, long long ld, long long nc, int Tn, int nBurnin, int L, int l, T* dst)
{
    constexpr int V = 16 / (int)sizeof(T);
    const bool wide = nc % V == 0 && ld % V == 0 && ((reinterpret_cast<unsigned long long>(src) | reinterpret_cast<unsigned long long>(dst)) & 15ull) == 0ull;
    const long long k0 = (long long)blockIdx.x * blockDim.x + threadIdx.x, kstep = (long long)gridDim.x * blockDim.x;
    for (int r = (int)blockIdx.y; r < Tn; r += (int)gridDim.y) {
        const T* s = src + (long long)(nBurnin + r) * ld;
        T* d = dst + ((long long)r * L + l) * nc;
        if (wide) {
            const uint4* s4 = reinterpret_cast<const uint4*>(s);
            uint4* d4 = reinterpret_cast<uint4*>(d);
            for (long long k = k0; k < nc / V; k += kstep) d4[k] = s4[k];
        } else {
            for (long long k = k0; k < nc; k += kstep) d[k] = s[k];
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// Synthetic data on the device: the generators of src/SimTools.jl -- setDataRtIrt :149-178, setDataRtIrtNull
// :117-144, setDataMlIrt :349-368, setDataRtIrtCross :220-255, setDataRtIrtLatent :304-343 -- written straight into the engine's
// resident buffers, one thread per subject.  Streams (DATA_SUBJ, i) / (DATA_CELL, i, j) of the data seed: like the host generators,
// this is the reference's distribution, not Julia's Random.seed! stream.
//   gen 0 MlIrt : X[:,1] ~ Bernoulli(1/2), X[:,2:] ~ N(0,1), theta ~ N(X beta, 1)
//   gen 1 RtIrt : X ~ N(0,1), (theta, zeta) = X beta + N2(0, Sigp), logT ~ N(lambda_j - zeta_i, sig2t_j) truncated to (0, inf)
//   gen 2 Null  : (theta, zeta) ~ N2(0, Sigp), logT as RtIrt
//   gen 3 Cross : (theta, zeta) ~ N2(0, Sigp), logT = lambda_j - zeta_i - theta_i rho_j + e
//   gen 4 Latent: theta ~ N(0,1), X ~ N(0,1), zeta = [X theta] beta + e, logT = lambda_j - zeta_i + N(0,1)
//   e ("noise"): 0 N(0, 0.3), 1 t_5, 2 Gamma(1/2, 1) - 1   (the 0.3 belongs to the normal type only: src/SimTools.jl:238-247)
// Y_ij ~ Bernoulli(logistic(a_j (theta_i - b_j))) always.  logT is written raw; center_kernel subtracts the column means afterwards.
// ---------------------------------------------------------------------------------------------------------------------
struct GenArgs {
    uint8_t* Y; void* C; void* X; double* theta; double* zeta;   // C, X in the engine's cell type
    const double* truth;       // a[J] b[J] lambda[J] sig2t[J] rho[J] | Sigp chol L00 L10 L11 | beta (RtIrt: [F][2] row-major; MlIrt [F]; Latent [F+1])
    long long N; int J, F, gen, noise; uint64_t seed;
};
__device__ inline double gen_noise(Stream& s, int kind)      // src/SimTools.jl:238-247, 322-328: Normal(0, 0.3) | TDist(5) | Gamma(1/2, 1) - 1
{
    if (kind == 0) return 0.3 * normal<double>(s);
    if (kind == 1) { const double zn = normal<double>(s); return zn / sqrt(chisq(s, 5.0) / 5.0); }
    const double u = uniform<double>(s);
    const double g = gamma_mt(s, 1.5) * u * u;                            // Gamma(a) = Gamma(a + 1) U^(1/a), a = 1/2 (Marsaglia-Tsang needs a >= 1)
    return g - 1.0;
}
template <typename real>
__global__ void gen_kernel(GenArgs G)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= G.N) return;
    const int J = G.J, F = G.F;
    const double* a = G.truth, *b = a + J, *lam = b + J, *sg = lam + J, *rho = sg + J, *L = rho + J, *beta = L + 3;
    real* X = reinterpret_cast<real*>(G.X);
    real* C = reinterpret_cast<real*>(G.C);
    Stream ss(G.seed, 0u, SITE_DATA_SUBJ, (uint32_t)i, 0u, 0u);
    double mt = 0.0, mz = 0.0;
    for (int f = 0; f < F; ++f) {
        double x = normal<double>(ss);
        if (G.gen == 0 && f == 0) x = uniform<double>(ss) < 0.5 ? 1.0 : 0.0;
        const real xr = (real)x;                          // the model sees the stored value
        X[(size_t)i * F + f] = xr;
        if (G.gen == 0) mt += (double)xr * beta[f];
        else if (G.gen == 1) { mt += (double)xr * beta[2 * f]; mz += (double)xr * beta[2 * f + 1]; }
        else if (G.gen == 4) mz += (double)xr * beta[f];
    }
    const double z0 = normal<double>(ss), z1 = normal<double>(ss);
    double th, ze;
    if (G.gen == 0) { th = mt + z0; ze = 0.0; }
    else if (G.gen == 4) { th = z0; ze = mz + th * beta[F] + gen_noise(ss, G.noise); }
    else { th = mt + L[0] * z0; ze = mz + L[1] * z0 + L[2] * z1; }
    G.theta[i] = th; G.zeta[i] = ze;
    for (int j = 0; j < J; ++j) {
        Stream sc(G.seed, 0u, SITE_DATA_CELL, (uint32_t)i, (uint32_t)j, 0u);
        const double eta = a[j] * (th - b[j]);
        G.Y[(size_t)i * J + j] = uniform<double>(sc) < 1.0 / (1.0 + exp(-eta)) ? 1 : 0;
        if (G.gen == 0) continue;
        double lt;
        if (G.gen == 1 || G.gen == 2) lt = truncnorm0(sc, lam[j] - ze, sqrt(sg[j]));
        else if (G.gen == 3) lt = lam[j] - ze - th * rho[j] + gen_noise(sc, G.noise);
        else lt = lam[j] - ze + normal<double>(sc);
        C[(size_t)i * J + j] = (real)lt;
    }
}
// per-workgroup partial column sums of the generated data: [block][3][J] = sum kappa, sum logT, sum logT^2 (fp64), then x'x partials
template <typename real>
__global__ void colsum_kernel(const uint8_t* Y, const real* C, const real* X, long long N, int J, int F, int has_c, double* part)
{
    const long long per = (N + gridDim.x - 1) / gridDim.x, r0 = (long long)blockIdx.x * per, r1 = (r0 + per < N) ? r0 + per : N;
    const int p = F + 1;
    double* out = part + (size_t)blockIdx.x * (3 * J + p * p);
    for (int j = threadIdx.x; j < J; j += blockDim.x) {
        double sk = 0.0, s1 = 0.0, s2 = 0.0;
        for (long long i = r0; i < r1; ++i) {
            sk += (double)Y[(size_t)i * J + j] - 0.5;
            if (has_c) { const double c = (double)C[(size_t)i * J + j]; s1 += c; s2 += c * c; }
        }
        out[j] = sk; out[J + j] = s1; out[2 * J + j] = s2;
    }
    for (int e = threadIdx.x; e < p * p; e += blockDim.x) {
        const int u = e % p, v = e / p;
        double t = 0.0;
        for (long long i = r0; i < r1; ++i) {
            const double xu = u == 0 ? 1.0 : (double)X[(size_t)i * F + u - 1], xv = v == 0 ? 1.0 : (double)X[(size_t)i * F + v - 1];
            t += xu * xv;
        }
        out[3 * J + e] = t;
    }
}
// logT -> logT - column mean, and the centred sums of squares per workgroup ([block][J])
template <typename real>
__global__ void center_kernel(real* C, long long N, int J, const double* mean, double* part)
{
    const long long per = (N + gridDim.x - 1) / gridDim.x, r0 = (long long)blockIdx.x * per, r1 = (r0 + per < N) ? r0 + per : N;
    for (int j = threadIdx.x; j < J; j += blockDim.x) {
        const double m = mean[j];
        double sq = 0.0;
        for (long long i = r0; i < r1; ++i) {
            const double c = (double)C[(size_t)i * J + j] - m;
            const real cr = (real)c;
            C[(size_t)i * J + j] = cr;
            sq += (double)cr * (double)cr;
        }
        part[(size_t)blockIdx.x * J + j] = sq;
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// erm_run's bookkeeping in two small launches.  As separate stream operations (two host -> device copies of the counters, a fill of the tickets, three
// device -> host copies at the end) they were ~45 us of device time per erm_run -- more than two microseconds per sweep of a 20-sweep call.
//   run_begin_kernel : both copies of the chain's counters, the group tickets zeroed, the persistent launch's wait bound and test hook;
//   run_end_kernel   : the counters of both buffers and the time-out word into PINNED HOST memory (visible to the host once the stream has drained).
// ---------------------------------------------------------------------------------------------------------------------
// (the call's parameters come from PINNED HOST memory the host fills before it enqueues the call: the kernel's arguments never change, so it can sit at the head of a
// replayed graph that holds the whole call -- erm_run: whole_graph)
struct RunParams { Ctl v; unsigned int tmo_ticks, tmo_fault; };
__global__ void __launch_bounds__(256) run_begin_kernel(Ctl* c0, Ctl* c1, const RunParams* hp, unsigned int* gcnt, int n_gcnt)
{
    const int t = (int)threadIdx.x;
    const RunParams rp = *hp;
    if (t == 0) { *c0 = rp.v; *c1 = rp.v; }
    for (int k = t; k < n_gcnt; k += (int)blockDim.x) gcnt[k] = (k == n_gcnt - 3) ? rp.tmo_ticks : ((k == n_gcnt - 2) ? rp.tmo_fault : 0u);      // [tickets | tmo flag, ticks, fault, pad]
}
__global__ void __launch_bounds__(64) run_end_kernel(const Ctl* c0, const Ctl* c1, const unsigned int* tmo, Ctl* host_out, unsigned int* host_tmo)
{
    if (threadIdx.x == 0) { host_out[0] = *c0; host_out[1] = *c1; *host_tmo = *tmo; }
}
// up to 10 device buffers copied by ONE launch: the state a persistent erm_run saves before it starts (and restores if the launch times out)
struct CopySegs { const void* src[10]; void* dst[10]; unsigned long long bytes[10]; int n; };
__global__ void __launch_bounds__(256) copy_segments_kernel(CopySegs S)
{
    const size_t gt = (size_t)blockIdx.x * blockDim.x + threadIdx.x, gn = (size_t)gridDim.x * blockDim.x;
    for (int k = 0; k < S.n; ++k) {
        const size_t nb = (size_t)S.bytes[k], nw = nb / 16;                       // hipMalloc'd buffers: 256-byte aligned
        const uint4* s = reinterpret_cast<const uint4*>(S.src[k]);
        uint4* d = reinterpret_cast<uint4*>(S.dst[k]);
        for (size_t i = gt; i < nw; i += gn) d[i] = s[i];
        for (size_t i = nw * 16 + gt; i < nb; i += gn) reinterpret_cast<unsigned char*>(S.dst[k])[i] = reinterpret_cast<const unsigned char*>(S.src[k])[i];
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// DIC on the device.  getDic (src/GibbsRtIrt.pl.jl:432-472, src/GibbsRtIrtCross.pl.jl:330-353, src/GibbsRtIrtLatent.pl.jl:342-365):
//   Dhat = -2 logLik(Post.mean), Dbar = -2 mean(Post.logLike) over all iterations, pD = Dbar - Dhat, DIC = Dbar + pD.
// Post.mean never leaves the device: the post-burn-in SUMS of the subject-level draws are resident (sum_theta / sum_zeta / sum_nu), the item-level
// ones are summed from the resident item trace (item_sum_kernel, row order), and loglik_kernel evaluates the model's log-likelihood
//   getLogLikelihoodMlIrt / RtIrt / RtIrtNull (src/GibbsRtIrt.pl.jl:195-204, 262-272, 351-362), ...Cross / CrossQr (src/GibbsRtIrtCross.pl.jl:158-170, 240-258),
//   ...Latent / LatentQr (src/GibbsRtIrtLatent.pl.jl:151-162, 243-264)
// at sums * inv over the resident data set.  Plain fp64 with libm's log1p / exp / log (this runs once per sample!, not per sweep); every thread adds its
// terms in a fixed order, a workgroup's threads are summed by a fixed tree, the host adds the workgroups' partial sums in order: reproducible bit for bit.
// `sum` layout (the chain farm's summary vector): [item-level trace columns: a b lambda sig2t | small part of qr][theta N][zeta N, response-time models][nu N or N*J].
// ---------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) item_sum_kernel(const double* tr_item, long long wi, long long row0, long long row1, double* out)
{
    const long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= wi) return;
    double t = 0.0;
    for (long long r = row0; r < row1; ++r) t += tr_item[r * wi + k];
    out[k] += t;
}
// sum of the first n entries of the log-likelihood trace: thread t adds entries t, t + 256, ... in order, then a fixed tree
__global__ void __launch_bounds__(256) ll_trace_sum_kernel(const double* tr_ll, long long n, double* out)
{
    __shared__ double sh[256];
    double t = 0.0;
    for (long long r = threadIdx.x; r < n; r += 256) t += tr_ll[r];
    sh[threadIdx.x] = t;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) { if ((int)threadIdx.x < w) sh[threadIdx.x] += sh[threadIdx.x + w]; __syncthreads(); }
    if (threadIdx.x == 0) *out = sh[0];
}
struct LogLikArgs {
    const uint8_t* Y; const void* C; const void* X;      // resident data set: Y u8 [N][J], centred logT and X in the engine's cell type, row-major
    const double* cm;                                     // column means of logT [J]
    const double* sum; double inv;                        // Post.mean = sum * inv
    long long N; int J, F, model;                         // F = covariate columns the kernels see
    long long off_theta, off_zeta, off_nu;                // offsets into `sum` (off_zeta / off_nu < 0: absent)
    double k1, k2;
    long long rows_per_block;
    double* part;                                         // [gridDim.x]
};
template <typename real>
__global__ void __launch_bounds__(256) loglik_kernel(LogLikArgs D)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    double* sa = reinterpret_cast<double*>(smem);        // a b lambda sig2t rho [5][J] | Sigp [4] | beta [2 PMAX]
    const int J = D.J, F = D.F, p = F + 1, M = D.model, tid = (int)threadIdx.x;
    double* sb = sa + J, *sl = sa + 2 * J, *sg = sa + 3 * J, *sr = sa + 4 * J, *sS = sa + 5 * J, *sbeta = sS + 4;
    __shared__ double red[256];
    for (int e = tid; e < 4 * J; e += 256) sa[e] = D.sum[e] * D.inv;
    const double* q = D.sum + 4 * J;                      // the small part of qr (tiny_publish's order)
    // the small part's offsets and beta's slots come from the per-model table (erm_model.hpp); F is the number of columns the kernels see
    for (int j = tid; j < J; j += 256) sr[j] = model_traits(M).rho ? q[j] * D.inv : 0.0;
    if (tid < 4) sS[tid] = !model_traits(M).rt ? (tid == 0 || tid == 3 ? 1.0 : 0.0) : q[qr_sigp_off(M, J, F) + tid] * D.inv;
    if (tid < 2 * PMAX) { const int u = beta_slot_src(model_traits(M).beta, F, tid); sbeta[tid] = u >= 0 ? q[u] * D.inv : 0.0; }
    __syncthreads();
    const real* C = reinterpret_cast<const real*>(D.C);
    const real* X = reinterpret_cast<const real*>(D.X);
    const long long r0 = (long long)blockIdx.x * D.rows_per_block, r1 = (r0 + D.rows_per_block < D.N) ? r0 + D.rows_per_block : D.N;
    const long long ncell = (r1 > r0 ? r1 - r0 : 0) * J;
    double ll = 0.0;
    const bool qw = M == CROSSQR;                         // per-cell quantile weights
    for (long long c = tid; c < ncell; c += 256) {
        const long long i = r0 + c / J;
        const int j = (int)(c % J);
        const size_t e = (size_t)i * J + j;
        const double th = D.sum[D.off_theta + i] * D.inv;
        const double eta = sa[j] * (th - sb[j]);
        ll += (D.Y[e] ? eta : 0.0) - log1pexp_r(eta);
        if (M != MLIRT) {
            const double ze = D.sum[D.off_zeta + i] * D.inv;
            const double lt = (double)C[e] + D.cm[j];
            double mu = sl[j] - ze, var = sg[j];
            if (fam_cq(M)) {
                const double nu = qw ? D.sum[D.off_nu + (long long)e] * D.inv : 1.0;
                mu += -th * sr[j] + D.k1 * nu;
                var *= D.k2 * nu;
            }
            const double er = lt - mu;
            ll += -0.5 * LOG_2PI - 0.5 * log(var) - 0.5 * er * er / var;
        }
    }
    const double det = sS[0] * sS[3] - sS[1] * sS[2];
    for (long long i = r0 + tid; i < r1; i += 256) {
        const double th = D.sum[D.off_theta + i] * D.inv;
        double xb0 = 0.0, xb1 = 0.0;
        if (M == MLIRT || M == RTIRT || fam_lq(M)) {
            xb0 = sbeta[0]; xb1 = sbeta[PMAX];
            for (int f = 0; f < F; ++f) { const double x = (double)X[(size_t)i * F + f]; xb0 += x * sbeta[1 + f]; xb1 += x * sbeta[PMAX + 1 + f]; }
        }
        if (M == MLIRT) { const double e0 = th - xb0; ll += -0.5 * LOG_2PI - 0.5 * e0 * e0; continue; }
        const double ze = D.sum[D.off_zeta + i] * D.inv;
        if (fam_lq(M)) {
            const double nu = (M == LATENTQR) ? D.sum[D.off_nu + i] * D.inv : 1.0;
            const double mu = xb0 + th * sbeta[p] + D.k1 * nu, var = sS[3] * D.k2 * nu, er = ze - mu;
            ll += -0.5 * LOG_2PI - 0.5 * log(var) - 0.5 * er * er / var;
        } else {
            const double e0 = th - (M == RTIRT ? xb0 : 0.0), e1 = ze - (M == RTIRT ? xb1 : 0.0);
            const double quad = (sS[3] * e0 * e0 - (sS[1] + sS[2]) * e0 * e1 + sS[0] * e1 * e1) / det;
            ll += -LOG_2PI - 0.5 * log(det) - 0.5 * quad;
        }
    }
    red[tid] = ll;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) { if (tid < w) red[tid] += red[tid + w]; __syncthreads(); }
    if (tid == 0) D.part[blockIdx.x] = red[0];
}

// checkConvergence's counts (src/SimTools.jl:427-437) from the device arrays of ess / rhat: c[0] columns with a defined ESS, c[1] of them with ESS > ess_min,
// c[2] columns with a defined R-hat, c[3] of them with R-hat < rhat_max (integer atomics: order-independent)
__global__ void __launch_bounds__(256) diag_count_kernel(const double* ess, const double* rhat, long long n, double ess_min, double rhat_max, unsigned long long* c)
{
    unsigned long long t[4] = {0ull, 0ull, 0ull, 0ull};
    for (long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x; k < n; k += (long long)gridDim.x * blockDim.x) {
        const double e = ess[k], r = rhat[k];
        if (e == e) { ++t[0]; if (e > ess_min) ++t[1]; }
        if (r == r) { ++t[2]; if (r < rhat_max) ++t[3]; }
    }
    for (int q = 0; q < 4; ++q) if (t[q]) atomicAdd(c + q, t[q]);
}

// n draws of the structural step's 2 x 2 inverse Wishart (erm_debug_invwishart): stream (seed, SIGP, i = k, sweep)
__global__ void __launch_bounds__(256) invwishart_batch_kernel(uint64_t seed, uint32_t sweep, long long n, double df, double p0, double p1, double p2, double p3, double* out)
{
    const long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    Stream ss(seed, 0u, SITE_SIGP, (uint32_t)k, 0u, sweep);
    double v3[3], S[4];
    const double Psi[4] = { p0, p1, p2, p3 };
    bartlett2_variates(ss, df, v3);
    invwishart2(Psi, v3, S);
    for (int e = 0; e < 4; ++e) out[4 * k + e] = S[e];
}

// ---------------------------------------------------------------------------------------------------------------------
// unit kernels for parity tests of the device samplers against the oracle
// ---------------------------------------------------------------------------------------------------------------------
template <typename real>
__global__ void sample_batch_kernel(int which, uint64_t seed, uint32_t site, uint32_t sweep, long long n,
                                    const double* par0, const double* par1, double* out, const double* pgtab)
{
    __shared__ double2 sh_logtab[128];
    fm::fill_log_table(sh_logtab, (int)threadIdx.x, (int)blockDim.x);
    __syncthreads();
    const long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    Stream st(seed, 0u, site, (uint32_t)k, 0u, sweep);
    double v = 0.0;
    switch (which) {
    case 15: v = fm::log(par0[k], sh_logtab); break;           // the table form of the cell path's logarithm
    case 16: v = fm::cos2pi(par0[k]); break;
    case 18: v = fm::exp_neg_ll(par0[k]); break;               // the cell log-likelihood's form of e^{-a}
    case 19: v = fm::log_word((uint32_t)par0[k], sh_logtab); break;      // log((w + 1/2) 2^-32) of the word par0 stands for (the PG attempt's -log u1)
    case 0: v = (double)uniform<real>(st); break;
    case 1: v = (double)normal<real>(st); break;
    case 2: v = (double)expo<real>(st); break;
    case 3: v = (double)pg1<real>(st, (real)par0[k], pgtab); break;
    case 4: v = (double)invgauss(st, (real)par0[k], (real)par1[k]); break;
    case 5: v = truncnorm0(st, par0[k], par1[k]); break;
    case 6: v = gamma_mt(st, par0[k]); break;
    case 7: v = pg_tail_weight(par0[k], pgtab); break;
    case 8: v = (double)qr_weight<real>(st, (real)par0[k], (real)par1[k]); break;
    case 9: v = (double)ndtri((real)par0[k]); break;
    case 17: v = qr_weight_q(st, par0[k], par1[k], par1[k] * par1[k], sh_logtab); break;      // the fp64 cell path's form of the quantile weight (parA = par0, parB = par1 at unit scale)
    case 11: v = fm::log(par0[k]); break;           // the cell path's fp64 elementary functions (erm_rng.hpp, namespace fm)
    case 12: v = fm::exp_neg(par0[k]); break;
    case 13: v = fm::sqrt(par0[k]); break;
    case 14: v = fm::div(par0[k], par1[k]); break;
    case 10: {     // PG(1, par0) through the reference form of the attempt (every statement in fp64)
        const double z = 0.5 * fabs(par0[k]);
        double o = 0.0;
        for (int tries = 0; tries < MAX_TRIES; ++tries) {
            const uint32_t w0 = st.next(), w1 = st.next(), w2 = st.next(), w3 = st.next();
            if (pg1_attempt_ref(z, w0, w1, w2, w3, pgtab, o)) break;
        }
        v = o;
    } break;
    }
    out[k] = v;
}

__global__ void gig_batch_kernel(uint64_t seed, uint32_t site, uint32_t sweep, long long n, double p, double a, double b, double* out)
{
    const long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    Stream st(seed, 0u, site, (uint32_t)k, 0u, sweep);
    out[k] = gig(st, p, a, b);
}

}  // namespace erm

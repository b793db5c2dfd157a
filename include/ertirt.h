/*
 * ertirt.h -- C ABI of libertirt.so, the MI355X (gfx950) Gibbs engine behind the `sample!` path of
 * ExtendedRtIrtModeling.jl.
 *
 * The reference has no FFI: `sample!` is an ordinary Julia method whose loop body calls the draw functions of
 * src/Draw.pl.jl.  This boundary is therefore created at the `sample!` method level; each entry point names the
 * reference interface it replaces (paths relative to /root/reference).  The Julia-side binding (ccall) is in
 * INTEGRATION.md and extendedrtirtmodeling.jl_amd/julia/.
 *
 * Conventions: every function returns 0 on success or a negative ERM_ERR_* code; the message is available from
 * erm_last_error() (thread-local).  All host arrays are owned by the caller, are read/written only during the call,
 * and use Julia's column-major layout.  The library owns all device memory behind the opaque handle.
 * A handle is not re-entrant; distinct handles are independent.
 */
#ifndef ERTIRT_H
#define ERTIRT_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef struct erm_engine* erm_handle;

enum {
    ERM_MODEL_MLIRT = 0,    /* GibbsMlIrt          src/GibbsRtIrt.pl.jl:76-106, sample! :210-257 */
    ERM_MODEL_RTIRT = 1,    /* GibbsRtIrt          src/GibbsRtIrt.pl.jl:114-146, sample! :278-346 */
    ERM_MODEL_CROSSQR = 2,  /* GibbsRtIrtCrossQr   src/GibbsRtIrtCross.pl.jl:115-147, sample! :265-325 */
    ERM_MODEL_LATENTQR = 3, /* GibbsRtIrtLatentQr  src/GibbsRtIrtLatent.pl.jl:105-137, sample! :271-337 */
    /* the non-quantile variants */
    ERM_MODEL_NULL = 4,     /* GibbsRtIrtNull      src/GibbsRtIrt.pl.jl:151-183, sample! :367-426 (no regression; Data.X ignored) */
    ERM_MODEL_CROSS = 5,    /* GibbsRtIrtCross     src/GibbsRtIrtCross.pl.jl:77-110, sample! :176-235 */
    ERM_MODEL_LATENT = 6    /* GibbsRtIrtLatent    src/GibbsRtIrtLatent.pl.jl:70-102, sample! :168-233 */
};
enum { ERM_OK = 0, ERM_ERR_ARG = -1, ERM_ERR_HIP = -2, ERM_ERR_STATE = -3, ERM_ERR_NONFINITE = -4, ERM_ERR_NOTRACE = -5, ERM_ERR_NOMEM = -6 };
enum { ERM_PREC_F32 = 0, ERM_PREC_F64 = 1 };
enum { ERM_TRACE_SUMMARY = 0, ERM_TRACE_FULL = 1 };
enum { ERM_TRACE_RA = 0, ERM_TRACE_RT = 1, ERM_TRACE_QR = 2, ERM_TRACE_LOGLIKE = 3 };

/* Mirrors SimConditions / setCond (src/Base.pl.jl:45-62) plus the sample! kwargs
 * (intercept, itemtype, cov2one: src/GibbsRtIrt.pl.jl:210,278; src/GibbsRtIrtCross.pl.jl:265; src/GibbsRtIrtLatent.pl.jl:271). */
typedef struct {
    int32_t model;          /* ERM_MODEL_* */
    int32_t n_item;         /* Cond.nItem; 1 .. 896 (the fused sweep kernel keeps per-wave item accumulators in LDS; the single-pass models keep the fused sweep up to 512 items in fp64
                             * and 640 in fp32 (GibbsMlIrt, with four statistics per item, a little further); beyond that, and always for the Cross family, the engine takes the two-kernel schedule) */
    int64_t n_subj;         /* Cond.nSubj */
    int32_t n_feat;         /* Cond.nFeat (columns of Data.X; ignored by the Cross family and Null); 0 .. 14 (the structural draws hold the <= 16-column design [1 X theta] in LDS) */
    int32_t n_iter;         /* Cond.nIter */
    int32_t n_chain;        /* Cond.nChain: sweep (m,l) of the reference's interleaved loop is trace row m*nChain+l */
    int32_t n_burnin;       /* Cond.nBurnin (setCond forces round(nIter/2); the host shim does the same) */
    int32_t intercept;      /* sample!(...; intercept=false) */
    int32_t one_pl;         /* itemtype == "1pl" */
    int32_t cov2one;        /* sample!(...; cov2one) */
    int32_t sigp_mode;      /* LatentQr Sigma_p scale: 0 = reference expression src/Draw.pl.jl:594 (the N x N `/` in closed form), 1 = the evidently intended sum r_i^2/(2 k2 nu_i) */
    int32_t chain_id;       /* selects an independent random stream (one chain per GPU farms use the rank); 0 .. 255 (eight bits of the Philox counter) */
    double  q_rt;           /* Cond.qRt */
    uint64_t seed;
    int32_t device;         /* HIP device ordinal */
    int32_t precision;      /* ERM_PREC_F32: fp32 cell arithmetic + fp64 accumulation; ERM_PREC_F64: all fp64 */
    int32_t trace_mode;     /* ERM_TRACE_FULL keeps theta/zeta(/nu) per sweep (Post.ra/rt/qr); SUMMARY keeps item-level traces + running means */
    int32_t lanes_per_row;  /* 0 = auto; power of two in [1,64]: lanes that share one subject */
    int32_t block_threads;  /* 0 = auto */
    int32_t grid_blocks;    /* 0 = auto */
    int32_t profile;        /* 1 = bracket sweep-kernel launches with HIP events for erm_get_timing: two single sweeps before every replayed 32-sweep block of a
                             * long run; every sweep (in replayed 16- / 4-sweep graphs) of a run shorter than 68 sweeps */
    int32_t flags;          /* ERM_FLAG_* (diagnostics; a schedule flag keeps the launch geometry, so none changes a result); bits outside ERM_FLAG_ALL are refused */
    double  nu_trace_max_gb; /* GibbsRtIrtCrossQr, ERM_TRACE_FULL: budget in GiB for the per-sweep vec(nu) block of Post.qr (0 = the default, 16; negative or NaN is refused) */
} erm_config;
enum {
    ERM_FLAG_NO_FUSE = 1,          /* two kernels per sweep (stand-alone tiny step + row pass) instead of the fused sweep kernel */
    ERM_FLAG_NO_GRAPH = 2,         /* enqueue every sweep instead of replaying the captured 32-sweep hipGraph */
    ERM_FLAG_FARM_FORCE_RCCL = 4,  /* erm_farm_get_mean reduces over RCCL even when all chains share one device (one-rank communicator; tests) */
    ERM_FLAG_NO_PERSIST = 8,       /* small data sets: one launch per sweep instead of ONE persistent launch per erm_run (the statistics cross between its sweeps as tagged packets) */
    ERM_FLAG_TEST_PERSIST_TIMEOUT = 16, /* tests: the SECOND persistent erm_run of the engine loses one workgroup's statistics packet and waits 2 ms instead of 1 s, so that
                                        * the time-out -> restore -> per-sweep replay path of erm_run is exercised (the chain is still the per-sweep chain bit for bit) */
    ERM_FLAG_ALL = 31
};

/* Mirrors InputPara (src/Base.pl.jl:100-115).  NULL members are skipped.  Shapes:
 * theta,zeta [nSubj]; a,b,lambda,sig2t,rho [nItem]; sigp [4] = vec(Sigma_p);
 * beta: MlIrt [nFeat+1], RtIrt / Null [(nFeat+1)*2] = vec(beta) (Null: always zero), LatentQr / Latent [nFeat+2];
 * nu: LatentQr [nSubj], CrossQr [nSubj*nItem] column-major. */
typedef struct {
    double *theta, *a, *b, *zeta, *lambda, *sig2t, *beta, *sigp, *rho, *nu;
} erm_state;

typedef struct {
    double run_ms;          /* device time of the last erm_run (HIP events on the engine's stream) */
    double pass_ms_total;   /* sum of row-pass kernel durations in the last erm_run (profile=1; event-pair overhead subtracted), else 0 */
    double event_overhead_ms; /* mean duration of an empty HIP event pair on the engine's stream, measured in the same run */
    int64_t pass_launches;  /* number of row-pass launches timed */
    int64_t sweeps;         /* sweeps in the last erm_run */
    int32_t lanes_per_row, block_threads, grid_blocks, lds_bytes;
    int32_t cu_count;
    int32_t persistent;     /* 1 = this engine runs erm_run as ONE persistent launch (small data sets; ERM_FLAG_NO_PERSIST turns it off) */
    int32_t persist_fallbacks; /* persistent launches that timed out waiting for a workgroup that never became resident (another process holds compute units): the
                             * erm_run restored the state it had saved, replayed the call on the per-sweep schedule and the engine stays there (persistent = 0) */
    int32_t reserved_;
} erm_timing;

/* Replaces the Gibbs* constructors' allocation of Post and Para (src/GibbsRtIrt.pl.jl:94-104,134-144). */
int erm_create(const erm_config* cfg, erm_handle* out);
void erm_destroy(erm_handle h);

/* Replaces InputData (src/Base.pl.jl:67-78): Y 0/1 bytes [nSubj x nItem], logT = log.(T), X [nSubj x nFeat]; column-major.
 * logT may be NULL for MlIrt; X may be NULL when n_feat == 0 or for CrossQr. */
int erm_set_data(erm_handle h, const uint8_t* Y, const double* logT, const double* X);

/* Simulation studies.  Replaces setDataRtIrt / setDataRtIrtNull / setDataMlIrt / setDataRtIrtCross / setDataRtIrtLatent
 * (src/SimTools.jl:117-368): draws covariates, subject parameters and responses ON the device from the true item / structural
 * parameters in `truth` (a, b, lambda, sig2t, rho, sigp as in erm_state; beta WITHOUT intercept row: RtIrt [nFeat][2] column-major, MlIrt
 * [nFeat], Latent(Qr) [nFeat+1]; theta / zeta / nu ignored) and installs them as the resident data set, exactly as erm_set_data would.
 * noise: 0 "norm", 1 "tail" (t5), 2 "skew" (Gamma(1/2,1) - 1) for the Cross / Latent generators.  erm_get_truth returns the generated
 * theta, zeta; erm_get_data the resident data set (either source) in the caller's column-major layout (any pointer may be NULL). */
int erm_simulate_data(erm_handle h, const erm_state* truth, uint64_t seed, int noise);
int erm_get_truth(erm_handle h, double* theta, double* zeta);
int erm_get_data(erm_handle h, uint8_t* Y, double* logT, double* X);

/* Para in / out (setInitialValues: src/GibbsRtIrt.pl.jl:84-93,122-133; Cross :123-134; Latent :113-124).
 * After erm_run, erm_get_state returns the last recorded trace row bit for bit -- except nu (the quantile models): every schedule draws
 * nu_{t+1} at the end of sweep t (it depends on sweep t's draws only), so the state holds the nu that the NEXT sweep reads and records,
 * not the nu of the last trace row.  Post.mean and the traces hold nu_t; the next erm_run of the engine records state-nu as its first nu row. */
int erm_set_state(erm_handle h, const erm_state* st);
int erm_get_state(erm_handle h, erm_state* st);

/* The body of `for m in 1:nIter, l in 1:nChain` (src/GibbsRtIrt.pl.jl:221-246, 289-324; Cross :276-302; Latent :282-314):
 * runs `nsweeps` sweeps continuing from the current state; sweeps fill trace rows in order. */
int erm_run(erm_handle h, int64_t nsweeps);
/* A new seed for the chain's random streams (a simulation study re-uses ONE engine for all replications of a condition: src/SimTools.jl:457-495 constructs a
 * fresh sampler per replication, which draws from Julia's global stream).  Takes effect with the next erm_run, which then draws the chain a freshly created
 * engine with this seed would draw from the same data and state (the sweep counter that addresses the streams starts over). */
int erm_set_seed(erm_handle h, uint64_t seed);
int64_t erm_rows_done(erm_handle h);
int erm_reset_trace(erm_handle h);   /* forget recorded rows and running means (state is kept) */

/* Post.ra / Post.rt / Post.qr / Post.logLike (src/GibbsRtIrt.pl.jl:35-71; Cross :55-69; Latent :50-64) in Julia layout
 * [nIter][width][nChain], nIter fastest.  Needs ERM_TRACE_FULL for RA/RT/QR.  GibbsRtIrtCrossQr's qr carries vec(nu) (nSubj*nItem values per
 * sweep); it is recorded when nIter*nChain*nSubj*nItem values fit erm_config.nu_trace_max_gb (default 16 GiB), else ERM_ERR_NOTRACE. */
int64_t erm_trace_width(erm_handle h, int which);
int erm_get_trace(erm_handle h, int which, double* out);
/* item-level trace, always kept: out[row][4*nItem + nq] = a, b, lambda, sig2t, small part of qr (row-major) */
int64_t erm_item_trace_width(erm_handle h);
int erm_get_item_trace(erm_handle h, double* out);

/* Post.mean (src/GibbsRtIrt.pl.jl:249-254, 327-343): mean over rows >= nBurnin*nChain of everything in erm_state. */
int erm_get_mean(erm_handle h, erm_state* out);
int64_t erm_post_count(erm_handle h);   /* number of rows that entered the means */

/* checkConvergence's inputs (src/SimTools.jl:419-443, MCMCChains' ess_rhat on Post.ra / rt / qr after burn-in), computed on the device
 * from the resident traces: ess[k], rhat[k] for every column k of trace `which` (width erm_trace_width); split-R-hat and the effective
 * sample size by Geyer's initial monotone sequence over the 2*nChain split chains (the non-rank-normalised estimator); NaN for a column
 * that never moves: one whose used draws (the first and last floor((nIter - nBurnin) / 2) post-burn-in draws of every chain) are all equal -- decided on the draws,
 * not on a variance computed from a rounded mean.  The sum of pair sums P_k = rho_2k + rho_2k+1 stops before the first one that is not positive: a column whose
 * first pair sum is not positive gets -M n (M = 2*nChain sequences of n draws), a defined and negative ESS (and any column whose pair sums add up to less than
 * 1/2 gets a negative one: seen on sampler traces with n = 4 .. 8, not with n >= 32).  Needs ERM_TRACE_FULL and a completed run with at least
 * 8 post-burn-in iterations and at most 16 chains (ERM_ERR_ARG otherwise). */
int erm_get_diagnostics(erm_handle h, int which, double* ess, double* rhat);
/* checkConvergence's summary itself (src/SimTools.jl:427-437) without the N-wide vectors: counts4 = { columns with a defined ESS, of those ESS > 400, columns with a
 * defined R-hat, of those R-hat < 1.1 } for trace `which`, counted on the device. */
int erm_get_convergence(erm_handle h, int which, int64_t* counts4);
/* The rank-normalised diagnostics of Vehtari, Gelman, Simpson, Carpenter and Buerkner (2021) -- what `ess_rhat` of MCMCChains 6 / MCMCDiagnosticTools 0.3 (the
 * versions the reference's Project.toml names) reports: bulk-ESS, tail-ESS and rank-normalised split-R-hat of every column of trace `which`, computed on the
 * device from the resident traces (the N-wide traces never cross to the host).  On the heavy-tailed columns of this model family (sig2t, Sigma_p, the quantile
 * models' nu) the moment-based estimator above is blind to chains that differ in scale and its ESS is dominated by a few extreme draws; this one is not.
 * Definition.  The used draws of a column are those of erm_get_diagnostics: with Tn = n_iter - n_burnin and n = floor(Tn / 2) the first n and the last n
 * post-burn-in draws of every chain (an odd Tn drops the middle draw): M = 2 n_chain sequences, S = M n pooled draws, S even.  E(.) and R(.) are the ESS and the
 * split-R-hat defined above, applied to a transformed column (same stop rule, same -M n case, same "never moves -> NaN" rule decided on the series).
 *   1. ranks          r_i = the average rank of x_i among the S pooled draws; ties share the mean of their positions (-0.0 and +0.0 tie)
 *   2. normal scores  z_i = Phi^-1((r_i - 3/8) / (S + 1/4)): one fp64 subtraction, one addition, one division, then the device's fp64 normal quantile
 *                     (Wichura's AS 241), whatever the engine's precision
 *   3. bulk ESS       ess_bulk = E(z)
 *   4. folding        med = (x_(S/2) + x_(S/2+1)) / 2 with order statistics of the pooled draws, f_i = |x_i - med|, z' = the normal scores of f
 *   5. rank R-hat     rhat_rank = max(R(z), R(z')) over those of the two that are defined (a two-valued column split evenly makes f constant: R(z') is
 *                     undefined and rhat_rank = R(z))
 *   6. tail ESS       k = ceil(S / 20) = (S + 19) / 20 in integers, L_i = [x_i <= x_(k)], U_i = [x_i >= x_(S+1-k)], ess_tail = min(E(L), E(U)); NaN if either
 *                     indicator column is constant.  Order statistics, not interpolated quantiles: every decision up to the normal quantile is an ordering
 *                     or an integer.  (Stan and ArviZ interpolate the 5 % and 95 % quantiles; the difference is below the estimator's own noise.)
 *   7. a column that never moves: all three NaN.
 * An fp32 engine's traces are float: the stored values are ranked, widened to double.  Any of the three output pointers may be NULL; width erm_trace_width.
 * One workgroup sorts and ranks a column in LDS, so S is capped at 8192 used draws per column (ERM_ERR_ARG above it, the message names the cap); otherwise the
 * limits of erm_get_diagnostics: ERM_TRACE_FULL (ERM_ERR_NOTRACE), a completed run (ERM_ERR_STATE), >= 8 post-burn-in iterations and <= 16 chains
 * (ERM_ERR_ARG).  Device scratch is bounded (columns go through in chunks, 256 MB of staged draws at most; ERM_ERR_NOMEM if it cannot be had).  The call only
 * reads the engine: the chain and every other read-out are unchanged by it.  All sums have a fixed order: the results are bit-reproducible from call to call
 * and a column's result does not depend on the other columns. */
int erm_get_rank_diagnostics(erm_handle h, int which, double* ess_bulk, double* ess_tail, double* rhat_rank);
/* counts6 = { bulk-ESS defined, bulk-ESS > 400, tail-ESS defined, tail-ESS > 400, rank R-hat defined, rank R-hat < 1.1 } of trace `which`: the reference's
 * thresholds, counted on the device as for erm_get_convergence. */
int erm_get_rank_convergence(erm_handle h, int which, int64_t* counts6);

/* getDic (src/GibbsRtIrt.pl.jl:432-472, src/GibbsRtIrtCross.pl.jl:330-353, src/GibbsRtIrtLatent.pl.jl:342-365) from device-resident state:
 * out = { Dbar, Dhat, pD, DIC } with Dbar = -2 mean(Post.logLike) over ALL recorded rows (burn-in included, as the reference does), Dhat = -2 logLik(Post.mean) from
 * ONE evaluation pass over the resident data set at the running means (theta, zeta, nu sums and the post-burn-in item-level trace rows; nothing N-wide crosses
 * the boundary), pD = Dbar - Dhat, DIC = Dbar + pD.  Needs a run with post-burn-in rows. */
int erm_get_dic(erm_handle h, double* out4);

/* WAIC (Watanabe 2010; Vehtari, Gelman and Gabry 2017), accumulated on the device sweep by sweep.  The reference offers DIC only.  A unit u is a subject or a
 * cell (i, j); l_u^(s) is the unit's part of the model's own getLogLikelihood* at the values of trace row s: per cell y eta - log(1 + e^eta), eta = a_j (theta_i - b_j),
 * plus -- for every model but GibbsMlIrt -- the normal log-density of logT_ij (mean lambda_j - zeta_i [- theta_i rho_j + k1 nu_ij], variance sig2t_j [k2 nu_ij]; brackets:
 * Cross family); a subject's is the sum of its cells.  The structural term (theta, zeta given beta, Sigma_p) is NOT part of it: this is the conditional WAIC,
 * leave-one-unit-out given the subject's own parameters.  S = the post-burn-in rows, exactly those behind Post.mean (|S| = erm_post_count):
 *   lppd_u = log mean_S exp l_u,  p_u = Var_S(l_u) (|S| - 1 in the denominator),  elpd_u = lppd_u - p_u,
 *   elpd = sum_u elpd_u,  p_waic = sum_u p_u,  waic = -2 elpd,  se_waic = 2 sqrt(U Var_u(elpd_u)).
 * erm_set_pointwise enables it (four doubles of device memory per unit; GibbsRtIrtCrossQr also keeps a copy of nu_t, nSubj * nItem values, taken ahead of the pass
 * that overwrites it) and is allowed only while no trace row is recorded (after erm_create or erm_reset_trace; ERM_ERR_STATE otherwise).  Unknown unit: ERM_ERR_ARG;
 * a subject-sharded engine: ERM_ERR_STATE; no memory for the accumulators: ERM_ERR_NOMEM, the engine stays as it was.  From then on every sweep is followed by one
 * streaming pass over the resident data set (on the stream and inside the captured graphs; burn-in rows return at once), and small data sets are run one launch per
 * sweep at the persistent schedule's geometry, as under ERM_FLAG_NO_PERSIST (erm_timing.persistent = 0): the chain itself is bit for bit the chain without WAIC.
 * In profile mode the event bracket of a timed sweep also holds the pointwise pass.  erm_reset_trace clears the accumulators.  The chain farm keeps no such accumulators:
 * its WAIC is the marginal one below, erm_farm_get_marginal_waic.
 * erm_get_waic: out = { elpd, p_waic, waic, se_waic, lppd, n_units, n_rows, number of units with p_u > 0.4 }, finished and summed on the device (needs two
 * post-burn-in rows).  erm_get_pointwise: lppd_u / p_u of every unit (either may be NULL): subjects in order, cells column-major [nSubj][nItem]. */
enum { ERM_POINTWISE_OFF = 0, ERM_POINTWISE_SUBJECT = 1, ERM_POINTWISE_CELL = 2 };
int erm_set_pointwise(erm_handle h, int unit);
int erm_get_waic(erm_handle h, double* out_eight);
int64_t erm_pointwise_units(erm_handle h);
int erm_get_pointwise(erm_handle h, double* lppd_u, double* p_u);

/* Marginal WAIC: the unit is a subject with its own theta_i and zeta_i INTEGRATED OUT.  The conditional WAIC above answers "how well would new responses of the same
 * persons be predicted"; its effective number of parameters grows with nSubj, and it holds fixed exactly the part in which GibbsRtIrt, Null, Cross and Latent differ (how
 * theta and zeta hang together).  For choosing between latent-variable models the marginal criterion is the one to use (Merkle, Furr and Rabe-Hesketh 2019).  Once
 * theta_i and zeta_i are gone, a subject's log-likelihood at trace row s depends on that row's item-level and structural parameters only -- the columns of the item-level
 * trace, which is always kept, in fp64, in both trace modes -- so everything is computed AFTER the run from resident state: no pass behind the sweep, no erm_set_pointwise,
 * no change to any schedule, and the calls only read the engine (the chain, the traces and the accumulators of erm_get_waic are unchanged by them).
 * Served: GibbsMlIrt, GibbsRtIrt, GibbsRtIrtNull, GibbsRtIrtCross, GibbsRtIrtLatent.  The two quantile models are refused with ERM_ERR_ARG: with nu integrated out the
 * response-time term is no longer Gaussian in zeta.  GibbsRtIrtLatentQr has entries of its own, erm_get_quantile_marginal_waic below; for GibbsRtIrtCrossQr the
 * zeta integral has no closed form.
 * Definition, for subject i at row s; items j = 1..J, y_j in {0,1}, t_j = logT_ij, x = the subject's covariates, S = Sigma_p with S12 read as (Sigma_p[1] + Sigma_p[2]) / 2.
 *   Population law -- the structural term of the model's own getLogLikelihood*:  theta ~ N(mu, S11'),  zeta | theta ~ N(m0 + m1 theta, v)
 *     MlIrt         mu = beta0 + x beta, S11' = 1; no zeta, no response times
 *     RtIrt         mu = [1 x] beta[:,1], S11' = S11;  m1 = S12 / S11, m0 = [1 x] beta[:,2] - m1 mu, v = S22 - S12^2 / S11
 *     Null, Cross   mu = 0, S11' = S11;  m1 = S12 / S11, m0 = 0, v = S22 - S12^2 / S11
 *     Latent        mu = 0, S11' = S11;  m0 = beta0 + x beta_x, m1 = beta_theta, v = S22.  The theta law is the prior Latent's theta draw uses (drawSubjAbilityNull,
 *                   src/Draw.pl.jl:67-80: mean 0, variance Sigma_p[1,1]); the reference's getLogLikelihoodRtIrtLatent carries no density for theta.
 *   Response part   B(theta) = sum_j [ y_j eta_j - log(1 + e^eta_j) ],  eta_j = a_j (theta - b_j)
 *   Response times, zeta integrated out analytically.  g_j = 1 / sig2t_j, d_j(theta) = lambda_j - t_j - rho_j theta (rho = 0 outside Cross),
 *     P = sum g_j,  R(theta) = sum g_j d_j = R0 - theta R1,  D(theta) = sum g_j d_j^2 = D0 - 2 theta D1 + theta^2 D2,  m = m0 + m1 theta,
 *     T(theta) = -(J/2) log 2 pi - 1/2 sum_j log sig2t_j - 1/2 log(1 + v P) - 1/2 [ D + (P m^2 - 2 R m - v R^2) / (1 + v P) ]      (MlIrt: T = 0)
 *     = log N(t; lambda - rho theta - m, diag(sig2t) + v 1 1').  No 1 / v: a Sigma_p of correlation +-1 after cov2one (v = 0) is an ordinary case.
 *   theta integral: a fixed rule of Q nodes, Q odd:  z_q = -6 + q h, h = 12 / (Q - 1), theta_q = mu + sqrt(S11') z_q,
 *     e_q = log h - 1/2 log 2 pi - 1/2 z_q^2 + B(theta_q) + T(theta_q),   l_i^(s) = log sum_q exp(e_q) = M + log S with M = max_q e_q, S = sum_q exp(e_q - M).
 *     The rule fails when the posterior of theta is narrower than the spacing (many items).  A subject is COARSE if S < 2 at some row: the largest node carries more
 *     than half the mass (for a Gaussian posterior: sd < 0.8 h, where the rule's relative error passes about 3e-6).  Raise Q until no unit is coarse.
 *   WAIC: S = the post-burn-in rows, those behind Post.mean (rows >= n_burnin * n_chain; |S| = erm_post_count), applied in trace order to the accumulators of
 *     erm_get_waic; lppd_i, p_i, elpd, p_waic, waic and se_waic are formed exactly as erm_get_waic forms them.  All fp64, whatever the engine's precision (an fp32
 *     engine's resident logT and X are widened).
 * A subject's result depends on its own data, the rows and Q only -- not on nSubj, the other subjects, the launch or the device: eight lanes share a subject whatever the
 * sizes, every sum has a fixed order, and nothing is atomic.  The results are bit-reproducible from call to call and do not depend on how the sweeps were split into
 * erm_run calls.
 * erm_get_marginal_waic: out10 = the eight values of erm_get_waic (n_units = n_subj), then Q, then the number of coarse units.  lppd_u, p_u [n_subj] may be NULL.
 *   n_nodes = 0 means 61; otherwise odd and in 3 .. 1025 (ERM_ERR_ARG).  Works in both trace modes; reads the item trace in place from row n_burnin * n_chain.
 *   Refused: a quantile model (ERM_ERR_ARG), a subject-sharded engine (ERM_ERR_STATE), fewer than two post-burn-in rows, no data set or an engine whose last erm_run
 *   failed part-way (ERM_ERR_STATE), no scratch memory (ERM_ERR_NOMEM; four doubles and a flag per subject).
 * erm_farm_get_marginal_waic: the same over the rows of the whole farm -- the post-burn-in rows of chain 0, then chain 1, ..., as one table on chain 0's device, whose
 *   resident data set supplies the data (n_rows = erm_farm_post_count).  The chains' item-trace rows cross through the host (item-level: a few hundred kilobytes); no
 *   device setting is touched.  Every chain must have recorded the same number of rows, at least two of them post-burn-in (ERM_ERR_STATE, the message names the chain).
 *   A farm of one chain returns its engine's result bit for bit.
 * erm_marginal_loglik: the same kernel on caller-supplied data (Y, logT, X column-major as erm_set_data takes them; X is ignored by the models that see no covariates)
 *   and caller-supplied rows [n_rows][erm_item_trace_width], exactly as erm_get_item_trace returns them.  l [n_subj][n_rows], column-major (the subject fastest),
 *   receives every l_i^(s); out10, lppd_u, p_u as above over all n_rows rows.  Any output may be NULL; n_rows >= 1 for l, >= 2 for the WAIC outputs (ERM_ERR_ARG).
 *   A NaN anywhere: ERM_ERR_NONFINITE.  A row with sig2t <= 0, Sigma_p[1,1] <= 0 or v < 0: ERM_ERR_ARG, the message names the row.  Serves item traces that are no
 *   longer resident and the scoring of new respondents against a saved posterior. */
int erm_get_marginal_waic(erm_handle h, int32_t n_nodes, double* out10, double* lppd_u, double* p_u);
int erm_marginal_loglik(int device, int model, int64_t n_subj, int32_t n_item, int32_t n_feat, const uint8_t* Y, const double* logT, const double* X, const double* rows,
                        int64_t n_rows, int32_t n_nodes, double* l, double* out10, double* lppd_u, double* p_u);

/* Marginal WAIC and PSIS-LOO of GibbsRtIrtLatentQr (= GibbsRtIrtQuantile): the unit is a subject with theta_i, zeta_i AND the quantile weight nu_i integrated out,
 * so a Latent fit and a LatentQr fit of the same data -- or two levels q_rt -- are compared in the same unit, "subject-marginal".  Entries of their own, because
 * every entry above refuses the quantile models; computed after the run from resident state, exactly as erm_get_marginal_waic is.
 * Served: LatentQr only.  A model without quantile weights: ERM_ERR_ARG, the message names erm_get_marginal_waic.  CrossQr: ERM_ERR_ARG -- with nu_ij integrated out
 * every cell's response time is asymmetric Laplace in zeta, so -log p(t | theta, zeta) is piecewise linear in zeta with J kinks that move with theta; a fixed zeta rule
 * is second order at best there, and the exact route sorts J break points per (subject, row, node).
 * Definition, for subject i at row s (a LatentQr row has Latent's layout: a b lambda sig2t | beta0 beta_x[F] beta_theta | vec(Sigma_p)); q = q_rt,
 * k1 = (1 - 2q) / (q (1 - q)), k2 = 2 / (q (1 - q)), s = Sigma_p[2,2], m = m0 + m1 theta with m0 = beta0 + x beta_x, m1 = beta_theta.
 *   nu.     The model's own getLogLikelihoodRtIrtLatentQr has zeta_i | theta_i, nu_i ~ N(m + k1 nu_i, s k2 nu_i).  The conditional drawQrWeightsLatentQr draws from
 *           (src/Draw.pl.jl:325-343: 1 / nu ~ InverseGaussian(B / A, B^2), B^2 = (2 k2 + k1^2) / (s k2)) is the one this likelihood gives under
 *           nu_i ~ Exponential(mean s): that is the prior the sampler implies, and the one integrated over here.  It leaves zeta | theta asymmetric Laplace:
 *             log p(zeta | theta) = log(q (1 - q) / s) - u (q - [u < 0]),  u = (zeta - m) / s.
 *   theta.  theta ~ N(0, Sigma_p[1,1]), the law drawSubjAbilityNull uses, exactly as for Latent; the node rule (Q odd, z_q = -6 + q h, theta_q = sd z_q,
 *           e_q = log h - 1/2 log 2 pi - 1/2 z_q^2 + B(theta_q) + T(theta_q), l = M + log S, COARSE if S < 2 at some row) and B(theta) are erm_get_marginal_waic's, unchanged.
 *   zeta.   The response times are Gaussian in zeta, so zeta is integrated out in closed form.  g_j = 1 / sig2t_j, d0_j = lambda_j - t_j,
 *           P = sum g_j, R0 = sum g_j d0_j, D0 = sum g_j d0_j^2, L = sum log sig2t_j;  bU = R0 - q / s,  bL = R0 + (1 - q) / s,
 *             up = bU^2 / (2 P) + q m / s       + logPhi(-(m - bU / P) sqrt(P))          (the part zeta >= m)
 *             lo = bL^2 / (2 P) - (1 - q) m / s + logPhi( (m - bL / P) sqrt(P))          (the part zeta <  m)
 *             T(theta) = -(J/2) log 2 pi - L / 2 - D0 / 2 + log(q (1 - q) / s) + 1/2 log(2 pi / P) + logaddexp(up, lo).
 *           logPhi, the log of the normal distribution function, in three arms, the same on host and device:  x >= 0: log1p(-erfc(x / sqrt 2) / 2);
 *           -36 <= x < 0: log(erfc(-x / sqrt 2) / 2);  x < -36: -x^2 / 2 - log(-x) - 1/2 log 2 pi + log1p(-r + 3 r^2 - 15 r^3 + ... + 2027025 r^8), r = 1 / x^2
 *           (eight terms of the asymptotic series by Horner's rule; the ninth is below 4e-21).  logaddexp(a, b) = max(a, b) + log1p(exp(-|a - b|)).
 *           T needs s > 0, P > 0 and 0 < q < 1.  bU^2 / (2 P) cancels against logPhi when s is tiny: at J = 1, s = 0.001 the float64 value is good to about 1e-11.
 *   All else -- the WAIC over the post-burn-in rows, PSIS-LOO on l, fp64 whatever the engine's precision, independence of the launch -- as defined above.
 * erm_get_quantile_marginal_waic / erm_farm_get_quantile_marginal_waic: the outputs, n_nodes, the row limits and the refusals (a shard, a failed run, no data set, too
 *   few rows) of erm_get_marginal_waic / erm_farm_get_marginal_waic, at the engine's (the farm's) q_rt.
 * erm_get_quantile_marginal_loo / erm_farm_get_quantile_marginal_loo: those of erm_get_marginal_loo / erm_farm_get_marginal_loo below (25 .. 8192 rows, chunked scratch).
 * erm_quantile_marginal_loglik: erm_marginal_loglik with the caller's q_rt; validated as a Latent table is, and also: q_rt outside (0, 1): ERM_ERR_ARG; a row with
 *   Sigma_p[2,2] <= 0: ERM_ERR_ARG, "row r: Sigma_p[2,2] must be positive". */
int erm_get_quantile_marginal_waic(erm_handle h, int32_t n_nodes, double* out10, double* lppd_u, double* p_u);
int erm_get_quantile_marginal_loo(erm_handle h, int32_t n_nodes, double* out12, double* pw);
int erm_quantile_marginal_loglik(int device, int model, int64_t n_subj, int32_t n_item, int32_t n_feat, const uint8_t* Y, const double* logT, const double* X,
                                 const double* rows, int64_t n_rows, double q_rt, int32_t n_nodes, double* l, double* out10, double* lppd_u, double* p_u);

/* Scores of respondents: the posterior mean and standard deviation of every subject's theta_i and zeta_i, their covariance, and what the rows were worth -- the
 * standard errors and reliabilities an IRT model is fitted for -- from the item-level trace alone.  Given a row of the item-level trace, a subject's (theta, zeta)
 * depends on nothing but its own data, so no trace of theta is needed: the row-wise posterior moments, averaged over the rows, are the Rao-Blackwell estimators of
 * E[theta_i | data] and Var[theta_i | data] with the item and structural uncertainty integrated.  Computed AFTER the run from resident state, in ERM_TRACE_SUMMARY as in
 * ERM_TRACE_FULL; the calls only read the engine.  Served: the five models of erm_get_marginal_waic; the two quantile models are refused with ERM_ERR_ARG for its reason.
 * Definition, for subject i at row s.  The population law (mu, sd = sqrt(S11'), m0, m1, v), the node rule (z_q, theta_q, e_q, M, S) and the item sums (P, R0, R1, ...)
 * are exactly those of erm_get_marginal_waic above; l_s = M + log S.
 *   theta at the row   w_q = exp(e_q - M) / S,  Z1 = sum w_q z_q,  Z2 = sum w_q z_q^2;   E_s = mu + sd Z1,  V_s = sd^2 (Z2 - Z1^2), clamped at 0.
 *                      The three sums S, sum exp(e_q - M) z_q, sum exp(e_q - M) z_q^2 stream and merge under the same running maximum as M and S do there.
 *   zeta at the row    given theta and the response times, zeta ~ N(c0 + c1 theta, u):  u = v / (1 + v P),  c0 = (m0 + v R0) / (1 + v P),  c1 = (m1 - v R1) / (1 + v P).
 *                      No 1 / v: v = 0 is an ordinary case.  Hence Ez_s = c0 + c1 E_s,  Vz_s = u + c1^2 V_s,  C_s = c1 V_s.  MlIrt has no zeta: its zeta columns and
 *                      its covariance are NaN.
 *   across the rows    in trace order, with weight omega_s:
 *                        ERM_SCORE_EQUAL       omega_s = 1: right for the subjects of the data set the chain was fitted to, and the usual operational scoring, in
 *                                              which a new respondent does not update the item posterior;
 *                        ERM_SCORE_LIKELIHOOD  omega_s = exp(l_s - Lambda), Lambda the running maximum of l_s (what is held is rescaled when Lambda rises): the
 *                                              posterior of a new respondent given their own data and the saved item posterior.
 *                      West's weighted Welford on the pair (E_s, Ez_s) with its co-moment, the weighted means of V_s, Vz_s and C_s, sum omega and sum omega^2: eleven
 *                      doubles per subject, held in registers from the first row to the last.
 *   results            the law of total variance, W = sum omega:  theta = mean E,  theta_sd^2 = mean V + M2_E / W,  cov = mean C + C_EEz / W,  zeta and zeta_sd
 *                      likewise,  row_ess = W^2 / sum omega^2 (= n_rows under equal weights).
 * Population law, not the sampler's conditionals.  The scores are posterior under the law erm_get_marginal_waic defines: theta borrows strength from the response
 * times through S12 (RtIrt, Null, Cross) or beta_theta (Latent) and rho (Cross).  The reference's sampler is not the Gibbs sampler of that joint model for the
 * response-time models -- drawSubjAbility (src/Draw.pl.jl:49-62) and drawSubjSpeed (:132-141) each use the marginal prior and ignore Sigma_p[1,2]; Latent's theta draw
 * ignores zeta's regression on theta -- so for those models the scores differ from Post.mean BY DESIGN.  Only for GibbsMlIrt is the sampler's theta conditional the
 * model's own, and there the two agree (tests/test_score_host.py, tests/test_gpu_scores.py).
 * Output: score, column-major [n_subj][7], column ERM_SCORE_*; COARSE is 1.0 if S < 2 at some row (the marginal WAIC's rule) and 0.0 otherwise.
 *   out4 (may be NULL) = { n_subj, n_rows, Q, number of coarse subjects }.  Everything is fp64 whatever the engine's precision; every sum has a fixed order and nothing
 *   is atomic; a subject's result depends on its own data, the rows, Q and the weighting only; results are bit-reproducible from call to call and do not depend on
 *   how the sweeps were split into erm_run calls.
 * erm_get_scores: the post-burn-in rows of the resident item trace, read in place, equal weights.  n_nodes and the refusals as erm_get_marginal_waic's, except that
 *   ONE post-burn-in row is enough.  erm_farm_get_scores (below): the same over the chain-major table of erm_farm_get_marginal_waic on chain 0's device; a farm of one
 *   chain returns its engine's result bit for bit.
 * erm_score: the same kernel on caller-supplied data and rows, validated as erm_marginal_loglik validates them (a NaN: ERM_ERR_NONFINITE; a bad row: ERM_ERR_ARG,
 *   the message names the row); n_rows >= 1; an unknown weighting: ERM_ERR_ARG. */
enum { ERM_SCORE_EQUAL = 0, ERM_SCORE_LIKELIHOOD = 1 };
enum { ERM_SCORE_THETA = 0, ERM_SCORE_THETA_SD = 1, ERM_SCORE_ZETA = 2, ERM_SCORE_ZETA_SD = 3, ERM_SCORE_COV = 4, ERM_SCORE_ROW_ESS = 5, ERM_SCORE_COARSE = 6, ERM_SCORE_COLS = 7 };
int erm_get_scores(erm_handle h, int32_t n_nodes, double* score, double* out4);
int erm_score(int device, int model, int64_t n_subj, int32_t n_item, int32_t n_feat, const uint8_t* Y, const double* logT, const double* X, const double* rows,
              int64_t n_rows, int32_t n_nodes, int32_t weighting, double* score, double* out4);

/* Plausible values: K draws of (theta_i, zeta_i) from every subject's posterior, the input of a secondary analysis (a regression of ability on covariates, a population
 * variance, a comparison of groups: Mislevy 1991; large-scale assessments publish five per student), from the item-level trace alone.  erm_get_scores gives a point and
 * a standard error; these are draws from the same posterior -- at every row the draw has exactly the mean E_s and the variance V_s (and, for zeta, Ez_s, Vz_s and the
 * covariance C_s) that erm_get_scores reports, with the shape of the rule's posterior, not a Gaussian's.  The traces cannot supply them: ERM_TRACE_SUMMARY keeps no
 * theta or zeta draw, the draws ERM_TRACE_FULL keeps are not draws from the joint model for the response-time models (see erm_get_scores: the sampler's conditionals
 * ignore Sigma_p[1,2]), and a new respondent scored against a saved posterior has no chain.  Computed AFTER the run from resident state, in both trace modes; the calls
 * only read the engine.  Served and refused as erm_get_scores.
 * Definition, for subject i, draw k = 0..K-1, over a table of n_rows item-trace rows (an engine: its post-burn-in rows; a farm: the chain-major table of
 * erm_farm_get_marginal_waic), equal weights:
 *   1. row      r_k = ((2 k + 1) n_rows) / (2 K) in 64-bit integer division: evenly spaced and rising with k, distinct when K <= n_rows, each row m times when K = m n_rows.
 *   2. the rule at row r_k: exactly erm_get_marginal_waic's -- the same population law, item sums, nodes z_q, theta_q and e_q, q = 0..Q-1 -- and from them the row's
 *               M, S, E, V of erm_get_scores and its zeta conditional (c0, c1, u).
 *   3. node     Gumbel-max: key_q = e_q + g_q,  g_q = -log(-log u(w)),  u(w) = (w + 1/2) 2^-32,  w = word 0 of the Philox4x32-10 block with key = seed and
 *               ctr = { i, k, q, 16 << 24 } (stream site 16; the chain bits are zero).  The chosen node q* has the largest key; of equal keys the smaller q wins.  This
 *               picks q with probability w_q = exp(e_q - M) / S, and the maximum is associative: the choice does not depend on how the nodes are dealt to lanes.
 *               The 32-bit uniform bounds g at about 22.9 (and at -3.13 below): a node whose weight is below e^-26 of the largest can never be chosen.
 *   4. theta    one more block at ctr = { i, k, 0xFFFFFFFF, 16 << 24 } with words w0, w1, w2:  theta* = theta_q* + sd h (u(w0) - 1/2), uniform within the node's cell.
 *               That adds sd^2 h^2 / 12 to the row's variance, so it is taken out:  c = sqrt(V / (V + sd^2 h^2 / 12)), c = 0 when V = 0;  theta = E + c (theta* - E).
 *   5. zeta     zeta = c0 + c1 theta + sqrt(u) n,  n = sqrt(-2 log u(w1)) cos(2 pi u(w2)).  GibbsMlIrt has no zeta: its block is NaN.
 *   6. coarse   a subject is coarse if S < 2 at some row it used (the marginal WAIC's rule, over the rows r_k only).
 * Everything is fp64 whatever the engine's precision.  i is the subject's index within the call's data set.  A subject's draws depend on its own data, the rows, Q, K,
 * seed and i only -- not on n_subj, the other subjects, the launch or the chunking, nor on whether draws that share a row share one node pass; nothing is atomic;
 * results are bit-reproducible from call to call and do not depend on how the sweeps were split into erm_run calls.
 * Output: pv, column-major [n_subj][K][2]: the theta block [n_subj][K] first, the zeta block second.  node (may be NULL), int32 column-major [n_subj][K]: q*, for the
 *   tests and to show where a coarse rule put its mass.  coarse (may be NULL), int32 [n_subj]: 1 for a coarse subject, else 0.  out4 (may be NULL) = { n_subj, n_rows, Q,
 *   number of coarse subjects }.  1 <= n_draws <= 4096, else ERM_ERR_ARG; n_nodes as erm_get_marginal_waic.  The draws pass through bounded device scratch: the subjects
 *   go through in chunks of at most 256 MB of draws (ERM_PV_CHUNK in the environment caps the chunk length in subjects: no result changes by a bit); ERM_ERR_NOMEM if
 *   the scratch cannot be had.
 * erm_get_plausible_values: the post-burn-in rows of the resident item trace, read in place.  Refused as erm_get_scores refuses (a quantile model: ERM_ERR_ARG; a shard,
 *   no data set, a failed run, no post-burn-in row: ERM_ERR_STATE); ONE post-burn-in row is enough.  erm_farm_get_plausible_values (below): the same over the farm's
 *   chain-major table on chain 0's device; a farm of one chain returns its engine's result bit for bit.
 * erm_plausible_values: the same kernel on caller-supplied data and rows, validated as erm_score validates them (a NaN: ERM_ERR_NONFINITE; a bad row: ERM_ERR_ARG, the
 *   message names the row); n_rows >= 1.
 * Out of scope: likelihood weighting of the rows (ERM_SCORE_LIKELIHOOD's weights would need a resampling pass over the rows before the draws), the two quantile models,
 * and subject-sharded engines. */
enum { ERM_PV_DRAWS_DEFAULT = 5, ERM_PV_DRAWS_MAX = 4096 };
int erm_get_plausible_values(erm_handle h, int32_t n_nodes, int32_t n_draws, uint64_t seed, double* pv, int32_t* node, int32_t* coarse, double* out4);
int erm_plausible_values(int device, int model, int64_t n_subj, int32_t n_item, int32_t n_feat, const uint8_t* Y, const double* logT, const double* X, const double* rows,
                         int64_t n_rows, int32_t n_nodes, int32_t n_draws, uint64_t seed, double* pv, int32_t* node, int32_t* coarse, double* out4);

/* Incomplete response patterns: respondents who did not see every item (booklet designs, adaptive forms, not-reached items, time limits) scored against a saved
 * posterior -- the three caller-data entries above with an OBSERVED MASK.  Calibration keeps its complete-data contract (erm_set_data takes no mask); scoring,
 * plausible values and the held-out marginal log-likelihood take incomplete respondents.
 * The mask is obs, uint8 [n_subj][n_item], column-major as Y is.  1: the cell was administered, so both its response and its log-time are observed; 0: it was not.
 * O_i = the observed items of subject i in rising item order, n_i = |O_i|.  ONE mask bit per cell: separate response and time masks (an omitted response with a
 * recorded time) are out of scope.
 * Definition.  Everything in the definitions of erm_get_marginal_waic, erm_get_scores and erm_get_plausible_values holds, with three changes:
 *   - "sum over j = 1..J" is read as "sum over j in O_i, in rising order";
 *   - T(theta) takes n_i for J in -(n_i / 2) log 2 pi;
 *   - each of these sums runs over O_i only: A1 = sum y_j a_j, A0 = sum y_j a_j b_j, sum_j log(1 + e^eta_j), and P, R0, R1, D0, D1, D2, L = sum log sig2t_j.
 *   The population law, the node rule, COARSE, the row weights, the row accumulator, the Gumbel-max node choice and its Philox counters (the subject index i within
 *   the call) are unchanged.
 * Consequences:
 *   - n_i = 0 is an ordinary case: every sum is empty and T = 0.  The score is the population law averaged over the rows; zeta | theta ~ N(m0 + m1 theta, v), because
 *     P = 0; l is the log of the rule's total weight.
 *   - Y and logT at unobserved cells are never read: they may be NaN, 255 or anything else; the validation skips them and no result changes by a bit.
 *   - obs == NULL means complete, and the result is the unmasked entry's bit for bit (the unmasked entry is called); n_obs receives n_item.
 *   - with obs all ones the result is also the unmasked entry's bit for bit: lane s of a subject adds the list positions s, s + 8, ... in order, every node's chain
 *     runs over the list in order, and the butterflies are those of the complete kernel.
 *   - a subject with pattern O gives the result of that subject in a data set that has only the items O, scored through the unmasked entry on the rows restricted to
 *     the columns of those items (a, b, lambda, sig2t, and Cross's rho, subset in the same order): the order of every floating-point operation is the same.
 * Work, memory and traffic are proportional to the observed cells: the host compacts every subject's cells into a list (item index, y, logT) while it validates them,
 * and the kernels' item sums and node chains run over the list.
 * n_obs, int32 [n_subj], receives n_i; it may be NULL.  All other outputs, n_nodes, n_draws, weighting and the row limits are the unmasked entries'.  Served: the five
 * models of erm_get_marginal_waic; the quantile models are refused with its messages (erm_quantile_marginal_loglik has no masked sibling).
 * Validation: erm_marginal_loglik's, with these differences -- an obs value above 1: ERM_ERR_ARG; a NaN in logT: ERM_ERR_NONFINITE, and Y > 1: ERM_ERR_ARG, at
 *   observed cells only.  X and the rows are validated as there.
 * PSIS-LOO of incomplete respondents needs nothing new: erm_psis_loo takes the l erm_marginal_loglik_masked returns.
 * The engine and farm entries (erm_get_scores and the others) take no mask: a resident data set is complete by construction. */
int erm_marginal_loglik_masked(int device, int model, int64_t n_subj, int32_t n_item, int32_t n_feat, const uint8_t* Y, const double* logT, const double* X,
                               const uint8_t* obs, const double* rows, int64_t n_rows, int32_t n_nodes, double* l, double* out10, double* lppd_u, double* p_u,
                               int32_t* n_obs);
int erm_score_masked(int device, int model, int64_t n_subj, int32_t n_item, int32_t n_feat, const uint8_t* Y, const double* logT, const double* X, const uint8_t* obs,
                     const double* rows, int64_t n_rows, int32_t n_nodes, int32_t weighting, double* score, double* out4, int32_t* n_obs);
int erm_plausible_values_masked(int device, int model, int64_t n_subj, int32_t n_item, int32_t n_feat, const uint8_t* Y, const double* logT, const double* X,
                                const uint8_t* obs, const double* rows, int64_t n_rows, int32_t n_nodes, int32_t n_draws, uint64_t seed, double* pv, int32_t* node,
                                int32_t* coarse, double* out4, int32_t* n_obs);

/* Person fit: whether a respondent's score can be trusted -- a fit flag beside every score, for the fitted data set, new respondents and incomplete patterns, from the
 * item-level trace alone.  Pre-knowledge, rapid guessing, copying and a speeded ending show as a response pattern or a time pattern that the model finds improbable
 * for that person.  Deterministic (no random numbers); computed AFTER the run from resident state, in both trace modes; the calls only read the engine.  Served: the
 * five models of erm_get_marginal_waic; the two quantile models are refused with ERM_ERR_ARG for its reason.
 * Definition, for subject i at row s.  O_i = the observed items, n = n_i their count (all n_item on complete data).  The population law, the node rule (z_q, theta_q,
 * e_q, M, S) and the item sums (P, R0, R1, D0, D1, D2) are exactly those of erm_get_marginal_waic; (M, S) are its (M, S) bit for bit, so COARSE is its flag.
 *   responses, at node theta_q    eta_j = a_j (theta_q - b_j),  t_j = e^-|eta_j|;  r_j = t_j / (1 + t_j) if (y_j = 1) <=> (eta_j >= 0), else r_j = 1 / (1 + t_j).
 *                      W = sum_{j in O_i} (2 y_j - 1) r_j eta_j  (= l0 - E[l0 | theta], l0 = sum y eta - log(1 + e^eta));
 *                      Vw = sum_{j in O_i} eta_j^2 t_j / (1 + t_j)^2  (= Var[l0 | theta]);   lz(theta_q) = W / sqrt(Vw), and 0 (its Phi: 1/2) when Vw = 0.
 *                      lz is the statistic of Drasgow, Levine and Williams (1985); negative means misfit.  This is the form with no cancellation: W is never formed
 *                      as theta A1 - A0 - sum p eta, which loses every digit at a node where all items are decided (a_j = 8, |eta| > 30).
 *   response times, at node theta_q (models with times)    Qf = D + (P m^2 - 2 R m - v R^2) / (1 + v P), clamped at 0, with R = R0 - theta R1,
 *                      D = D0 - 2 theta D1 + theta^2 D2, m = m0 + m1 theta: exactly -2 (T(theta) - its constants).  Given theta the log-times are
 *                      N(lambda - rho theta - m 1, diag sig2t + v 1 1'); Qf is their Mahalanobis form: chi^2_n exactly, with zeta integrated out.
 *                      tail(theta_q) = P(chi^2_n >= Qf), the finite sum for integer n: with y = Qf / 2, o = n mod 2, m = floor(n / 2),
 *                        base = o ? erfc(sqrt y) : 0,  t_0 = e^-y (o ? 2 sqrt(y / pi) : 1),  t_k = t_(k-1) y / (k + o / 2),  tail = base + sum_{k < m} t_k;  0 for y > 700.
 *                      ltz(theta_q) = ((Qf / n)^(1/3) - (1 - 2 / (9 n))) / sqrt(2 / (9 n)): Wilson-Hilferty's z, positive means misfit.  Descriptive: it is not
 *                      used for the p-value.
 *   at the row         four weighted means under w_q = exp(e_q - M) / S:  LZ_s = sum w_q lz(theta_q),  PY_s = sum w_q Phi(lz(theta_q)), Phi(x) = erfc(-x / sqrt 2) / 2,
 *                      LTZ_s = sum w_q ltz(theta_q),  PT_s = sum w_q tail(theta_q).  The six running sums S, S LZ, S PY, S LTZ, S PT and M stream and merge under the
 *                      running maximum exactly as the scores' sums do.  PY and PT are posterior predictive p-values with a realised discrepancy (Gelman, Meng and
 *                      Stern 1996): PY through lz's normal approximation, PT exact given theta.  Small means misfit for both.
 *   across the rows    in trace order, with weight omega_s = 1 (ERM_SCORE_EQUAL) or exp(l_s - Lambda) with the running-maximum rescale (ERM_SCORE_LIKELIHOOD), as
 *                      erm_get_scores: the weighted running means of the four row values;  row_ess = (sum omega)^2 / sum omega^2.
 * Output: fit, column-major [n_subj][6], column ERM_FIT_*; COARSE is 1.0 if S < 2 at some row and 0.0 otherwise.  out4 (may be NULL) = { n_subj, n_rows, Q, number of
 *   coarse subjects }.  GibbsMlIrt gets NaN in LTZ and P_TIME.  A subject with n_i = 0 gets NaN in all four statistic columns; ROW_ESS and COARSE stay ordinary.
 *   Everything is fp64 whatever the engine's precision; every sum has a fixed order and nothing is atomic; a subject's result depends on its own data, the rows, Q and
 *   the weighting only; results are bit-reproducible from call to call and do not depend on how the sweeps were split into erm_run calls.
 * erm_get_person_fit: the post-burn-in rows of the resident item trace, read in place, equal weights.  n_nodes and the refusals as erm_get_scores' (a shard, no data
 *   set, a failed run, no post-burn-in row: ERM_ERR_STATE, the words name "the person fit"); ONE post-burn-in row is enough.  erm_farm_get_person_fit (below): the
 *   same over the farm's chain-major table on chain 0's device.
 * erm_person_fit: the same kernel on caller-supplied data and rows, validated as erm_score validates them; n_rows >= 1; an unknown weighting: ERM_ERR_ARG.
 * erm_person_fit_masked: erm_person_fit with the observed mask of erm_score_masked, with its validation and its n_obs; obs == NULL calls erm_person_fit.
 * Out of scope: the quantile models, separate response and time masks, a joint p-value. */
enum { ERM_FIT_LZ = 0, ERM_FIT_P_RESP = 1, ERM_FIT_LTZ = 2, ERM_FIT_P_TIME = 3, ERM_FIT_ROW_ESS = 4, ERM_FIT_COARSE = 5, ERM_FIT_COLS = 6 };
int erm_get_person_fit(erm_handle h, int32_t n_nodes, double* fit, double* out4);
int erm_person_fit(int device, int model, int64_t n_subj, int32_t n_item, int32_t n_feat, const uint8_t* Y, const double* logT, const double* X, const double* rows,
                   int64_t n_rows, int32_t n_nodes, int32_t weighting, double* fit, double* out4);
int erm_person_fit_masked(int device, int model, int64_t n_subj, int32_t n_item, int32_t n_feat, const uint8_t* Y, const double* logT, const double* X, const uint8_t* obs,
                          const double* rows, int64_t n_rows, int32_t n_nodes, int32_t weighting, double* fit, double* out4, int32_t* n_obs);

/* Item fit and drift: whether saved item parameters still hold for a sample -- the fitted one or, above all, a NEW one scored against a saved calibration (a leaked
 * item that has become easier and faster, a translated item that behaves differently, an item whose times drift at the end of a booklet).  Per item: infit and outfit
 * mean squares, a signed response residual, a response-time mean square and a signed response-time residual, from the item-level trace alone.  Deterministic;
 * computed AFTER the run from resident state, in both trace modes; the calls only read the engine.  Served: the five models of erm_get_marginal_waic; the two quantile
 * models are refused with ERM_ERR_ARG for its reason.
 * Definition.  Subject i, row s, O_i the observed items.  For an observed cell (i, j) at node theta_q the law (mu, sd, m0, m1, v; v clamped at 0, m = m0 + m1 theta_q),
 * the node rule, e_q, M, S, w_q = exp(e_q - M) / S and the item sums P, R0, R1 are erm_get_person_fit's unchanged: (M, S) and COARSE are the marginal WAIC's bit for bit.
 *   responses          eta = a_j (theta_q - b_j), t = e^-|eta|;  "agree" means (y = 1) <=> (eta >= 0).
 *                      r = t / (1 + t) if agree, else 1 / (1 + t)  (= |y - p|);   c = t / (1 + t)^2  (= p (1 - p));
 *                      z^2 = t if agree, else exp(min(|eta|, 700))  (= r^2 / c without the cancellation; the clamp keeps every term finite -- the library clamps
 *                      |eta| inside t as well, which moves r and c by less than 1e-304);   signed residual e = (2 y - 1) r.
 *   response times (models with times)   u = lambda_j - rho_j theta_q - logT_ij, g = 1 / sig2t_j, R = R0 - theta_q R1.  The residual is the leave-one-item-out
 *                      prediction given theta and the subject's OTHER observed times, with zeta integrated out:
 *                        Pi = 1 + v (P - g),   m_ = (m + v (R - g u)) / Pi,   v_ = v / Pi,   d = -(u - m_) / sqrt(sig2t_j + v_).
 *                      Positive d: slower than predicted; d^2 is exactly chi^2_1 given theta.  The form has no 1 / v: v = 0 is an ordinary case.  (The marginal
 *                      residual (u - m)^2 / (sig2t + v) is less sharp: on an item whose time variance was quadrupled it read 2.4 .. 2.9 where this reads 3.6 .. 4.1.)
 *   per cell           six posterior means under w_q: E[e], E[r^2], E[c], E[z^2], E[d], E[d^2]; averaged over the rows with EQUAL weights, in trace order.  There is no
 *                      likelihood weighting (the normaliser of a subject's row weights is known only after the last row), so the entries take no weighting.
 *   per item           sums over the subjects i with j in O_i, n_j their count:
 *                        ERM_IFIT_INFIT   = sum E[r^2] / sum E[c]        mean square, about 1
 *                        ERM_IFIT_OUTFIT  = sum E[z^2] / n_j             mean square, outlier-sensitive (long upper tail on very easy or very hard items)
 *                        ERM_IFIT_RESP_Z  = sum E[e] / sqrt(sum E[c])    signed; negative = harder than calibrated
 *                        ERM_IFIT_RT_MSQ  = sum E[d^2] / n_j             about 1
 *                        ERM_IFIT_RT_Z    = sum E[d] / sqrt(n_j)         signed; positive = slower than calibrated
 *                        ERM_IFIT_N_OBS   = n_j
 * Output: fit, column-major [n_item][ERM_IFIT_COLS].  out4 (may be NULL) = { n_subj, n_rows, Q, number of coarse subjects }.  GibbsMlIrt gets NaN in the two RT columns;
 *   an item nobody observed (n_j = 0) gets NaN in the five statistics.  Everything is fp64 whatever the engine's precision.  Nothing is atomic: every word of the
 *   per-cell workspace has one writer, and the sums over the subjects have one order -- blocks of 256 consecutive subjects by global index, each by a fixed binary tree
 *   (absent subjects count 0), then the block sums in rising block order -- so results are bit-reproducible from call to call and do not depend on the chunking.
 * Reading.  The mean squares alone do not find drift reliably (a difficulty shifted by one logit left infit between 0.89 and 1.42); the signed columns do.  A misfit
 *   that a free a_j or sig2t_j can absorb -- a coin-toss item fitted with a about 0 -- leaves every column near its null value when the item is checked on its own
 *   calibration sample: that is inherent to a 2PL.  Check a second sample against the saved rows (erm_item_fit).
 * erm_get_item_fit: the post-burn-in rows of the resident item trace, read in place.  n_nodes and the refusals as erm_get_person_fit's (a shard, no data set, a failed
 *   run, no post-burn-in row: ERM_ERR_STATE, the words name "the item fit"); ONE post-burn-in row is enough.  erm_farm_get_item_fit (below): the same over the farm's
 *   chain-major table on chain 0's device.
 * erm_item_fit: the same kernels on caller-supplied data and rows, validated as erm_person_fit_masked validates them; n_rows >= 1.  obs may be NULL: complete data, the
 *   unmasked kernel; obs of all ones gives its result bit for bit.
 * Out of scope: the quantile models, likelihood row weights, separate response and time masks, standardised mean squares (ZSTD), group-wise DIF beyond one call per
 *   group. */
enum { ERM_IFIT_INFIT = 0, ERM_IFIT_OUTFIT = 1, ERM_IFIT_RESP_Z = 2, ERM_IFIT_RT_MSQ = 3, ERM_IFIT_RT_Z = 4, ERM_IFIT_N_OBS = 5, ERM_IFIT_COLS = 6 };
int erm_get_item_fit(erm_handle h, int32_t n_nodes, double* fit, double* out4);
int erm_item_fit(int device, int model, int64_t n_subj, int32_t n_item, int32_t n_feat, const uint8_t* Y, const double* logT, const double* X, const uint8_t* obs,
                 const double* rows, int64_t n_rows, int32_t n_nodes, double* fit, double* out4);

/* Marginal PSIS-LOO: Pareto-smoothed importance-sampling leave-one-subject-out (Vehtari, Gelman and Gabry 2017; Vehtari, Simpson, Gelman, Yao and Gabry 2024), the
 * criterion the "p_u > 0.4" count of erm_get_waic / erm_get_marginal_waic sends its reader to, and with it a Pareto k^ per respondent: for which respondents the
 * posterior would move if they were left out -- the aberrant or highly influential response / time patterns.  (ERM_SCORE_LIKELIHOOD importance-weights the rows with raw
 * weights; this is the stabilised form of that idea, with a diagnostic.)  It sits on l_s = l_i^(s) of erm_get_marginal_waic, the marginal log-likelihood of subject i at
 * row s, so it too is computed AFTER the run from resident state, in both trace modes, and the calls only read the engine.  Served and refused as erm_get_marginal_waic
 * serves and refuses (the two quantile models: ERM_ERR_ARG).  Everything is fp64 whatever the engine's precision.  Relative efficiency is taken as 1, as the R
 * package loo does when none is supplied.
 * Definition, for one unit with the values l_s, s = 1..S, in trace order (an engine: the post-burn-in rows behind Post.mean; a farm: the chain-major table of
 * erm_farm_get_marginal_waic).  Limits: 25 <= S <= 8192 (ERM_ERR_ARG, the message names the limit): the lower one gives M >= 5, the upper one is that of the sort in LDS
 * (the cap of erm_get_rank_diagnostics).
 *   1. log ratios   lw_s = -l_s - max_t(-l_t): the largest is 0.
 *   2. order        ascending by (lw, position s): the position breaks ties (the sorting network of erm_get_rank_diagnostics).
 *   3. tail         M = min(ceil(S / 5), ceil(3 sqrt(S))) in integers (ceil(3 sqrt(S)) = the smallest m with m^2 >= 9 S; the arms cross at S = 225); the tail is the M
 *                   largest; the cutoff c = the sorted value number S - M (1-based), the largest outside the tail; exceedances x_i = exp(tail_i) - exp(c), i = 1..M, ascending.
 *   4. fit          (Zhang and Stephens 2009)  G = 30 + floor(sqrt(M)),  x* = x[floor(M / 4 + 0.5)] (1-based),  b_j = 1 / x_M + (1 - sqrt(G / (j - 0.5))) / (3 x*), j = 1..G,
 *                   k_j = mean_i log1p(-b_j x_i),  L_j = M (log(-b_j / k_j) - k_j - 1),  w_j = exp(L_j - LSE(L)),  b^ = sum_j b_j w_j,  k_raw = mean_i log1p(-b^ x_i),
 *                   sigma = -k_raw / b^,  k^ = (M k_raw + 5) / (M + 10).  Sums over i run i = 1..M in order, sums over j run j = 1..G in order, LSE(L) = max + log sum exp(L_j - max).
 *                   Unfittable tail: x* <= 0, or x_M - x_1 <= 0, or any of b^, sigma, k^ not finite: k^ = +Inf and the weights stay unsmoothed.
 *   5. smoothing    p_i = (i - 1/2) / M,  tail_i <- min(0, log(exp(c) + sigma expm1(-k^ log1p(-p_i)) / k^)), at k^ = 0 the limit -sigma log1p(-p_i); assigned in sorted order.
 *   6. per unit     with lw' the smoothed log ratios:  elpd_i = LSE_s(lw'_s + l_s) - LSE_s(lw'_s),  p_i = lppd_i - elpd_i with lppd_i = max l + log(sum_s exp(l_s - max l) / S)
 *                   (erm_get_marginal_waic's lppd_i),  neff_i = (sum w)^2 / sum w^2 with w = exp(lw'),  k^_i.
 *                   A sum over s is taken in the SORTED order of step 2: 256 partial sums (sorted value number p, 0-based, goes to partial p mod 256, in rising p), a
 *                   binary tree over each run of 64 partials (partial q += partial q + 32, then + 16, ... + 1), the four runs added in order; each LSE about its maximum.
 *   7. out12        { elpd_loo = sum_u elpd_u, p_loo = sum_u p_u, looic = -2 elpd_loo, se = 2 sqrt(U Var_u(elpd_u)) (U - 1 in the denominator, the squared deviations
 *                   about the mean in a second pass: as se_waic), lppd = sum_u lppd_u, n_units, n_rows = S, #(k^ > 0.7) (Inf included), #(k^ > min(1 - 1 / log10(S), 0.7)),
 *                   M, Q, number of coarse units }.  A sum over the units: 256 partial sums (unit u to partial u mod 256, in rising u), the same tree, the four runs in order.
 * Nothing is atomic.  A unit's result depends on its own l_s only -- not on n_subj, the other units, the launch, the chunking or how many units share a workgroup
 * (one wave carries a unit up to 2048 padded rows, two up to 4096, a workgroup beyond: the order of every sum is the same in all three).  Results are
 * bit-reproducible from call to call.
 * What k^ means: the estimated shape of the tail of unit i's importance ratios.  k^ <= min(1 - 1 / log10(S), 0.7): elpd_i is reliable.  Above: the posterior without
 * respondent i differs from the full posterior by more than S rows can correct -- the respondent is influential or poorly described by the model; elpd_i is optimistic.
 * erm_get_marginal_loo: out12 as above; pw, column-major [n_subj][4] with the columns ERM_LOO_*, may be NULL.  n_nodes as erm_get_marginal_waic.  l is produced by the
 *   marginal WAIC's kernel into bounded device scratch -- the subjects go through in chunks of at most 256 MB of l (twice that is held: l and its transpose), then
 *   the PSIS kernel runs on the chunk; ERM_ERR_NOMEM if the scratch cannot be had.  Refused: as erm_get_marginal_waic (a quantile model: ERM_ERR_ARG; a shard, no data
 *   set, a failed run: ERM_ERR_STATE), and S outside 25 .. 8192 (ERM_ERR_ARG).
 * erm_farm_get_marginal_loo (below): the same over the farm's chain-major table on chain 0's device; every chain must have recorded the same number of rows, at least one
 *   of them post-burn-in (ERM_ERR_STATE, the message names the chain), S = all chains' post-burn-in rows.  A farm of one chain returns its engine's result bit for bit.
 * erm_psis_loo: the same kernel on a caller-supplied l, column-major [n_subj][n_rows] (the subject fastest), exactly what erm_marginal_loglik returns; lw (may be NULL)
 *   receives the smoothed, normalised log-weights lw' - LSE(lw') in the same layout.  Q and the coarse count are 0.  A NaN or an infinity in l: ERM_ERR_NONFINITE.
 *   Serves saved log-likelihood tables, conditional ones included, and the tests. */
enum { ERM_LOO_ELPD = 0, ERM_LOO_P = 1, ERM_LOO_KHAT = 2, ERM_LOO_NEFF = 3, ERM_LOO_COLS = 4 };
int erm_get_marginal_loo(erm_handle h, int32_t n_nodes, double* out12, double* pw);
int erm_psis_loo(int device, const double* l, int64_t n_subj, int64_t n_rows, double* out12, double* pw, double* lw);

/* Posterior predictive checks (Gelman, Meng and Stern 1996; Sinharay 2006; Glas and Meijer 2003; Marianti et al. 2014), drawn and accumulated on the device.  The
 * reference has no counterpart.  Post-burn-in row number k = 1, 2, ... (the rows behind Post.mean) is a REPLICATE row when (k - 1) mod thin = 0.  At a replicate
 * row the whole data set is drawn again from the model at the values of that row -- the law whose log-density is WAIC's cell term: y_rep ~ Bernoulli(p),
 * p = 1 / (1 + e^-eta), eta = a_j (theta_i - b_j); logT_rep = mu + sqrt(var) z with WAIC's mean and variance, z standard normal -- from ONE Philox4x32-10 block per
 * cell at stream (site 14, subject, item, sweep, chain): y_rep = [u(w0) < p], z = sqrt(-2 log u(w1)) cos(2 pi u(w2)), u(w) = (w + 1/2) 2^-32.  The draws depend on
 * (seed, chain, subject, item, sweep) only.  Three discrepancies of the replicate are compared with the same discrepancies of the data:
 *   RA     responses, the deviance:        D = -2 sum (y eta - log(1 + e^eta));  D_rep - D_obs = 2 sum (y - y_rep) eta, an exact zero when the replicate repeats the data
 *   RT     response times, chi^2:          D_obs = sum (logT - mu)^2 / var,  D_rep = sum z^2                      (NaN for GibbsMlIrt)
 *   SCORE  the item score (items only):    T_obs = sum_i y_ij,  T_rep = sum_i y_rep,ij
 * for every subject (over its items), every item (over all subjects) and the data set.  Per unit and component four doubles, updated once per replicate row in trace
 * order: { n_ge = #(rep >= obs), n_gt = #(rep > obs), mean of obs, mean of rep }; with R = erm_predictive_reps the posterior predictive p-value is n_ge / R and its
 * mid-p form (n_gt + (n_ge - n_gt) / 2) / R (a person with few items often replicates its responses exactly: a tie).
 * erm_set_predictive(h, on, thin) enables (on != 0; thin >= 1, else ERM_ERR_ARG) or disables it; 64 bytes of device memory per subject and 96 per item, a few MB
 * of workgroup partial sums, and GibbsRtIrtCrossQr's copy of nu_t as for WAIC.  Like erm_set_pointwise it is allowed only while no trace row is recorded
 * (ERM_ERR_STATE otherwise), refused on a subject-sharded engine (ERM_ERR_STATE), and ERM_ERR_NOMEM leaves the engine as it was.  From then on every sweep is followed
 * by one streaming pass over the resident data set and a one-workgroup item step (on the stream and inside the captured graphs; rows that are no replicate rows
 * return at once; with WAIC enabled too, both passes run), and small data sets are run one launch per sweep at the persistent schedule's geometry
 * (erm_timing.persistent = 0): the chain itself is bit for bit the chain without it.  All sums are order-deterministic (no atomics) at a geometry that depends on
 * (n_subj, n_item) only: the accumulators are bit-reproducible and do not depend on lanes_per_row / block_threads / grid_blocks, the schedule or how the sweeps
 * are split into erm_run calls.  In profile mode the event bracket of a timed sweep also holds the pass.  erm_reset_trace and erm_set_seed clear the accumulators
 * and the replicate count.  The chain farm has no predictive checks yet.
 * erm_get_predictive (needs R >= 1, else ERM_ERR_STATE; any pointer may be NULL):
 *   item  [3][4][n_item]   components RA, RT, SCORE x { n_ge, n_gt, mean_obs, mean_rep } x item
 *   subj  [2][4][n_subj]   components RA, RT
 *   total [2][4]           components RA, RT */
enum { ERM_PPC_RA = 0, ERM_PPC_RT = 1, ERM_PPC_SCORE = 2 };
int erm_set_predictive(erm_handle h, int on, int32_t thin);
int64_t erm_predictive_reps(erm_handle h);
int erm_get_predictive(erm_handle h, double* item, double* subj, double* total);

int erm_get_timing(erm_handle h, erm_timing* out);
/* Subject sharding of ONE chain over several devices (second bullet).  The reference has no counterpart: its
 * conditionals (src/Draw.pl.jl:36-606) make subjects independent given the item / structural parameters, so each device keeps
 * n_subj of the n_subj_total subjects (local row 0 is subject row_base), every device repeats the tiny step on identical inputs, and
 * the only exchange is an all-gather of one row of sufficient statistics per row pass (stat width x 8 bytes per device) plus two
 * all-gathers of column sums inside erm_set_data.  Random streams are addressed by the global subject index: a sharded chain equals
 * the unsharded one up to the summation order of the statistics.
 * `exchange` is the caller's all-gather: it must place device r's `bytes_per_rank` bytes from `dev_send` at
 * dev_recv + r * bytes_per_rank on every device, return 0 when dev_recv is complete, non-zero on failure (erm_run then returns
 * ERM_ERR_STATE).  Both pointers are device memory of this engine; the engine's stream is idle during the call.  The library itself
 * stays free of any communication dependency: the host side plugs in RCCL (torch.distributed) or whatever moves the bytes.
 * Call after erm_create and before erm_set_data, on every device with the same count / n_subj_total and disjoint row ranges.
 * theta / zeta / nu in erm_state, the subject blocks of the traces and erm_get_mean cover the LOCAL subjects; item and structural
 * entries are identical on all devices.  erm_simulate_data is not available on a shard. */
typedef int (*erm_exchange_fn)(void* user, const void* dev_send, void* dev_recv, size_t bytes_per_rank);
int erm_set_shard(erm_handle h, int rank, int count, int64_t n_subj_total, int64_t row_base, erm_exchange_fn exchange, void* user);
/* The same, with the all-gather enqueued by the library itself on the engine's stream over RCCL (xGMI): no host synchronisation per
 * pass, the one-launch-per-sweep schedule and hipGraph replay stay in force.  RCCL is bound at run time (dlopen; ERM_RCCL_LIB
 * overrides the name), so nothing changes for callers that never shard.  erm_rccl_unique_id fills the 128-byte ncclUniqueId on ONE
 * process; the caller hands it to all ranks (any transport), then every rank calls erm_set_shard_rccl (collective: ncclCommInitRank). */
int erm_rccl_unique_id(void* out128);
int erm_set_shard_rccl(erm_handle h, int rank, int count, int64_t n_subj_total, int64_t row_base, const void* unique_id128);
/* hipMemcpy(dst, src, bytes, hipMemcpyDefault): lets a host-side exchange stage the buffers above without binding HIP itself. */
int erm_copy(void* dst, const void* src, size_t bytes);

/* Chain farm: the reference's nChain chains as INDEPENDENT chains, one per GPU (north_star).  Replaces the chain index of
 * `for m in 1:nIter, l in 1:nChain` (src/GibbsRtIrt.pl.jl:289) and the joint mean over iterations and chains (:327-343).  Chain l runs on
 * HIP device devices[l] (devices may repeat) with random stream chain_id = l and a full copy of the data; cfg->device, cfg->chain_id and
 * cfg->n_chain are ignored (every chain records cfg->n_iter rows).  One host thread per chain inside the library drives that chain's
 * stream, so the chains sample concurrently and never communicate.  erm_farm_get_mean is the only collective: the post-burn-in sums
 * of the chains on one device are added on that device, the devices' vectors are summed by ONE ncclAllReduce (RCCL over xGMI, bound at
 * run time as for erm_set_shard_rccl; skipped when all chains share one device unless ERM_FLAG_FARM_FORCE_RCCL is set) and divided by the
 * total number of post-burn-in rows.  Deliberate deviation from the reference: its nChain > 1 is ONE chain whose sweeps are dealt
 * round-robin to nChain trace slabs (erm_create with n_chain > 1 reproduces that); independent chains leave Post.mean unchanged in
 * expectation and make R-hat meaningful.
 * erm_farm_get_trace fills Post.ra / rt / qr / logLike [nIter][width][nChain] with chain l in slab l.  erm_farm_engine lends chain l's
 * engine (owned by the farm) for erm_get_item_trace / erm_get_diagnostics / erm_get_timing: erm_get_diagnostics (and erm_get_rank_diagnostics) on it remains the
 * diagnostic of that ONE chain, M = 2 split halves, blind to the other chains.  erm_farm_get_diagnostics and its three siblings below add what several chains are
 * run for: the estimators over all chains jointly, between-chain variance included. */
typedef struct erm_farm* erm_farm_handle;
int erm_farm_create(const erm_config* cfg, const int32_t* devices, int32_t n_chains, erm_farm_handle* out);
void erm_farm_destroy(erm_farm_handle f);
int32_t erm_farm_chains(erm_farm_handle f);
erm_handle erm_farm_engine(erm_farm_handle f, int32_t chain);
int erm_farm_set_data(erm_farm_handle f, const uint8_t* Y, const double* logT, const double* X);   /* as erm_set_data, to every chain */
int erm_farm_set_state(erm_farm_handle f, int32_t chain, const erm_state* st);                     /* each chain's own setInitialValues */
int erm_farm_get_state(erm_farm_handle f, int32_t chain, erm_state* st);
int erm_farm_run(erm_farm_handle f, int64_t nsweeps);                                              /* nsweeps sweeps of EVERY chain, concurrently */
int erm_farm_reset_trace(erm_farm_handle f);
int erm_farm_get_trace(erm_farm_handle f, int which, double* out);
int erm_farm_get_mean(erm_farm_handle f, erm_state* out);
int erm_farm_get_dic(erm_farm_handle f, double* out4);     /* as erm_get_dic: Dbar over the rows of all chains, Dhat at the joint Post.mean (the same reduction as erm_farm_get_mean, evaluated on the first device) */
int erm_farm_get_marginal_waic(erm_farm_handle f, int32_t n_nodes, double* out10, double* lppd_u, double* p_u);   /* the marginal WAIC over the rows of all chains: see erm_get_marginal_waic */
int erm_farm_get_scores(erm_farm_handle f, int32_t n_nodes, double* score, double* out4);                          /* the scores over the rows of all chains: see erm_get_scores */
int erm_farm_get_person_fit(erm_farm_handle f, int32_t n_nodes, double* fit, double* out4);                        /* the person fit over the rows of all chains: see erm_get_person_fit */
int erm_farm_get_item_fit(erm_farm_handle f, int32_t n_nodes, double* fit, double* out4);                          /* the item fit over the rows of all chains: see erm_get_item_fit */
int erm_farm_get_quantile_marginal_waic(erm_farm_handle f, int32_t n_nodes, double* out10, double* lppd_u, double* p_u);   /* LatentQr: see erm_get_quantile_marginal_waic */
int erm_farm_get_quantile_marginal_loo(erm_farm_handle f, int32_t n_nodes, double* out12, double* pw);                        /* LatentQr: see erm_get_quantile_marginal_waic */
int erm_farm_get_marginal_loo(erm_farm_handle f, int32_t n_nodes, double* out12, double* pw);                        /* the marginal PSIS-LOO over the rows of all chains: see erm_get_marginal_loo */
int erm_farm_get_plausible_values(erm_farm_handle f, int32_t n_nodes, int32_t n_draws, uint64_t seed, double* pv, int32_t* node, int32_t* coarse, double* out4);   /* plausible values over the rows of all chains: see erm_get_plausible_values */
int erm_farm_set_seed(erm_farm_handle f, uint64_t seed);
/* The farm's joint convergence diagnostics: the estimators of erm_get_diagnostics / erm_get_convergence / erm_get_rank_diagnostics / erm_get_rank_convergence, as
 * defined there, applied to the L = erm_farm_chains chains jointly -- chain l takes the place of interleaved chain l: M = 2 L sequences of
 * n = floor((n_iter - n_burnin) / 2) draws, S = M n pooled draws for the rank estimators.  Same NaN rules, same -M n case, same stop rule, same thresholds for the
 * counts; width erm_trace_width(erm_farm_engine(f, 0), which); output in the caller's column order (GibbsRtIrtCrossQr's nu block column-major, as erm_get_diagnostics
 * returns it).  A farm of one chain returns what erm_get_diagnostics of its engine returns, bit for bit.
 * Everything is computed on the device of chain 0 by the kernels the engine entries run: a gather kernel copies the post-burn-in rows of a chunk of columns of every
 * chain into one interleaved scratch (at most 256 MB of gathered draws a chunk; the rank estimators stage as much again), and the full traces never cross to the
 * host.  A chain on another device compacts its chunk into a slab there, which is copied to chain 0's device (hipMemcpyPeerAsync; peer access is not enabled and
 * no device setting is touched).  The calls only read the farm.  ERM_FARM_DIAG_CHUNK (environment) caps the chunk length in columns and ERM_FARM_DIAG_REMOTE=1
 * sends every chain but chain 0 through the slab path whatever its device: neither changes a result by a bit (tests).
 * Limits: at most 16 chains and at least 8 post-burn-in iterations (ERM_ERR_ARG); the rank entries also S <= 8192 (ERM_ERR_ARG, the message names the cap); every
 * chain has recorded all n_iter rows (ERM_ERR_STATE, the message names the chain); ERM_TRACE_FULL, and the nu block recorded for GibbsRtIrtCrossQr's qr
 * (ERM_ERR_NOTRACE); `which` = ERM_TRACE_LOGLIKE or a trace the model lacks: ERM_ERR_ARG; no scratch: ERM_ERR_NOMEM.  NULL outputs as the engine entries treat
 * them: ess, rhat, counts4 and counts6 are required, any of the three rank vectors may be NULL. */
int erm_farm_get_diagnostics(erm_farm_handle f, int which, double* ess, double* rhat);
int erm_farm_get_convergence(erm_farm_handle f, int which, int64_t* counts4);
int erm_farm_get_rank_diagnostics(erm_farm_handle f, int which, double* ess_bulk, double* ess_tail, double* rhat_rank);
int erm_farm_get_rank_convergence(erm_farm_handle f, int which, int64_t* counts6);
int64_t erm_farm_post_count(erm_farm_handle f);
int erm_farm_used_rccl(erm_farm_handle f);                  /* 1 if the last erm_farm_get_mean reduced over RCCL */
/* What a multi-GPU benchmark of the farm reports: wall-clock of the last erm_farm_run (all chains, host side), the device time of each chain's
 * last erm_run (run_ms[n_chains], may be NULL), the wall-clock of the last erm_farm_get_mean (without the one-off communicator creation) and of its all-reduce alone, and the number of ranks
 * of the library's own RCCL communicator (ncclCommCount; 0 if no communicator exists). */
typedef struct {
    double run_wall_ms, gather_ms, allreduce_ms;
    double comm_init_ms;    /* ncclCommInitAll, paid by the first erm_farm_get_mean over more than one device (not part of gather_ms) */
    int32_t rccl_ranks, n_devices;
} erm_farm_timing;
int erm_farm_get_timing(erm_farm_handle f, erm_farm_timing* out, double* run_ms);

const char* erm_last_error(void);
const char* erm_version(void);
/* Layout version of the structs above (erm_config, erm_timing, ...): a binder compares it with the ERM_ABI_VERSION it was written against before the first
 * erm_create.  4: erm_timing grew by persist_fallbacks; erm_config.flags refuses unknown bits. */
#define ERM_ABI_VERSION 4
int erm_abi_version(void);

/* Diagnostics: run a device sampler on n independent streams (stream k = (seed, site, i=k, sweep)); used by the parity
 * tests to compare the device restatement of each sampler with the oracle.  which: 0 uniform, 1 normal, 2 expo,
 * 3 PG(1, par0), 4 IG(par0, par1), 5 TN(par0, par1; 0, inf), 6 Gamma(par0), 7 PG mixture weight(par0), 8 QR weight(par0, par1),
 * 9 normal quantile(par0), 10 PG(1, par0) through the reference form of the attempt (fp64: every decision in fp64),
 * 11-14 the fp64 cell path's log(par0), exp(-par0), sqrt(par0), par0 / par1; 15 its table-driven log(par0), 16 cos(2 pi par0), 17 its form of the QR weight (par0 = |residual|, par1 = parB at unit scale: the same variate as 8),
 * 18 the cell log-likelihood's exp(-par0), 19 log((w + 1/2) 2^-32) of the 32-bit word w = par0 (the PG attempt's logarithm of a uniform). */
int erm_debug_sample(int device, int precision, int which, uint64_t seed, uint32_t site, uint32_t sweep, int64_t n,
                     const double* par0, const double* par1, double* out);

/* n draws of the 2 x 2 InverseWishart(nu, Psi) of drawSubjCovariance (src/Draw.pl.jl:499-515) through the device code the structural step runs (Bartlett factor of
 * the Wishart on Psi^-1, then the inverse): out[4 k .. 4 k + 3] = vec(Sigma) of draw k, which uses stream (seed, site SIGP, i = k, sweep).  psi = vec(Psi). */
int erm_debug_invwishart(int device, uint64_t seed, uint32_t sweep, int64_t n, double nu, const double* psi4, double* out);

/* checkConvergence's four counts of n caller-supplied ess / rhat values, through the device code erm_get_convergence runs on its own vectors (the same kernel, the
 * same thresholds ESS > 400 and R-hat < 1.1, both strict; a NaN is "not defined" and enters no count): lets a test put values ON the thresholds, where a sampler's
 * trace never lands.  counts4 as for erm_get_convergence. */
int erm_debug_convergence(int device, int64_t n, const double* ess, const double* rhat, int64_t* counts4);

/* erm_get_rank_diagnostics' kernels on caller-supplied draws x[n_draw][n_col][n_chain] (Julia layout, the draw fastest, already post-burn-in): the same staging
 * and rank kernels, at n_iter = n_draw and n_burnin = 0.  precision ERM_PREC_F32 rounds x to float on upload (the fp32 engines' trace type); the diagnostics
 * themselves are fp64 either way.  Any of the three output pointers (n_col doubles each) may be NULL.  Limits as for erm_get_rank_diagnostics; a NaN in x:
 * ERM_ERR_NONFINITE.  Serves traces that are not resident on one device (erm_farm_get_trace output) and the tests. */
int erm_debug_rank_diagnostics(int device, int precision, const double* x, int64_t n_draw, int64_t n_col, int32_t n_chain,
                               double* ess_bulk, double* ess_tail, double* rhat_rank);

/* The same for the basic estimator: erm_get_diagnostics' kernel (diag_kernel, at n_iter = n_draw and n_burnin = 0) on caller-supplied draws x[n_draw][n_col][n_chain],
 * with the same layout, the same rounding to float under ERM_PREC_F32 and the same refusal of a NaN (ERM_ERR_NONFINITE).  ess and rhat (n_col doubles each) are
 * required; at least 8 draws and at most 16 chains (ERM_ERR_ARG). */
int erm_debug_diagnostics(int device, int precision, const double* x, int64_t n_draw, int64_t n_col, int32_t n_chain, double* ess, double* rhat);

/* n draws of the generalized inverse Gaussian GIG(p, a, b) (density ~ x^(p-1) exp(-(a x + b/x)/2); the distribution type of
 * src/GenInvGaussian.jl:17-30, whose sampler :76-106 is dead code in the reference) by Devroye's (2014) sampler, fp64; element k uses
 * stream (seed, site, i = k, sweep).  The live quantile weights are the p = -1/2 case and use the inverse-Gaussian sampler. */
int erm_sample_gig(int device, uint64_t seed, uint32_t site, uint32_t sweep, int64_t n, double p, double a, double b, double* out);

#ifdef __cplusplus
}
#endif
#endif

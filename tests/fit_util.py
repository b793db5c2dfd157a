"""Helpers shared by the tests of the person fit (tests/test_fit_host.py, tests/test_gpu_person_fit.py): an independent reference for one subject
-- scipy.integrate.quad over theta with scipy's own chi2.sf and norm.cdf, the quadratic form by numpy.linalg.solve on the dense covariance --, simulated data with
planted aberrant respondents, the one table of cases at which the kernel is compared with the twin, and the comparison of two results."""
import functools

import numpy as np

import marginal_util as mu
import obs_util as ou
import parity_util as pu

COLS = ("lz", "pResp", "ltz", "pTime", "rowEss")
STATS = COLS[:4]
WEIGHTINGS = ("equal", "likelihood")
COARSE_S, S_MARGIN = 2.0, 0.1


def pkg():
    return pu.ge.load_package()


def dense_quad(sg, lam, t, rho, m0, m1, v, th):
    """The Mahalanobis form of the log-times given theta by numpy.linalg.solve on diag(sig2t) + v 1 1'."""
    d = t - (lam - (m0 + m1 * th) - rho * th)
    return float(d @ np.linalg.solve(np.diag(sg) + v * np.ones((sg.size, sg.size)), d))


def quad_row(model, y, t, x, row):
    """(LZ, PY, LTZ, PT, l) of subject (y, t, x) at `row`: the means of lz, norm.cdf(lz), Wilson-Hilferty's z and chi2.sf under the posterior of theta, by
    scipy.integrate.quad with marginal_util.quad_l's integrand and break points; Qf from dense_quad -- not the closed form."""
    from scipy.integrate import quad
    from scipy.optimize import minimize_scalar
    from scipy.stats import chi2, multivariate_normal, norm
    J = y.size
    F = 0 if x is None or model in ("null", "cross") else x.size
    a, b, lam, sg = row[:J], row[J:2 * J], row[2 * J:3 * J], row[3 * J:4 * J]
    rho = row[4 * J:5 * J] if model == "cross" else np.zeros(J)
    m_, s11, m0, m1, v = mu.law(model, row, J, F, x if F else None)
    v = max(v, 0.0)
    rt = model != "mlirt"
    mvn = multivariate_normal(np.zeros(J), np.diag(sg) + v * np.ones((J, J)), allow_singular=True) if rt else None

    @functools.lru_cache(maxsize=None)
    def logf(th):
        eta = a * (th - b)
        out = float(np.sum(y * eta - np.logaddexp(0.0, eta))) + norm.logpdf(th, m_, np.sqrt(s11))
        if rt:
            out += mvn.logpdf(t - (lam - (m0 + m1 * th) - rho * th))
        return out

    def lz(th):
        eta = a * (th - b)
        p = 1.0 / (1.0 + np.exp(-eta))
        l0 = np.sum(y * eta - np.logaddexp(0.0, eta))
        El0 = np.sum(p * eta - np.logaddexp(0.0, eta))
        var = np.sum(p * (1.0 - p) * eta * eta)
        return (l0 - El0) / np.sqrt(var) if var > 0.0 else 0.0

    qf = lambda th: dense_quad(sg, lam, t, rho, m0, m1, v, th)
    c = 2.0 / (9.0 * J)
    sd = np.sqrt(s11)
    grid = m_ + sd * np.linspace(-8, 8, 321)
    k = int(np.argmax([logf(float(th)) for th in grid]))
    opt = minimize_scalar(lambda th: -logf(float(th)), bracket=(grid[max(k - 1, 0)], grid[k], grid[min(k + 1, 320)]) if 0 < k < 320 else None, tol=1e-12)
    mode, top = float(opt.x), -opt.fun
    d = 1e-3 * sd
    psd = 1.0 / np.sqrt(max(-(logf(mode + d) - 2.0 * top + logf(mode - d)) / (d * d), 1.0 / s11))
    lo, hi = m_ - 12 * sd, m_ + 12 * sd
    pts = sorted({float(np.clip(mode + k * psd, lo, hi)) for k in (-10, -3, 0, 3, 10)})
    integ = lambda f: quad(lambda th: f(th) * np.exp(logf(float(th)) - top), lo, hi, points=pts, epsabs=0.0, epsrel=1e-12, limit=400)[0]
    n0 = integ(lambda th: 1.0)
    LZ, PY = integ(lz) / n0, integ(lambda th: norm.cdf(lz(th))) / n0
    if not rt:
        return LZ, PY, np.nan, np.nan, top + np.log(n0)
    LTZ = integ(lambda th: (np.cbrt(qf(th) / J) - (1.0 - c)) / np.sqrt(c)) / n0
    PT = integ(lambda th: chi2.sf(qf(th), J)) / n0
    return LZ, PY, LTZ, PT, top + np.log(n0)


def quad_fit(model, Y, logT, X, rows, weighting, obs=None):
    """A dict of COLS [N] from quad_row, the rows joined by their weighted means.  obs: every subject through its reduced data set (obs_util.reduced_subject)."""
    N = Y.shape[0]
    out = {c: np.full(N, np.nan) for c in COLS}
    for i in range(N):
        if obs is None:
            yi, ti, xi, ri = Y[i], None if logT is None else logT[i], None if X is None else X[i], rows
        else:
            red = ou.reduced_subject(model, Y, logT, X, rows, obs, i)
            if red is None:
                continue
            yi, ti, xi, ri = red[0][0], None if red[1] is None else red[1][0], None if red[2] is None else red[2][0], red[3]
        per = np.array([quad_row(model, yi.astype(np.float64), ti, xi, r) for r in ri])
        om = np.exp(per[:, 4] - per[:, 4].max()) if weighting == "likelihood" else np.ones(len(per))
        for k, c in enumerate(STATS):
            out[c][i] = np.sum(om * per[:, k]) / om.sum()
        out["rowEss"][i] = om.sum() ** 2 / np.sum(om * om)
    return out


def errors(got, ref, cols=STATS):
    """Per column the largest |got - ref| / max(|ref|, 1); NaN must stand against NaN."""
    get = lambda o, c: np.asarray(o[c] if isinstance(o, dict) else getattr(o, c), dtype=np.float64)
    return {c: ou.rel(get(got, c), get(ref, c)) for c in cols}


# ------------------------------------------------------------------------------------------------------------ simulated respondents
def simulate(model, N, J, seed, F=0):
    """Data simulated from the model at its generating parameters, which are returned as ONE item-trace row: (Y, logT, X, row [1, width], theta, zeta)."""
    L, g = mu.lib(), np.random.default_rng(seed)
    row = mu.make_rows(model, J, F, 1, seed=seed)[0]
    X = g.normal(0, 1, (N, F)) if F > 0 and model in ("mlirt", "rtirt", "latent") else None
    a, b, lam, sg = row[:J], row[J:2 * J], row[2 * J:3 * J], row[3 * J:4 * J]
    rho = row[4 * J:5 * J] if model == "cross" else np.zeros(J)
    theta, zeta = np.empty(N), np.zeros(N)
    for i in range(N):
        m_, s11, m0, m1, v = mu.law(model, row, J, 0 if X is None else F, None if X is None else X[i])
        theta[i] = m_ + np.sqrt(s11) * g.normal()
        zeta[i] = m0 + m1 * theta[i] + np.sqrt(max(v, 0.0)) * g.normal()
    eta = a[None, :] * (theta[:, None] - b[None, :])
    Y = (g.uniform(size=(N, J)) < 1.0 / (1.0 + np.exp(-eta))).astype(np.uint8)
    logT = None if model == "mlirt" else lam[None, :] - zeta[:, None] - rho[None, :] * theta[:, None] + np.sqrt(sg)[None, :] * g.normal(size=(N, J))
    return Y, logT, X, row[None, :].copy(), theta, zeta


def plant_guessers(Y, who, seed):
    """The respondents `who` answer by the toss of a coin."""
    Y = Y.copy()
    Y[who] = np.random.default_rng(seed).uniform(size=(len(who), Y.shape[1])) < 0.5
    return Y


def plant_time_shift(logT, row, who, sigmas=2.0):
    """The respondents `who` take sigmas standard deviations longer on the first half of the items."""
    J = logT.shape[1]
    logT = logT.copy()
    logT[np.ix_(who, np.arange(J // 2))] += sigmas * np.sqrt(row[0, 3 * J:3 * J + J // 2])[None, :]
    return logT


# The end-to-end case: GibbsRtIrt fitted to a complete 96 x 12 data set with two planted respondents (as aberrant_problem of tests/test_gpu_psis_loo.py plants one).
# The seed is chosen in tests/test_fit_host.py with the twin on the oracle's chain, which the fp64 engine follows to 1e-7.
E2E_N, E2E_J, E2E_SWEEPS, E2E_BURNIN, E2E_SEED, E2E_WHO_RESP, E2E_WHO_TIME, E2E_SHIFT = 96, 12, 200, 100, 74, 17, 58, 3.5


def aberrant_problem(seed=E2E_SEED):
    """(Y, logT, X, who_resp, who_time) of make_problem("rtirt", 96, 12): respondent who_resp has the six hardest items correct and the six easiest wrong, its
    times untouched; respondent who_time answers the six hardest items 3.5 log-seconds faster than the item's mean time and the six easiest 3.5 slower, its
    responses untouched (a common shift would be taken up by zeta)."""
    Y, logT, X, init, tp = pu.make_problem("rtirt", E2E_N, E2E_J, 3, seed=seed)
    Y, logT = Y.copy(), logT.copy()
    order = np.argsort(np.asarray(tp.b).ravel())
    easy, hard = order[:E2E_J // 2], order[E2E_J // 2:]
    Y[E2E_WHO_RESP, hard], Y[E2E_WHO_RESP, easy] = 1, 0
    cm = logT.mean(axis=0)
    logT[E2E_WHO_TIME, hard], logT[E2E_WHO_TIME, easy] = cm[hard] - E2E_SHIFT, cm[easy] + E2E_SHIFT
    return Y, logT, X, E2E_WHO_RESP, E2E_WHO_TIME


def oracle_rows(model, Y, logT, X, init, sweeps, burnin):
    """The post-burn-in item-trace rows [a b lambda sig2t | small part of qr] of the oracle's chain."""
    N = Y.shape[0]
    t = pu.OracleProblem(model, Y, logT, X, init, qRt=0.85, cov2one=model not in ("latentqr", "latent"), seed=1234).run(sweeps)
    return np.ascontiguousarray(np.hstack([t["ra"][:, N:], t["rt"][:, N:], t["qr"]])[burnin:])


# ------------------------------------------------------------------------------------------------------------ the cases of the kernel against the twin
# One table for tests/test_fit_host.py (the preconditions on the CPU with the twin alone: its conditioning against numpy.longdouble, and S at least S_MARGIN from
# 2 so that COARSE is decidable) and tests/test_gpu_person_fit.py (the kernel).  A case is (kind, model, ...):
#   ("shape", model, N, J, R, Q)     marginal_util's random rows and data, F = 3
#   ("a8", model)                    a_j = 8, one subject all correct, one all wrong (37 x 9, 3 rows)
#   ("far", model)                   logT of one subject 22 away from lambda, alternating in sign
#   ("v0", model)                    Sigma_p of correlation 1 (Latent: Sigma_p[2,2] = 0), Q = 127
#   ("masked", model, J)             obs_util.problem(model, 33, J, 3): n_i = 0, 1, J - 8, about J / 2 and J side by side in one wave
SHAPES = [(N, J, R, Q) for N in (1, 33) for J in (1, 9, 65) for R in (1, 3) for Q in (3, 61, 127)]
CASES = ([("shape", m, *s) for m in mu.MODELS for s in SHAPES] + [("a8", m) for m in mu.MODELS] + [("far", m) for m in mu.MODELS if m != "mlirt"] +
         [("v0", m) for m in mu.MODELS if m != "mlirt"] + [("masked", m, J) for m in mu.MODELS for J in (9, 65)])
# case -> data seed where DEFAULT_SEED leaves a twin S within S_MARGIN of 2 (tests/test_fit_host.py checks every case): the first seed from 12 on with a margin of 0.15
SEEDS = {("a8", "mlirt"): 108, ("a8", "null"): 17, ("a8", "cross"): 15, ("a8", "latent"): 13}
DEFAULT_SEED = 11


def case_id(case):
    return "-".join(str(v) for v in case)


@functools.lru_cache(maxsize=None)
def problem(case):
    """(model, Y, logT, X as the kernels see it, rows, Q, obs) of a case; computed once per process and never written to."""
    kind, model = case[0], case[1]
    seed = SEEDS.get(case, DEFAULT_SEED)
    obs, Q = None, 61
    if kind == "shape":
        N, J, R, Q = case[2:]
        rows = mu.make_rows(model, J, 3, R, seed=seed)
        Y, logT, X = mu.make_data(model, N, J, 3, seed=seed)
    elif kind == "a8":
        rows = mu.make_rows(model, 9, 3, 3, seed=seed, a=8.0)
        Y, logT, X = mu.make_data(model, 37, 9, 3, seed=seed)
        Y[5, :], Y[6, :] = 1, 0
    elif kind == "far":
        rows = mu.make_rows(model, 9, 3, 3, seed=seed)
        Y, logT, X = mu.make_data(model, 37, 9, 3, seed=seed)
        logT[3, :] += 22.0 * (-1.0) ** np.arange(9)
    elif kind == "v0":
        rows = mu.make_rows(model, 9, 3, 3, seed=seed, sigp=[1.5, 0.0, 0.0, 0.0] if model == "latent" else [4.0, 2.0, 2.0, 1.0])
        Y, logT, X = mu.make_data(model, 37, 9, 3, seed=seed)
        Q = 127           # (sd = 2 doubles the spacing of the nodes in theta: at 61 nodes some S of 111 lies within S_MARGIN of 2 at every seed tried)
    elif kind == "masked":
        Y, logT, X, rows, obs = ou.problem(model, 33, case[2], 3, seed=seed)
    else:
        raise ValueError(kind)
    out = (model, Y, logT, ou.kernel_x(model, X), rows, Q, obs)
    for a_ in out[1:]:
        if isinstance(a_, np.ndarray):
            a_.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def twin(case, weighting, longdouble=False):
    """(personFitHost's result, S (R, N)) of a case."""
    model, Y, logT, X, rows, Q, obs = problem(case)
    return pkg().personFitHost(mu.CODE[model], Y, logT, X, rows, Q, weighting, obs=obs, dtype=np.longdouble if longdouble else np.float64, with_S=True)


# The conditioning of the float64 twin on CASES: the largest error of STATS and rowEss against the same twin in numpy.longdouble, relative to max(|ref|, 1), as
# tests/test_fit_host.py::test_twin_conditioning_on_the_gpu_cases measures it (and asserts that it is no larger than this).  The kernel must agree with the float64
# twin within max(1e-10, 10 x TWIN_COND).
TWIN_COND = 2e-13
KERNEL_TOL = max(1e-10, 10.0 * TWIN_COND)


# GibbsMlIrt against the posterior predictive check of the same run: the rank correlation of pResp with getPpc's subject ppp_mid of the response deviance, on
# waic_util.spread_problem (seed 5 on the device).  Its floor is measured on the CPU with the twins on the oracle's chain at five OTHER data seeds
# (tests/test_fit_host.py: 0.9738, 0.9746, 0.9689, 0.9715, 0.9768), less a margin for the device's own replicate stream.
PPC_SEEDS, PPC_MIN_MEASURED, PPC_MARGIN = (6, 7, 8, 9, 10), 0.9689, 0.03
PPC_FLOOR = PPC_MIN_MEASURED - PPC_MARGIN

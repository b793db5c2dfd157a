"""Helpers shared by the tests of the item fit (tests/test_ifit_host.py, tests/test_gpu_item_fit.py): an independent reference for one subject's
six cell means -- scipy.integrate.quad_vec over theta with fit_util.quad_row's integrand and break points, the leave-one-item-out residual from the dense
covariance by numpy.linalg.solve --, a second sample with planted item drift, the one table of cases at which the kernels are compared with the twin, and the
comparison of two results."""
import functools

import numpy as np

import fit_util as fu
import marginal_util as mu
import obs_util as ou
import parity_util as pu

COLS = ("infit", "outfit", "respZ", "rtMsq", "rtZ")
CELLS = ("e", "r2", "c", "z2", "d", "d2")
COARSE_S, S_MARGIN = fu.COARSE_S, fu.S_MARGIN


def pkg():
    return pu.ge.load_package()


def get(o, c):
    return np.asarray(o[c] if isinstance(o, dict) else getattr(o, c), dtype=np.float64)


def errors(got, ref, cols=COLS):
    """Per column the largest |got - ref| / max(|ref|, 1); NaN must stand against NaN."""
    return {c: ou.rel(get(got, c), get(ref, c)) for c in cols}


# ------------------------------------------------------------------------------------------------------------ one subject by quadrature
def quad_cells(model, y, t, x, row):
    """The six cell means (J, 6) of subject (y, t, x) at `row` under the posterior of theta, by scipy.integrate.quad_vec: fit_util.quad_row's integrand (the
    dense multivariate normal of the log-times) and break points; r = |y - p| and c = p (1 - p) from p itself, z^2 = r^2 / c, and d from the conditional law of
    one log-time given the others by numpy.linalg.solve on the dense covariance -- not the closed forms."""
    from scipy.integrate import quad_vec
    from scipy.optimize import minimize_scalar
    from scipy.stats import multivariate_normal, norm
    J = y.size
    F = 0 if x is None or model in ("null", "cross") else x.size
    a, b, lam, sg = row[:J], row[J:2 * J], row[2 * J:3 * J], row[3 * J:4 * J]
    rho = row[4 * J:5 * J] if model == "cross" else np.zeros(J)
    m_, s11, m0, m1, v = mu.law(model, row, J, F, x if F else None)
    v = max(v, 0.0)
    rt = model != "mlirt"
    cov = np.diag(sg) + v * np.ones((J, J)) if rt else None
    mvn = multivariate_normal(np.zeros(J), cov, allow_singular=True) if rt else None

    @functools.lru_cache(maxsize=None)
    def logf(th):
        eta = a * (th - b)
        out = float(np.sum(y * eta - np.logaddexp(0.0, eta))) + norm.logpdf(th, m_, np.sqrt(s11))
        if rt:
            out += mvn.logpdf(t - (lam - (m0 + m1 * th) - rho * th))
        return out

    def cells(th):
        p = 1.0 / (1.0 + np.exp(-a * (th - b)))
        r, c = np.abs(y - p), p * (1.0 - p)
        out = [(2.0 * y - 1.0) * r, r * r, c, r * r / c]
        if rt:
            mean = lam - (m0 + m1 * th) - rho * th                    # of the log-times given theta
            d = np.empty(J)
            for j in range(J):
                o = np.arange(J) != j
                if o.any():
                    k = np.linalg.solve(cov[np.ix_(o, o)], cov[o, j])
                    cm, cv = mean[j] + k @ (t[o] - mean[o]), cov[j, j] - k @ cov[o, j]
                else:
                    cm, cv = mean[j], cov[j, j]
                d[j] = (t[j] - cm) / np.sqrt(cv)                      # positive: slower than predicted
            out += [d, d * d]
        else:
            out += [np.zeros(J), np.zeros(J)]
        return np.array(out).T.ravel()                                # (J * 6,)

    sd = np.sqrt(s11)
    grid = m_ + sd * np.linspace(-8, 8, 321)
    k = int(np.argmax([logf(float(th)) for th in grid]))
    opt = minimize_scalar(lambda th: -logf(float(th)), bracket=(grid[max(k - 1, 0)], grid[k], grid[min(k + 1, 320)]) if 0 < k < 320 else None, tol=1e-12)
    mode, top = float(opt.x), -opt.fun
    dd = 1e-3 * sd
    psd = 1.0 / np.sqrt(max(-(logf(mode + dd) - 2.0 * top + logf(mode - dd)) / (dd * dd), 1.0 / s11))
    lo, hi = m_ - 12 * sd, m_ + 12 * sd
    pts = sorted({float(np.clip(mode + k * psd, lo, hi)) for k in (-10, -3, 0, 3, 10)})
    f = lambda th: np.concatenate([[1.0], cells(float(th))]) * np.exp(logf(float(th)) - top)
    val = quad_vec(f, lo, hi, points=pts, epsabs=0.0, epsrel=1e-11, limit=400)[0]
    return (val[1:] / val[0]).reshape(J, 6)


# ------------------------------------------------------------------------------------------------------------ a second sample with planted drift
def drifted_sample(model, N, J, seed, row, item_b=None, item_lam=None):
    """(Y, logT) of N new respondents drawn at `row` [1, width] (fit_util.simulate's recipe, F = 0) with b of item_b raised by one logit and lambda of item_lam
    by half of that item's sigma in the GENERATING parameters only: the sample is then checked against the unchanged row."""
    g = np.random.default_rng(seed)
    true = row[0].copy()
    if item_b is not None:
        true[J + item_b] += 1.0
    if item_lam is not None:
        true[2 * J + item_lam] += 0.5 * np.sqrt(true[3 * J + item_lam])
    a, b, lam, sg = true[:J], true[J:2 * J], true[2 * J:3 * J], true[3 * J:4 * J]
    rho = true[4 * J:5 * J] if model == "cross" else np.zeros(J)
    m_, s11, m0, m1, v = mu.law(model, true, J, 0, None)
    theta = m_ + np.sqrt(s11) * g.normal(size=N)
    zeta = m0 + m1 * theta + np.sqrt(max(v, 0.0)) * g.normal(size=N)
    eta = a[None, :] * (theta[:, None] - b[None, :])
    Y = (g.uniform(size=(N, J)) < 1.0 / (1.0 + np.exp(-eta))).astype(np.uint8)
    logT = lam[None, :] - zeta[:, None] - rho[None, :] * theta[:, None] + np.sqrt(sg)[None, :] * g.normal(size=(N, J))
    return Y, logT


# ------------------------------------------------------------------------------------------------------------ the cases of the kernels against the twin
# One table for tests/test_ifit_host.py (the preconditions on the CPU with the twin alone) and tests/test_gpu_item_fit.py (the kernels).  fit_util.CASES' kinds
# without the weightings, the shapes with N = 257 as well (it crosses a reduction block of 256 subjects), and two kinds of their own:
#   ("nobody", model)                the masked wave at J = 9 with item 4 observed by nobody (n_j = 0 -> NaN)
#   ("wide", model)                  896 items x 33 subjects x 1 row, Q = 61
SHAPES = [(N, J, R, Q) for N in (1, 33, 257) for J in (1, 9, 65) for R in (1, 3) for Q in (3, 61, 127)]
CASES = ([("shape", m, *s) for m in mu.MODELS for s in SHAPES] + [c for c in fu.CASES if c[0] != "shape"] + [("nobody", m) for m in mu.MODELS] + [("wide", "rtirt")])
# case -> data seed where the default leaves a twin S within S_MARGIN of 2 (tests/test_ifit_host.py checks every case); fit_util's own moves hold for its kinds
SEEDS = {}
DEFAULT_SEED = fu.DEFAULT_SEED


def case_id(case):
    return "-".join(str(v) for v in case)


@functools.lru_cache(maxsize=None)
def problem(case):
    """(model, Y, logT, X as the kernels see it, rows, Q, obs) of a case; computed once per process and never written to."""
    kind, model = case[0], case[1]
    seed = SEEDS.get(case, DEFAULT_SEED)
    if kind == "shape" and case[2] == 257:
        N, J, R, Q = case[2:]
        rows = mu.make_rows(model, J, 3, R, seed=seed)
        Y, logT, X = mu.make_data(model, N, J, 3, seed=seed)
        out = (model, Y, logT, ou.kernel_x(model, X), rows, Q, None)
    elif kind == "nobody":
        Y, logT, X, rows, obs = ou.problem(model, 33, 9, 3, seed=seed)
        obs = obs.copy()
        obs[:, 4] = 0
        out = (model, Y, logT, ou.kernel_x(model, X), rows, 61, obs)
    elif kind == "wide":
        rows = mu.make_rows(model, 896, 3, 1, seed=seed)
        Y, logT, X = mu.make_data(model, 33, 896, 3, seed=seed)
        out = (model, Y, logT, ou.kernel_x(model, X), rows, 61, None)
    else:
        return fu.problem(case)
    for a_ in out[1:]:
        if isinstance(a_, np.ndarray):
            a_.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def twin(case, longdouble=False):
    """(itemFitHost's result, the cells (N, J, 6), S (R, N)) of a case."""
    model, Y, logT, X, rows, Q, obs = problem(case)
    return pkg().itemFitHost(mu.CODE[model], Y, logT, X, rows, Q, obs=obs, dtype=np.longdouble if longdouble else np.float64, with_cells=True, with_S=True)


# The conditioning of the float64 twin on CASES: the largest error of COLS against the same twin in numpy.longdouble, relative to max(|ref|, 1), as
# tests/test_ifit_host.py::test_twin_conditioning_on_the_gpu_cases measures it (and asserts that it is no larger than this).  The kernels must agree with the
# float64 twin within max(1e-10, 10 x TWIN_COND).
TWIN_COND = 1e-13           # measured 4.9e-14 (the "far" case of latent)
KERNEL_TOL = max(1e-10, 10.0 * TWIN_COND)


# The end-to-end case: GibbsRtIrt calibrated on a clean pu.make_problem("rtirt", 400, 12, 3) sample with 200 sweeps; a second sample of 400 from the same true
# parameters with b of E2E_ITEM_B raised by 1 and lambda of E2E_ITEM_LAM by half a sigma, checked against the calibration's post-burn-in rows.  The seed is chosen
# in tests/test_ifit_host.py with the twin on the oracle's chain.
E2E_N, E2E_J, E2E_SWEEPS, E2E_BURNIN, E2E_SEED, E2E_ITEM_B, E2E_ITEM_LAM = 400, 12, 200, 100, 76, 3, 8
# Measured there at seed 76: RESP_Z -9.07 on the planted item against 2.82 for the largest other |RESP_Z| (factor 3.22), RT_Z +9.24 against 3.43 (factor 2.70);
# seeds 74 and 75 give 1.50 / 3.37 and 1.90 / 3.15.  The device must keep the factors less E2E_MARGIN, and its columns must stand within E2E_GAP_BOUND of the
# twin's on the oracle's chain (the fp64 engine follows the oracle to 1e-7).
E2E_RESP_FACTOR, E2E_RT_FACTOR, E2E_MARGIN, E2E_GAP_BOUND = 3.22, 2.70, 0.5, 1e-6


@functools.lru_cache(maxsize=None)
def e2e_oracle_rows():
    (Y, logT, X, init), _ = e2e_problem()
    return fu.oracle_rows("rtirt", Y, logT, X, init, E2E_SWEEPS, E2E_BURNIN)


def e2e_problem(seed=E2E_SEED):
    """(calibration (Y, logT, X, init), second sample (Y, logT, X)): the clean make_problem sample, and E2E_N new respondents drawn by setDataRtIrt from the
    calibration problem's true parameters with the two planted shifts."""
    import copy
    P = pkg()
    Y, logT, X, init, tp = pu.make_problem("rtirt", E2E_N, E2E_J, 3, seed=seed)
    tp2 = copy.deepcopy(tp)
    tp2.b = np.array(tp.b, dtype=np.float64).copy()
    tp2.lam = np.array(tp.lam, dtype=np.float64).copy()
    tp2.b[E2E_ITEM_B] += 1.0
    tp2.lam[E2E_ITEM_LAM] += 0.5 * np.sqrt(np.asarray(tp.sig2t)[E2E_ITEM_LAM])
    D = P.setDataRtIrt(P.setCond(nSubj=E2E_N, nItem=E2E_J, nFeat=3, nIter=10, nChain=1, qRt=0.85), tp2, seed=np.random.default_rng(seed + 1000))
    return (Y, logT, X, init), (D.Y, D.logT, D.X)

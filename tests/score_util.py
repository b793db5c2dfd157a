"""Helpers shared by the tests of the scores (tests/test_score_host.py, tests/test_gpu_scores.py): an independent reference for one subject at one row --
scipy.integrate.quad over theta of marginal_util.quad_l's integrand, zeta given theta by numpy Gaussian conditioning on diag(sig2t) + v 1 1' -- the rows joined in
two passes, and the comparison of two score tables."""
import functools

import numpy as np

import marginal_util as mu
import parity_util as pu

COLS = ("theta", "thetaSd", "zeta", "zetaSd", "cov", "rowEss")
NEAR_ZERO = ("theta", "zeta", "cov")          # outputs that may be near 0: errors relative to max(|ref|, 1)


def quad_row(model, y, t, x, row):
    """(E, V, Ez, Vz, C, l) of subject (y, t, x) at `row`: the moments of theta under exp(logf) with quad_l's integrand and break points; zeta | theta, t at every
    theta by conditioning the joint Gaussian of (zeta, t) with numpy.linalg.solve -- not the closed form."""
    from scipy.integrate import quad
    from scipy.optimize import minimize_scalar
    from scipy.stats import multivariate_normal, norm
    J = y.size
    F = 0 if x is None or model in ("null", "cross") else x.size
    a, b, lam, sg = row[:J], row[J:2 * J], row[2 * J:3 * J], row[3 * J:4 * J]
    rho = row[4 * J:5 * J] if model == "cross" else np.zeros(J)
    m_, s11, m0, m1, v = mu.law(model, row, J, F, x if F else None)
    rt = model != "mlirt"
    if rt:
        Sig = np.diag(sg) + v * np.ones((J, J))
        mvn = multivariate_normal(np.zeros(J), Sig)
        K = np.linalg.solve(Sig, np.column_stack([np.ones(J), t - lam, rho]))          # Sigma^-1 [1, t - lambda, rho]
        u = v - v * v * float(np.ones(J) @ K[:, 0])                                      # Var(zeta) - Cov(zeta, t) Sigma^-1 Cov(t, zeta), Cov(zeta, t) = -v 1'

    @functools.lru_cache(maxsize=None)
    def logf(th):
        eta = a * (th - b)
        out = float(np.sum(y * eta - np.logaddexp(0.0, eta))) + norm.logpdf(th, m_, np.sqrt(s11))
        if rt:
            out += mvn.logpdf(t - (lam - (m0 + m1 * th) - rho * th))
        return out

    def ez(th):      # E[zeta | theta, t] = m - v 1' Sigma^-1 (t - E t),  E t = lambda - m - rho theta
        m = m0 + m1 * th
        return m - v * float(np.ones(J) @ (K[:, 1] + m * K[:, 0] + th * K[:, 2]))

    sd = np.sqrt(s11)
    grid = m_ + sd * np.linspace(-8, 8, 321)
    k = int(np.argmax([logf(float(th)) for th in grid]))
    opt = minimize_scalar(lambda th: -logf(float(th)), bracket=(grid[max(k - 1, 0)], grid[k], grid[min(k + 1, 320)]) if 0 < k < 320 else None, tol=1e-12)
    mode, top = float(opt.x), -opt.fun
    d = 1e-3 * sd
    psd = 1.0 / np.sqrt(max(-(logf(mode + d) - 2.0 * top + logf(mode - d)) / (d * d), 1.0 / s11))
    lo, hi = m_ - 12 * sd, m_ + 12 * sd
    pts = sorted({float(np.clip(mode + k * psd, lo, hi)) for k in (-10, -3, 0, 3, 10)})
    integ = lambda f: quad(lambda th: f(th) * np.exp(logf(float(th)) - top), lo, hi, points=pts, epsabs=0.0, epsrel=1e-13, limit=400)[0]
    # moments about the mode, in units of the posterior's width: no cancellation in the variance
    n0 = integ(lambda th: 1.0)
    d1 = integ(lambda th: (th - mode) / psd) / n0
    d2 = integ(lambda th: ((th - mode) / psd) ** 2) / n0
    E, V, l = mode + psd * d1, psd * psd * (d2 - d1 * d1), top + np.log(n0)
    if not rt:
        return E, V, np.nan, np.nan, np.nan, l
    ezm = ez(mode)
    z1 = integ(lambda th: ez(th) - ezm) / n0
    z2 = integ(lambda th: (ez(th) - ezm) ** 2) / n0
    zc = integ(lambda th: (ez(th) - ezm) * (th - mode) / psd) / n0
    return E, V, ezm + z1, u + z2 - z1 * z1, psd * (zc - z1 * d1), l


def join_rows(per, weighting):
    """The rows of one subject, per = [(E, V, Ez, Vz, C, l), ...], joined by the law of total variance in two passes: a dict of COLS."""
    E, V, Ez, Vz, C, l = (np.array(c, dtype=np.float64) for c in zip(*per))
    om = np.exp(l - l.max()) if weighting == "likelihood" else np.ones_like(l)
    W = om.sum()
    mean = lambda a: float(np.sum(om * a) / W)
    th, ze = mean(E), mean(Ez)
    return dict(theta=th, thetaSd=np.sqrt(mean(V) + mean((E - th) ** 2)), zeta=ze, zetaSd=np.sqrt(mean(Vz) + mean((Ez - ze) ** 2)),
                cov=mean(C) + mean((E - th) * (Ez - ze)), rowEss=float(W * W / np.sum(om * om)))


def quad_scores(model, Y, logT, X, rows, weighting):
    """A dict of COLS [N] from quad_row and join_rows."""
    N = Y.shape[0]
    out = {c: np.empty(N) for c in COLS}
    for i in range(N):
        j = join_rows([quad_row(model, Y[i], None if logT is None else logT[i], None if X is None else X[i], r) for r in rows], weighting)
        for c in COLS:
            out[c][i] = j[c]
    return out


def errors(got, ref, rt=True):
    """Per column the largest error of `got` (an OutputScores or a dict) against `ref` (likewise): relative, for NEAR_ZERO columns relative to max(|ref|, 1).  The
    zeta columns of a model without zeta must be NaN on both sides and are left out."""
    get = lambda o, c: np.asarray(o[c] if isinstance(o, dict) else getattr(o, c), dtype=np.float64)
    err = {}
    for c in COLS:
        g, r = get(got, c), get(ref, c)
        if not rt and c in ("zeta", "zetaSd", "cov"):
            assert np.all(np.isnan(g)), c
            continue
        assert np.all(np.isfinite(g)), c
        err[c] = float(np.max(np.abs(g - r) / (np.maximum(np.abs(r), 1.0) if c in NEAR_ZERO else np.abs(r))))
    return err


def mlirt_rows(M):
    """Item-trace rows of a GibbsMlIrt sampler-shaped namespace (waic_util.as_sampler): a, b, lambda = 0, sig2t = 1 | beta, post-burn-in."""
    C, P = M.Cond, M.Post
    N, J = C.nSubj, C.nItem
    ra, qr = P.ra[C.nBurnin:, :, 0], P.qr[C.nBurnin:, :, 0]
    return np.hstack([ra[:, N:N + J], ra[:, N + J:N + 2 * J], np.zeros((ra.shape[0], J)), np.ones((ra.shape[0], J)), qr])


def chain_agreement(scores, draws):
    """The two conditions under which the scores and the chain estimate the same thing, from theta's post-burn-in draws [rows, N]:
    r = RMS_i (theta_score - Post.mean theta) / thetaSd, and the ratio of the median sample sd of the draws to the median thetaSd."""
    r = float(np.sqrt(np.mean(((scores.theta - draws.mean(axis=0)) / scores.thetaSd) ** 2)))
    ratio = float(np.median(draws.std(axis=0, ddof=1)) / np.median(scores.thetaSd))
    return r, ratio


def pkg():
    return pu.ge.load_package()

"""Helpers shared by the marginal-WAIC tests (tests/test_marginal_host.py, tests/test_gpu_marginal_waic.py): random item-trace rows and data for the five models the
entry serves, and an independent reference for one l_i^(s): scipy.integrate.quad over theta of exp(B + log N(theta) + multivariate_normal.logpdf(t, ...))."""
import numpy as np

import parity_util as pu

MODELS = ["mlirt", "rtirt", "null", "cross", "latent"]
CODE = {"mlirt": 0, "rtirt": 1, "null": 4, "cross": 5, "latent": 6}


def lib():
    return pu.ge.load_package()._lib


def make_rows(model, J, F, R, seed, *, sigp=None, a=None, rho_sd=0.15):
    """R random item-trace rows [a b lambda sig2t | small part of qr] of `model` over F covariate columns (Null and Cross see none)."""
    L, g = lib(), np.random.default_rng(seed)
    m = CODE[model]
    Fk = L.kernel_feat(m, F)
    w = L.item_trace_width(m, J, Fk)
    rows = np.empty((R, w))
    for r in range(R):
        head = [g.uniform(0.5, 2.0, J) if a is None else np.full(J, float(a)), g.normal(0, 1, J), 4.0 + 0.3 * g.normal(0, 1, J), g.uniform(0.1, 0.6, J)]
        nq = w - 4 * J - (4 if model != "mlirt" else 0)
        q = np.zeros(nq) if model == "null" else (rho_sd if model == "cross" else 0.4) * g.normal(0, 1, nq)
        tail = []
        if model != "mlirt":
            if sigp is not None:
                tail = [np.asarray(sigp, dtype=np.float64)]
            else:
                s1, s2, rho = g.uniform(0.7, 1.3), g.uniform(0.3, 0.7), g.uniform(-0.6, 0.6)
                tail = [np.array([s1 * s1, rho * s1 * s2, rho * s1 * s2, s2 * s2])]
        rows[r] = np.concatenate(head + [q] + tail)
    return rows


def make_data(model, N, J, F, seed):
    g = np.random.default_rng(seed + 1000)
    Y = (g.uniform(size=(N, J)) < 0.55).astype(np.uint8)
    logT = None if model == "mlirt" else 4.0 + g.normal(0, 0.7, (N, J))
    X = g.normal(0, 1, (N, F)) if F > 0 else None
    return Y, logT, X


def law(model, row, J, F, x):
    """(mu, s11, m0, m1, v) of include/ertirt.h's table, written out per model."""
    q = row[4 * J:]
    x1 = np.concatenate([[1.0], np.zeros(0) if x is None else x])
    if model == "mlirt":
        return float(x1 @ q[:F + 1]), 1.0, 0.0, 0.0, 0.0
    S = q[-4:]
    s11, s12, s22 = S[0], 0.5 * (S[1] + S[2]), S[3]
    if model == "rtirt":
        mu, m1 = float(x1 @ q[:F + 1]), s12 / s11
        return mu, s11, float(x1 @ q[F + 1:2 * F + 2]) - m1 * mu, m1, s22 - s12 * s12 / s11
    if model == "latent":
        return 0.0, s11, float(x1 @ q[:F + 1]), q[F + 1], s22
    return 0.0, s11, 0.0, s12 / s11, s22 - s12 * s12 / s11


def quad_l(model, y, t, x, row):
    """log of the integral over theta of p(y | theta) p(t | theta) p(theta) with scipy.integrate.quad; p(t | theta) from scipy.stats.multivariate_normal."""
    from scipy.integrate import quad
    from scipy.optimize import minimize_scalar
    from scipy.stats import multivariate_normal, norm
    J = y.size
    F = 0 if x is None or model in ("null", "cross") else x.size
    a, b, lam, sg = row[:J], row[J:2 * J], row[2 * J:3 * J], row[3 * J:4 * J]
    rho = row[4 * J:5 * J] if model == "cross" else np.zeros(J)
    mu, s11, m0, m1, v = law(model, row, J, F, x if F else None)
    mvn = None if model == "mlirt" else multivariate_normal(np.zeros(J), np.diag(sg) + v * np.ones((J, J)))

    def logf(th):
        eta = a * (th - b)
        out = float(np.sum(y * eta - np.logaddexp(0.0, eta))) + norm.logpdf(th, mu, np.sqrt(s11))
        if mvn is not None:
            out += mvn.logpdf(t - (lam - (m0 + m1 * th) - rho * th))
        return out

    sd = np.sqrt(s11)
    grid = mu + sd * np.linspace(-8, 8, 321)
    k = int(np.argmax([logf(th) for th in grid]))
    opt = minimize_scalar(lambda th: -logf(th), bracket=(grid[max(k - 1, 0)], grid[k], grid[min(k + 1, 320)]) if 0 < k < 320 else None, tol=1e-12)
    mode, top = opt.x, -opt.fun
    d = 1e-3 * sd
    psd = 1.0 / np.sqrt(max(-(logf(mode + d) - 2.0 * top + logf(mode - d)) / (d * d), 1.0 / s11))      # the posterior's width at its mode: break points for quad
    lo, hi = mu - 12 * sd, mu + 12 * sd
    pts = sorted({float(np.clip(mode + k * psd, lo, hi)) for k in (-10, -3, 0, 3, 10)})
    val, _ = quad(lambda th: np.exp(logf(th) - top), lo, hi, points=pts, epsabs=0.0, epsrel=1e-13, limit=400)
    return top + np.log(val)

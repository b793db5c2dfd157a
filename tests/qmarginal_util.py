"""Helpers shared by the tests of LatentQr's marginal WAIC (tests/test_qmarginal_host.py, tests/test_gpu_quantile_marginal.py): random item-trace rows and data,
the extreme cases, data drawn from the model, and independent references for one l_i^(s):
  dblquad_l   scipy.integrate.dblquad over (theta, zeta) of exp(B + log N(theta) + sum_j log N(t_j; lambda_j - zeta, sig2t_j) + log ALD(zeta; m, s, q)), split at the
              asymmetric Laplace density's kink zeta = m(theta);
  quad_l      quad over theta of exp(B + log N(theta) + T(theta)), T by quad over zeta with break points at m and at R0 / P;
  mp_l        the rule of include/ertirt.h itself in 60-digit mpmath (the measure of the float64 formula's rounding)."""
import numpy as np

import marginal_util as mu
import parity_util as pu

CODE = 3          # ERM_MODEL_LATENTQR


def lib():
    return pu.ge.load_package()._lib


def make_rows(J, F, R, seed, *, s=None, s11=None, beta0=None, a=None):
    """R random LatentQr item-trace rows (Latent's layout: a b lambda sig2t | beta0 beta_x[F] beta_theta | vec(Sigma_p)); s = Sigma_p[2,2], the scale of zeta's law."""
    rows = mu.make_rows("latent", J, F, R, seed, a=a)
    rows[:, -3:-1] = 0.0
    if s is not None:
        rows[:, -1] = s
    if s11 is not None:
        rows[:, -4] = s11
    if beta0 is not None:
        rows[:, 4 * J] = beta0
    return rows


def make_data(N, J, F, seed):
    return mu.make_data("latent", N, J, F, seed)


def extreme_cases():
    """m = +-30 (beta0 = +-30), s in {0.001, 50}, one subject's logT 22 off, alternating in sign over the items, J = 1: (name, Y, logT, rows, q)."""
    out = []
    for b0 in (30.0, -30.0):
        for s in (0.001, 50.0):
            rows = make_rows(1, 0, 3, seed=61, s=s, beta0=b0)
            Y, logT, _ = make_data(5, 1, 0, seed=61)
            logT[3, :] += 22.0 * (-1.0) ** np.arange(1)
            out.append((f"beta0={b0:g} s={s:g}", Y, logT, rows, 0.85))
    return out


def simulate(N, J, q, seed, *, s11=1.3, s=0.15, beta0=0.2, btheta=0.4):
    """One row of parameters and data drawn from LatentQr at the level q (F = 0): a ~ U(0.7, 1.6), b ~ N(0, 1), lambda ~ N(4, 0.3^2), sig2t ~ U(0.1, 0.4);
    theta ~ N(0, s11), zeta = m + s (k1 nu + sqrt(k2 nu) e) with nu ~ Exp(1), e ~ N(0, 1)."""
    g = np.random.default_rng(seed)
    a, b, lam, sg = g.uniform(0.7, 1.6, J), g.normal(0, 1, J), g.normal(4.0, 0.3, J), g.uniform(0.1, 0.4, J)
    k1, k2 = (1 - 2 * q) / (q * (1 - q)), 2 / (q * (1 - q))
    th = g.normal(0, np.sqrt(s11), N)
    nu = g.exponential(1.0, N)
    ze = beta0 + btheta * th + s * (k1 * nu + np.sqrt(k2 * nu) * g.normal(0, 1, N))
    Y = (g.uniform(size=(N, J)) < 1.0 / (1.0 + np.exp(-a[None, :] * (th[:, None] - b[None, :])))).astype(np.uint8)
    logT = lam[None, :] - ze[:, None] + np.sqrt(sg)[None, :] * g.normal(0, 1, (N, J))
    row = np.concatenate([a, b, lam, sg, [beta0, btheta], [s11, 0.0, 0.0, s]])
    return Y, logT, row[None, :]


def _parts(y, t, x, row):
    J = y.size
    F = 0 if x is None else x.size
    a, b, lam, sg, q = row[:J], row[J:2 * J], row[2 * J:3 * J], row[3 * J:4 * J], row[4 * J:]
    m0 = q[0] + (0.0 if x is None else float(x @ q[1:F + 1]))
    return a, b, lam, sg, m0, q[F + 1], q[-4], q[-1]


def _norm_logpdf_sum(t, mean, var):
    return float(-0.5 * np.sum(np.log(2 * np.pi * var)) - 0.5 * np.sum((t - mean) ** 2 / var))


def _ald_logpdf(z, m, s, q):
    u = (z - m) / s
    return np.log(q * (1 - q) / s) - u * (q - (u < 0))


def dblquad_l(y, t, x, row, q):
    """log of the double integral over theta and zeta, the zeta range split at the kink of zeta's law."""
    from scipy.integrate import dblquad
    a, b, lam, sg, m0, m1, s11, s = _parts(y, t, x, row)
    sd = np.sqrt(s11)
    g = 1.0 / sg
    P, c = np.sum(g), np.sum(g * (lam - t)) / np.sum(g)

    def logf(ze, th):
        eta = a * (th - b)
        return float(np.sum(y * eta - np.logaddexp(0.0, eta))) + _norm_logpdf_sum(th, 0.0, s11) + _norm_logpdf_sum(t, lam - ze, sg) + float(_ald_logpdf(ze, m0 + m1 * th, s, q))

    ths = sd * np.linspace(-8, 8, 161)
    top = max(logf(ze, th) for th in ths for ze in (m0 + m1 * th, c, c - q / s / P, c + (1 - q) / s / P))
    w = 12.0 / np.sqrt(P)
    kink = lambda th: m0 + m1 * th
    f = lambda ze, th: np.exp(logf(ze, th) - top)
    lo, _ = dblquad(f, -10 * sd, 10 * sd, lambda th: min(kink(th), c) - w - 40 * s, kink, epsabs=0.0, epsrel=1e-12)
    hi, _ = dblquad(f, -10 * sd, 10 * sd, kink, lambda th: max(kink(th), c) + w + 40 * s, epsabs=0.0, epsrel=1e-12)
    return top + np.log(lo + hi)


def quad_T(t, lam, sg, m, s, q):
    """log of the zeta integral by quad: break points at the kink m and at the Gaussian's centre R0 / P."""
    from scipy.integrate import quad
    g = 1.0 / sg
    P, c = np.sum(g), np.sum(g * (lam - t)) / np.sum(g)
    w = 1.0 / np.sqrt(P)
    logf = lambda ze: _norm_logpdf_sum(t, lam - ze, sg) + float(_ald_logpdf(ze, m, s, q))
    cU, cL = c - q / s / P, c + (1 - q) / s / P
    cand = [m, c, max(m, cU), min(m, cL)]
    top = max(logf(z) for z in cand)
    lo, hi = min(m, cU) - 12 * w, max(m, cL) + 12 * w
    pts = sorted({float(np.clip(p, lo, hi)) for p in (m, c, cU, cL, max(m, cU) + 3 * w, min(m, cL) - 3 * w)})
    val, _ = quad(lambda ze: np.exp(logf(ze) - top), lo, hi, points=pts, epsabs=0.0, epsrel=1e-13, limit=400)
    return top + np.log(val)


def quad_l(y, t, x, row, q):
    """log of the integral over theta of exp(B + log N(theta) + T(theta)), T = quad_T."""
    from scipy.integrate import quad
    from scipy.optimize import minimize_scalar
    a, b, lam, sg, m0, m1, s11, s = _parts(y, t, x, row)
    sd = np.sqrt(s11)

    def logf(th):
        eta = a * (th - b)
        return float(np.sum(y * eta - np.logaddexp(0.0, eta))) + _norm_logpdf_sum(th, 0.0, s11) + quad_T(t, lam, sg, m0 + m1 * th, s, q)

    grid = sd * np.linspace(-8, 8, 161)
    k = int(np.argmax([logf(th) for th in grid]))
    opt = minimize_scalar(lambda th: -logf(th), bracket=(grid[max(k - 1, 0)], grid[k], grid[min(k + 1, 160)]) if 0 < k < 160 else None, tol=1e-12)
    mode, top = opt.x, -opt.fun
    d = 1e-3 * sd
    psd = 1.0 / np.sqrt(max(-(logf(mode + d) - 2.0 * top + logf(mode - d)) / (d * d), 1.0 / s11))
    lo, hi = -12 * sd, 12 * sd
    pts = sorted({float(np.clip(mode + k * psd, lo, hi)) for k in (-10, -3, 0, 3, 10)})
    val, _ = quad(lambda th: np.exp(logf(th) - top), lo, hi, points=pts, epsabs=0.0, epsrel=1e-13, limit=400)
    return top + np.log(val)


def mp_l(y, t, x, row, q, Q):
    """l = log sum_q exp(e_q) of include/ertirt.h's rule, every operation in 60-digit mpmath (logPhi = log(ncdf))."""
    import mpmath as mp
    with mp.workdps(60):
        f = lambda v: mp.mpf(float(v))
        J = y.size
        a, b, lam, sg, m0, m1, s11, s = _parts(y, t, x, row)
        a, b, lam, sg, tt = ([f(v) for v in arr] for arr in (a, b, lam, sg, t))
        m0, m1, sd, s, q = f(m0), f(m1), mp.sqrt(f(s11)), f(s), f(q)
        g = [1 / v for v in sg]
        P = mp.fsum(g)
        R0 = mp.fsum(gj * (l - tj) for gj, l, tj in zip(g, lam, tt))
        D0 = mp.fsum(gj * (l - tj) ** 2 for gj, l, tj in zip(g, lam, tt))
        L = mp.fsum(mp.log(v) for v in sg)
        bU, bL, h = R0 - q / s, R0 + (1 - q) / s, mp.mpf(12) / (Q - 1)
        es = []
        for k in range(Q):
            z = -6 + k * h
            th = sd * z
            B = mp.fsum(int(yj) * aj * (th - bj) - mp.log(1 + mp.exp(aj * (th - bj))) for yj, aj, bj in zip(y, a, b))
            m = m0 + m1 * th
            up = bU * bU / (2 * P) + q * m / s + mp.log(mp.ncdf(-(m - bU / P) * mp.sqrt(P)))
            lo = bL * bL / (2 * P) - (1 - q) * m / s + mp.log(mp.ncdf((m - bL / P) * mp.sqrt(P)))
            T = -mp.mpf(J) / 2 * mp.log(2 * mp.pi) - L / 2 - D0 / 2 + mp.log(q * (1 - q) / s) + mp.log(2 * mp.pi / P) / 2 + mp.log(mp.exp(up) + mp.exp(lo))
            es.append(mp.log(h) - mp.log(2 * mp.pi) / 2 - z * z / 2 + B + T)
        top = max(es)
        return float(top + mp.log(mp.fsum(mp.exp(e - top) for e in es)))


def host_build_l(exe, y, t, x, row, q, Q):
    """One l from the header's host build (tests/qmarginal_check.cpp, mode L)."""
    import subprocess
    F = 0 if x is None else x.size
    args = [repr(float(v)) for v in np.concatenate([row, y.astype(np.float64), t, np.zeros(0) if x is None else x])]
    r = subprocess.run([exe, "L", repr(float(q)), str(Q), str(y.size), str(F), *args], capture_output=True, text=True, timeout=60, check=True)
    return float(r.stdout.split()[0].split("=")[1])

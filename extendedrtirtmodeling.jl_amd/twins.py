"""The numpy / scipy test twins: every function here recomputes on the host what a device entry of libertirt.so computes, from the definitions in
include/ertirt.h and DESIGN.md 7, and no product path calls any of them -- the tests pin the kernels against them, and they serve traces and tables that are no
longer resident on a device.  Imports go one way: this module reads gibbs.py, base.py and _lib.py; gibbs.py reads nothing from here.
"""
from __future__ import annotations

import numpy as np

from . import _lib
from .base import OutputItemFit, OutputLoo, OutputPersonFit, OutputPpc, OutputPv, OutputScores, OutputWaic
from .gibbs import MARGINAL_UNIT, _GibbsBase, _log1pexp, _marginal_check, _norm_logpdf, marginalRows


# ------------------------------------------------------------------------------------------------------------------
# WAIC: getWaic's twin, from MCMC.Data and the full Post traces
# ------------------------------------------------------------------------------------------------------------------
def _rt_cell_law(MCMC, it, l, th):
    """Mean and variance (N, J) of every cell's log response time at trace row (it, l) of the full Post traces, for pointwiseLogLikHost and getPpcHost."""
    C, P, m = MCMC.Cond, MCMC.Post, MCMC._model
    N, J, q = C.nSubj, C.nItem, C.qRt
    rt = P.rt[it, :, l]
    ze, lam, sg = rt[:N], rt[N:N + J], rt[N + J:N + 2 * J]
    mu = lam[None, :] - ze[:, None]
    var = np.broadcast_to(sg[None, :], (N, J))
    if m in (_lib.MODEL_CROSS, _lib.MODEL_CROSSQR):
        qr = P.qr[it, :, l]
        mu = mu - th[:, None] * qr[None, :J]
        if m == _lib.MODEL_CROSSQR:
            k1, k2 = (1 - 2 * q) / (q * (1 - q)), 2 / (q * (1 - q))
            nu = qr[J + 4:].reshape(N, J, order="F")
            mu = mu + k1 * nu
            var = sg[None, :] * (k2 * nu)
    return mu, var


def pointwiseLogLikHost(MCMC: _GibbsBase, unit) -> np.ndarray:
    """l_u^(s) for every post-burn-in row s (iteration >= nBurnin, every interleaved chain) and unit u, with numpy from MCMC.Data and the full Post traces:
    an (|S|, U) array; cells in column-major order of (nSubj, nItem)."""
    if unit not in ("subject", "cell"):
        raise ValueError("unit must be 'subject' or 'cell'")
    C, D, P, m = MCMC.Cond, MCMC.Data, MCMC.Post, MCMC._model
    N, J = C.nSubj, C.nItem
    if np.ndim(P.ra) != 3:
        raise ValueError("getWaicHost needs the full Post traces (trace='full' and fill=True)")
    Y = np.asarray(D.Y, dtype=np.float64)
    logT = None if m == _lib.MODEL_MLIRT else np.asarray(D.logT, dtype=np.float64)
    if m == _lib.MODEL_CROSSQR and P.qr.shape[1] != J + 4 + N * J:
        raise ValueError("getWaicHost needs the per-sweep nu trace of GibbsRtIrtCrossQr in Post.qr")
    rows = [(it, l) for it in range(C.nBurnin, C.nIter) for l in range(C.nChain)]
    out = np.empty((len(rows), N * J if unit == "cell" else N))
    for s, (it, l) in enumerate(rows):
        ra = P.ra[it, :, l]
        th, a, b = ra[:N], ra[N:N + J], ra[N + J:N + 2 * J]
        eta = a[None, :] * (th[:, None] - b[None, :])
        ll = Y * eta - _log1pexp(eta)
        if m != _lib.MODEL_MLIRT:
            mu, var = _rt_cell_law(MCMC, it, l, th)
            ll = ll + _norm_logpdf(logT, mu, np.sqrt(var))
        out[s] = ll.reshape(-1, order="F") if unit == "cell" else ll.sum(axis=1)
    return out


def getWaicHost(MCMC: _GibbsBase, unit) -> OutputWaic:
    """getWaic evaluated with numpy on the host (the test twin of the device path): scipy's logsumexp and np.var(ddof=1) over pointwiseLogLikHost's rows."""
    out = waicFromLogLik(pointwiseLogLikHost(MCMC, unit), unit)
    if unit == "cell":
        sh = (MCMC.Cond.nSubj, MCMC.Cond.nItem)
        out.lppd_u, out.p_u = out.lppd_u.reshape(sh, order="F"), out.p_u.reshape(sh, order="F")
    return out


def _gaussian_rt_term(r, e, th, lt, lam, sg, rho, s11, m0, m1, v):
    """The response-time term of the five models without quantile weights: zeta | theta ~ N(m0 + m1 theta, v) integrated against the Gaussian response times.
    Returns e with the term added and sums = (P, R0 (N,), R1) of include/ertirt.h's definition."""
    J, g = sg.size, 1.0 / sg
    d = lam[None, None, :] - lt[:, None, :] - rho[None, None, :] * th[:, :, None]
    P, R, D = np.sum(g), np.sum(g * d, axis=2), np.sum(g * d * d, axis=2)
    m = np.asarray(m0)[:, None] + m1 * th if np.ndim(m0) else m0 + m1 * th
    e = e - 0.5 * J * np.log(2 * np.pi) - 0.5 * np.sum(np.log(sg)) - 0.5 * np.log1p(v * P) - 0.5 * (D + (P * m * m - 2 * R * m - v * R * R) / (1 + v * P))
    return e, (P, np.sum(g[None, :] * (lam[None, :] - lt), axis=1), np.sum(g * rho))


def _obs_mask(obs, shape):
    """The observed mask as a boolean (N, J) array: 1 = administered, 0 = not; anything else is refused."""
    O = np.asarray(obs)
    if O.shape != tuple(shape):
        raise ValueError("obs does not match Y")
    if not np.all((O == 0) | (O == 1)):
        raise ValueError("obs must be 0/1")
    return O.astype(bool)


def _masked_gaussian_rt_term(O):
    """_gaussian_rt_term over the observed cells O (N, J) alone, include/ertirt.h's definition for incomplete patterns restated: every sum over the items is a sum
    over O_i -- P, L and the n_i of -(n_i / 2) log 2 pi become per-subject -- and lt holds 0 at the unobserved cells.  sums = (P (N,), R0 (N,), R1 (N,))."""
    Of = O.astype(np.float64)
    n = Of.sum(axis=1)

    def term(r, e, th, lt, lam, sg, rho, s11, m0, m1, v):
        g = Of * (1.0 / sg)[None, :]                                                  # (N, J): g_j at the observed cells, 0 elsewhere
        d = lam[None, None, :] - lt[:, None, :] - rho[None, None, :] * th[:, :, None]
        P, R, D = np.sum(g, axis=1)[:, None], np.sum(g[:, None, :] * d, axis=2), np.sum(g[:, None, :] * d * d, axis=2)
        L = np.sum(Of * np.log(sg)[None, :], axis=1)[:, None]
        m = np.asarray(m0)[:, None] + m1 * th if np.ndim(m0) else m0 + m1 * th
        e = e - 0.5 * n[:, None] * np.log(2 * np.pi) - 0.5 * L - 0.5 * np.log1p(v * P) - 0.5 * (D + (P * m * m - 2 * R * m - v * R * R) / (1 + v * P))
        return e, (P[:, 0], np.sum(g * (lam[None, :] - lt), axis=1), np.sum(g * rho[None, :], axis=1))
    return term


def _marginal_rows_host(model, Y, logT, X, rows, Q, rt_term=_gaussian_rt_term, obs=None):
    """The rule at every row for marginalLogLikHost, quantileMarginalLogLikHost, scoresHost and plausibleValuesHost: the row unpacked, the population law, the
    theta part of e, and the family's response-time term.  Yields (e (N, Q), z (Q,), law, sums) with law = (mu (N,), sd, m0, m1, v) and sums as rt_term returns
    them (None for GibbsMlIrt).  obs (N, J), 0/1: incomplete patterns -- the response part and the response-time term are sums over the observed cells alone (the
    Gaussian family only); Y and logT at the unobserved cells are not read."""
    t = _lib.MODEL_TRAITS[model]
    O = None if obs is None else _obs_mask(obs, np.shape(Y))
    if O is not None:
        if rt_term is not _gaussian_rt_term:
            raise ValueError("an observed mask is served for the five models without quantile weights only")
        Y = np.where(O, np.asarray(Y), 0)
        logT = np.where(O, np.asarray(logT, dtype=np.float64), 0.0) if t.rt else None
        rt_term = _masked_gaussian_rt_term(O)
    Y = np.asarray(Y, dtype=np.float64)
    N, J = Y.shape
    F = 0 if X is None or not t.sees_x else np.shape(X)[1]
    x1 = np.ones((N, 1)) if F == 0 else np.hstack([np.ones((N, 1)), np.asarray(X, dtype=np.float64)])
    lt = np.asarray(logT, dtype=np.float64) if t.rt else None
    rows = np.atleast_2d(np.asarray(rows, dtype=np.float64))
    if rows.shape[1] != _lib.item_trace_width(model, J, F):
        raise ValueError(f"rows must have {_lib.item_trace_width(model, J, F)} columns")
    h = 12.0 / (Q - 1)
    z = -6.0 + h * np.arange(Q)
    zero = np.zeros(N)
    for r, row in enumerate(rows):
        a, b, lam, sg, q = row[:J], row[J:2 * J], row[2 * J:3 * J], row[3 * J:4 * J], row[4 * J:]
        rho = q[:J] if t.rho else np.zeros(J)
        m0, m1, v = zero, 0.0, 0.0
        if model == _lib.MODEL_MLIRT:
            mu, s11 = x1 @ q[:F + 1], 1.0
        else:
            Sp = q[len(q) - 4:]
            s11, s12, s22 = Sp[0], 0.5 * (Sp[1] + Sp[2]), Sp[3]
            if model == _lib.MODEL_RTIRT:
                mu = x1 @ q[:F + 1]
                m1 = s12 / s11
                m0, v = x1 @ q[F + 1:2 * F + 2] - m1 * mu, s22 - s12 * s12 / s11
            elif model in (_lib.MODEL_LATENT, _lib.MODEL_LATENTQR):      # (LatentQr's rows have Latent's layout; its v is the scale of zeta's asymmetric Laplace law)
                mu, m0, m1, v = zero, x1 @ q[:F + 1], q[F + 1], s22
            else:
                mu, m0, m1, v = zero, zero, s12 / s11, s22 - s12 * s12 / s11
        th = mu[:, None] + np.sqrt(s11) * z[None, :]                                  # (N, Q)
        eta = a[None, None, :] * (th[:, :, None] - b[None, None, :])                  # (N, Q, J)
        cell = Y[:, None, :] * eta - _log1pexp(eta)
        e = np.log(h) - 0.5 * np.log(2 * np.pi) - 0.5 * z[None, :] ** 2 + (np.sum(cell, axis=2) if O is None else np.sum(np.where(O[:, None, :], cell, 0.0), axis=2))
        sums = None
        if t.rt:
            e, sums = rt_term(r, e, th, lt, lam, sg, rho, s11, m0, m1, v)
        yield e, z, (mu, np.sqrt(s11), m0, m1, v), sums


def _loglik_rows(rule, with_S):
    """l (R, N) of the rows _marginal_rows_host yields, l = logsumexp_q e_q; with_S: (l, S), S (R, N) = sum_q exp(e_q - max_q e_q)."""
    from scipy.special import logsumexp
    per = [(logsumexp(e, axis=1), np.sum(np.exp(e - np.max(e, axis=1, keepdims=True)), axis=1)) for e, _, _, _ in rule]
    out, outS = np.array([p[0] for p in per]), np.array([p[1] for p in per])
    return (out, outS) if with_S else out


def marginalLogLikHost(model, Y, logT, X, rows, nodes=_lib.MARGINAL_NODES, with_S=False, obs=None) -> np.ndarray:
    """l_i^(s) of the marginal WAIC with numpy (the test twin of marginal_kernel): an (R, N) array for the item-trace rows [R, item_trace_width] (as
    Engine.item_trace() returns them) and the data Y, logT [N, J], X [N, F] or None.  with_S=True also returns S = sum_q exp(e_q - max_q e_q) per (row, subject):
    S < 2 marks a posterior too narrow for the rule.  obs (N, J), 0/1: the observed mask of incomplete patterns (the twin of the MASKED instantiations)."""
    return _loglik_rows(_marginal_rows_host(model, Y, logT, X, rows, _lib.marginal_nodes(nodes), obs=obs), with_S)


def waicFromLogLik(L, unit=MARGINAL_UNIT, **extra) -> OutputWaic:
    """WAIC from an (|S|, U) array of pointwise log-likelihoods with scipy's logsumexp and np.var(ddof=1)."""
    from scipy.special import logsumexp
    L = np.asarray(L, dtype=np.float64)
    S, U = L.shape
    if S < 2:
        raise ValueError("WAIC needs at least two post-burn-in rows")
    lppd_u = logsumexp(L, axis=0) - np.log(S)
    p_u = np.var(L, axis=0, ddof=1)
    el = lppd_u - p_u
    elpd = float(np.sum(el))
    se = 2.0 * float(np.sqrt(U * np.var(el, ddof=1))) if U > 1 else 0.0
    return OutputWaic(elpd=elpd, pWaic=float(np.sum(p_u)), WAIC=-2.0 * elpd, se=se, nHighVar=int(np.sum(p_u > 0.4)), lppd=float(np.sum(lppd_u)), unit=unit, nUnits=U,
                      nRows=S, lppd_u=lppd_u, p_u=p_u, **extra)


_QMARG_SERIES_X = -36.0


def _qmarg_log_ndtr(x):
    """log Phi(x) in the three arms of csrc/erm_qmarginal.hpp (qmarg_log_ndtr), restated with scipy's erfc: x >= 0: log1p(-erfc(x / sqrt 2) / 2);
    -36 <= x < 0: log(erfc(-x / sqrt 2) / 2); x < -36: -x^2 / 2 - log(-x) - 1/2 log 2 pi + log1p(-r + 3 r^2 - ... + 2027025 r^8), r = 1 / x^2."""
    from scipy.special import erfc
    x = np.asarray(x, dtype=np.float64)
    out = np.empty_like(x)
    hi, lo = x >= 0.0, x < _QMARG_SERIES_X
    mid = ~hi & ~lo
    out[hi] = np.log1p(-0.5 * erfc(x[hi] * np.sqrt(0.5)))
    out[mid] = np.log(0.5 * erfc(-x[mid] * np.sqrt(0.5)))
    xl = x[lo]
    r = 1.0 / (xl * xl)
    p = np.full_like(r, 2027025.0)
    for c in (-135135.0, 10395.0, -945.0, 105.0, -15.0, 3.0, -1.0):
        p = c + r * p
    out[lo] = -0.5 * xl * xl - np.log(-xl) - 0.5 * np.log(2 * np.pi) + np.log1p(r * p)
    return out


def _quantile_rt_term(q):
    """The response-time term of GibbsRtIrtLatentQr at the quantile level q: zeta | theta asymmetric Laplace (m0 + m1 theta, s = Sigma_p[2,2], q) integrated against
    the Gaussian response times in closed form -- two normal-CDF terms.  No sums: the scores and the plausible values do not serve this family."""
    def term(r, e, th, lt, lam, sg, rho, s11, m0, m1, s):
        if not (s > 0.0 and s11 > 0.0 and np.all(sg > 0.0)):
            raise ValueError(f"row {r}: sig2t, Sigma_p[1,1] and Sigma_p[2,2] must be positive")
        J, g = sg.size, 1.0 / sg
        d0 = lam[None, :] - lt
        P, R0, D0, L = np.sum(g), np.sum(g * d0, axis=1)[:, None], np.sum(g * d0 * d0, axis=1)[:, None], np.sum(np.log(sg))
        m = m0[:, None] + m1 * th                                                     # (N, Q)
        bU, bL, rP = R0 - q / s, R0 + (1.0 - q) / s, np.sqrt(P)
        up = bU * bU / (2.0 * P) + q * m / s + _qmarg_log_ndtr(-(m - bU / P) * rP)
        lo = bL * bL / (2.0 * P) - (1.0 - q) * m / s + _qmarg_log_ndtr((m - bL / P) * rP)
        return e - 0.5 * J * np.log(2 * np.pi) - 0.5 * L - 0.5 * D0 + np.log(q * (1.0 - q) / s) + 0.5 * (np.log(2 * np.pi) - np.log(P)) + np.logaddexp(up, lo), None
    return term


def quantileMarginalLogLikHost(model, Y, logT, X, rows, qRt, nodes=_lib.MARGINAL_NODES, with_S=False) -> np.ndarray:
    """l_i^(s) of GibbsRtIrtLatentQr's marginal WAIC with numpy (the test twin of marginal_kernel<LATENTQR>): an (R, N) array for the item-trace rows
    [R, item_trace_width] (Latent's layout) and the data Y, logT [N, J], X [N, F] or None at the quantile level qRt.  include/ertirt.h's definition restated:
    theta by the rule of marginalLogLikHost, zeta | theta asymmetric Laplace (m0 + m1 theta, s = Sigma_p[2,2], qRt) integrated against the Gaussian response times
    in closed form.  with_S=True also returns S per (row, subject)."""
    if model not in _lib.QUANTILE_MARGINAL_MODELS:
        raise ValueError("quantileMarginalLogLikHost serves GibbsRtIrtLatentQr only")
    q = float(qRt)
    if not 0.0 < q < 1.0:
        raise ValueError("qRt must be inside (0, 1)")
    return _loglik_rows(_marginal_rows_host(model, Y, logT, X, rows, _lib.marginal_nodes(nodes), _quantile_rt_term(q)), with_S)


def psisTailLen(S) -> int:
    """M = min(ceil(S / 5), ceil(3 sqrt(S))), as the float formula gives it."""
    return int(min(np.ceil(S / 5.0), np.ceil(3.0 * np.sqrt(S))))


def psisLooHost(L, dtype=np.float64, with_lw=False, with_fit=False):
    """PSIS-LOO of an (|S|, U) table of pointwise log-likelihoods with numpy (the test twin of psis_kernel), written from the papers: Vehtari, Gelman and Gabry
    (2017) for the estimator, Vehtari, Simpson, Gelman, Yao and Gabry (2024, Algorithm 1 and Appendix) for the tail length, the smoothing and the k^ prior, Zhang
    and Stephens (2009) for the generalised-Pareto fit; r_eff = 1.  dtype=np.longdouble runs the same arithmetic in extended precision (the tests' measure of the
    computation's own conditioning).  Returns an OutputLoo with the pointwise vectors; with_lw: also the smoothed, normalised log-weights (|S|, U); with_fit: also
    sigma (U,) (NaN where the tail could not be fitted)."""
    from math import floor
    L = np.asarray(L, dtype=dtype)
    if L.ndim != 2:
        raise ValueError("L must be (rows, units)")
    S, U = L.shape
    _lib.psis_rows(S)
    fl = dtype
    M = psisTailLen(S)
    G = 30 + int(floor(np.sqrt(M)))

    def lse(v):
        m = np.max(v)
        return m + np.log(np.sum(np.exp(v - m)))

    elpd, p, khat, neff, sig = (np.empty(U, dtype=fl) for _ in range(5))
    LW = np.empty((S, U), dtype=fl)
    for u in range(U):
        l = L[:, u]
        lw = -l - np.max(-l)
        order = np.argsort(lw, kind="stable")                 # ascending by (lw, position)
        srt = lw[order]
        c = srt[S - M - 1]
        x = np.exp(srt[S - M:]) - np.exp(c)
        k, sigma = fl(np.inf), fl(np.nan)
        xstar = x[int(floor(M / 4 + 0.5)) - 1]
        if xstar > 0 and x[-1] - x[0] > 0:
            with np.errstate(all="ignore"):
                j = np.arange(1, G + 1).astype(fl)
                b = 1 / x[-1] + (1 - np.sqrt(G / (j - fl(0.5)))) / (3 * xstar)
                kj = np.mean(np.log1p(-b[:, None] * x[None, :]), axis=1)
                Lj = M * (np.log(-b / kj) - kj - 1)
                w = np.exp(Lj - lse(Lj))
                bh = np.sum(b * w)
                kr = np.mean(np.log1p(-bh * x))
                sg = -kr / bh
                kh = (M * kr + 5) / fl(M + 10)
            if np.isfinite(bh) and np.isfinite(sg) and np.isfinite(kh):
                k, sigma = kh, sg
        new = srt.copy()
        if np.isfinite(k):
            with np.errstate(all="ignore"):
                pr = (np.arange(1, M + 1).astype(fl) - fl(0.5)) / M
                q = -sigma * np.log1p(-pr) if k == 0 else sigma * np.expm1(-k * np.log1p(-pr)) / k
                new[S - M:] = np.minimum(fl(0), np.log(np.exp(c) + q))
        lwp = np.empty(S, dtype=fl)
        lwp[order] = new
        norm = lse(lwp)
        elpd[u] = lse(lwp + l) - norm
        p[u] = (lse(l) - np.log(fl(S))) - elpd[u]
        khat[u], sig[u] = k, sigma
        wn = np.exp(lwp - norm)
        neff[u] = 1 / np.sum(wn * wn)
        LW[:, u] = lwp - norm
    thr = min(1.0 - 1.0 / np.log10(S), 0.7)
    el = elpd.astype(np.float64)
    se = 2.0 * float(np.sqrt(U * np.var(el, ddof=1))) if U > 1 else 0.0
    out = OutputLoo(elpd=float(np.sum(elpd)), pLoo=float(np.sum(p)), LOOIC=-2.0 * float(np.sum(elpd)), se=se, lppd=float(np.sum(elpd + p)), unit=None, nUnits=U, nRows=S,
                    nBadK=int(np.sum(khat > 0.7)), nHighK=int(np.sum(khat > thr)), tailLen=M, elpd_u=elpd, p_u=p, khat=khat, nEff=neff, nNodes=0, nCoarse=0)
    extra = ([LW] if with_lw else []) + ([sig] if with_fit else [])
    return (out, *extra) if extra else out


# ------------------------------------------------------------------------------------------------------------------
# The marginal getters' twins, both families: a family's log-likelihood twin; its scalars come from the sampler's conditions
# ------------------------------------------------------------------------------------------------------------------
_LOGLIK_TWINS = {"gaussian": marginalLogLikHost, "quantile": quantileMarginalLogLikHost}


def _marginal_loglik_host(MCMC, family, nodes, rows, who):
    """What the four get...MarginalHost functions start from: the family's twin's l [S, N], the node count, the subjects with a grid too coarse at any row."""
    Q = _marginal_check(MCMC, nodes, who, family)
    D, t = MCMC.Data, MCMC._traits
    if D is None:
        raise ValueError("Data is required")
    rows = marginalRows(MCMC) if rows is None else rows
    X = np.asarray(D.X, dtype=np.float64) if t.sees_x and MCMC.Cond.nFeat > 0 else None
    scalars = [{"q_rt": MCMC.Cond.qRt}[s] for s in _lib.MARGINAL_FAMILIES[family].scalars]
    L, S = _LOGLIK_TWINS[family](MCMC._model, D.Y, D.logT if t.rt else None, X, rows, *scalars, Q, with_S=True)
    return L, Q, int(np.sum(np.any(S < 2.0, axis=0)))


def _loo_marginal_host(MCMC, family, nodes, rows, who) -> OutputLoo:
    L, Q, n_coarse = _marginal_loglik_host(MCMC, family, nodes, rows, who)
    out = psisLooHost(L)
    out.unit, out.nNodes, out.nCoarse = MARGINAL_UNIT, Q, n_coarse
    return out


def getWaicMarginalHost(MCMC: _GibbsBase, nodes=_lib.MARGINAL_NODES, rows=None) -> OutputWaic:
    """getWaicMarginal evaluated with numpy / scipy on the host (the test twin of the device path) from MCMC.Data and the item-level trace rows (marginalRows, or
    `rows`)."""
    L, Q, n_coarse = _marginal_loglik_host(MCMC, "gaussian", nodes, rows, "getWaicMarginal")
    return waicFromLogLik(L, nNodes=Q, nCoarse=n_coarse)


def getLooMarginalHost(MCMC: _GibbsBase, nodes=_lib.MARGINAL_NODES, rows=None) -> OutputLoo:
    """getLooMarginal evaluated with numpy on the host (the test twin of the device path): marginalLogLikHost on MCMC.Data and the item-level trace rows
    (marginalRows, or `rows`), then psisLooHost."""
    return _loo_marginal_host(MCMC, "gaussian", nodes, rows, "getLooMarginal")


def getWaicMarginalQrHost(MCMC: _GibbsBase, nodes=_lib.MARGINAL_NODES, rows=None) -> OutputWaic:
    """getWaicMarginalQr evaluated with numpy / scipy on the host (the test twin of the device path)."""
    L, Q, n_coarse = _marginal_loglik_host(MCMC, "quantile", nodes, rows, "getWaicMarginalQr")
    return waicFromLogLik(L, nNodes=Q, nCoarse=n_coarse)


def getLooMarginalQrHost(MCMC: _GibbsBase, nodes=_lib.MARGINAL_NODES, rows=None) -> OutputLoo:
    """getLooMarginalQr evaluated with numpy on the host: quantileMarginalLogLikHost, then psisLooHost."""
    return _loo_marginal_host(MCMC, "quantile", nodes, rows, "getLooMarginalQr")


# ------------------------------------------------------------------------------------------------------------------
# Scores and plausible values: scoreRespondents' and drawPlausibleValues' twins on _marginal_rows_host
# ------------------------------------------------------------------------------------------------------------------
def _row_moments(e, z, law, sums, rt):
    """A row of _marginal_rows_host for scoresHost and plausibleValuesHost: theta's mean and variance E, V (N,) on the rule, zeta | theta ~ N(c0 + c1 theta, u)
    (zeros without response times), the largest e_q, M (N, 1), and the sum s (N,) of exp(e_q - M)."""
    mu, sd, m0, m1, v = law
    M = np.max(e, axis=1, keepdims=True)
    p = np.exp(e - M)
    s = np.sum(p, axis=1)
    w = p / s[:, None]
    Z1, Z2 = w @ z, w @ (z * z)
    E, V = mu + sd * Z1, np.maximum(sd * sd * (Z2 - Z1 * Z1), 0.0)
    c0, c1, u = 0.0, 0.0, 0.0
    if rt:
        P, R0, R1 = sums
        c0, c1, u = (m0 + v * R0) / (1 + v * P), (m1 - v * R1) / (1 + v * P), v / (1 + v * P)
    return E, V, c0, c1, u, M, s


def scoresHost(model, Y, logT, X, rows, nodes=_lib.MARGINAL_NODES, weighting="equal", obs=None) -> OutputScores:
    """scoreRespondents with numpy (the test twin of score_kernel), written beside marginalLogLikHost: the rule's weights at every row, the moments of theta, the
    zeta conditional, and the rows joined in two passes (the means, then the deviations from them).  obs (N, J), 0/1: the observed mask of incomplete patterns; the
    result then carries nObs (N,)."""
    if model not in _lib.MARGINAL_MODELS:
        raise ValueError("scoresHost serves the five models without quantile weights")
    Q, wt = _lib.marginal_nodes(nodes), _lib.score_weighting(weighting)
    rt = _lib.MODEL_TRAITS[model].rt
    E, V, Ez, Vz, Cz, l, S = ([] for _ in range(7))
    for e, z, law, sums in _marginal_rows_host(model, Y, logT, X, rows, Q, obs=obs):
        Es, Vs, c0, c1, u, M, s = _row_moments(e, z, law, sums, rt)
        for lst, val in zip((E, V, Ez, Vz, Cz, l, S), (Es, Vs, c0 + c1 * Es, u + c1 * c1 * Vs, c1 * Vs, M[:, 0] + np.log(s), s)):
            lst.append(val)
    E, V, Ez, Vz, Cz, l, S = (np.array(a) for a in (E, V, Ez, Vz, Cz, l, S))             # (R, N)
    om = np.exp(l - np.max(l, axis=0, keepdims=True)) if wt == _lib.SCORE_LIKELIHOOD else np.ones_like(l)
    W = np.sum(om, axis=0)
    mean = lambda a: np.sum(om * a, axis=0) / W
    th, ze = mean(E), mean(Ez)
    nan = np.full(E.shape[1], np.nan)
    coarse = np.any(S < 2.0, axis=0)
    out = OutputScores(theta=th, thetaSd=np.sqrt(np.maximum(mean(V) + mean((E - th) ** 2), 0.0)), zeta=ze if rt else nan,
                       zetaSd=np.sqrt(np.maximum(mean(Vz) + mean((Ez - ze) ** 2), 0.0)) if rt else nan, cov=mean(Cz) + mean((E - th) * (Ez - ze)) if rt else nan,
                       rowEss=W * W / np.sum(om * om, axis=0), coarse=coarse, nRows=E.shape[0], nNodes=Q, nCoarse=int(np.sum(coarse)),
                       weighting="likelihood" if wt else "equal")
    if obs is not None:
        out.nObs = _obs_mask(obs, np.shape(Y)).sum(axis=1).astype(np.int32)
    return out


# ------------------------------------------------------------------------------------------------------------------
# Person fit: personFit's twin beside scoresHost, on _marginal_rows_host's law
# ------------------------------------------------------------------------------------------------------------------
def chi2TailHost(Qf, n, dtype=np.float64):
    """P(chi^2_n >= Qf) by the finite sum of csrc/erm_fit.hpp (fit_chi2_tail), for integer n broadcast against Qf: y = Qf / 2, o = n mod 2, m = n // 2,
    base = o ? erfc(sqrt y) : 0, t_0 = e^-y (o ? 2 sqrt(y / pi) : 1), t_k = t_(k-1) y / (k + o / 2), tail = base + sum_(k < m) t_k; 0 for y > 700."""
    from scipy.special import erfc
    Qf = np.asarray(Qf, dtype=dtype)
    n = np.broadcast_to(np.asarray(n, dtype=np.int64), Qf.shape)
    o, m = (n % 2) == 1, n // 2
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        y = Qf / 2
        rt = np.sqrt(y)
        tail = np.where(o, erfc(rt.astype(np.float64)).astype(dtype), dtype(0))
        t = np.exp(-y) * np.where(o, 2 * rt / np.sqrt(np.arccos(dtype(-1))), dtype(1))
        for k in range(int(m.max()) if m.size else 0):
            tail = np.where(k < m, tail + t, tail)
            t = t * (y / (k + 1 + np.where(o, dtype(0.5), dtype(0))))
        return np.where(y > 700, dtype(0), tail)


def wilsonHilfertyHost(Qf, n, dtype=np.float64):
    """Wilson-Hilferty's z of a chi^2_n value (fit_wh): ((Qf / n)^(1/3) - (1 - 2 / (9 n))) / sqrt(2 / (9 n)); NaN for n = 0."""
    Qf, n = np.asarray(Qf, dtype=dtype), np.asarray(n, dtype=dtype)
    with np.errstate(divide="ignore", invalid="ignore"):
        c = 2 / (9 * n)
        return (np.cbrt(Qf / n) - (1 - c)) / np.sqrt(c)


def personFitHost(model, Y, logT, X, rows, nodes=_lib.MARGINAL_NODES, weighting="equal", obs=None, dtype=np.float64, with_S=False) -> OutputPersonFit:
    """personFit with numpy (the test twin of fit_kernel), written beside scoresHost: the population law of every row from _marginal_rows_host; then the definition
    of include/ertirt.h restated -- at every node lz from (W, Vw) in the form without cancellation, the quadratic form Qf of the log-times with its chi^2 tail
    (chi2TailHost) and its Wilson-Hilferty z, e_q from the same sums; the four means under the rule's weights at the row; the weighted means over the rows.
    obs (N, J), 0/1: the observed mask -- every sum over the items is a sum over the observed cells and n_i stands for J (restated here: the masked call never
    reduces the data and calls itself); the result then carries nObs (N,).  dtype=np.longdouble: the same arithmetic in extended precision, for the conditioning
    of the float64 result (erfc stays float64).  with_S: also S (R, N), the rule's sum at every row."""
    from scipy.special import erfc
    if model not in _lib.MARGINAL_MODELS:
        raise ValueError("personFitHost serves the five models without quantile weights")
    Q, wt = _lib.marginal_nodes(nodes), _lib.score_weighting(weighting)
    t = _lib.MODEL_TRAITS[model]
    f = dtype
    O = np.ones(np.shape(Y), dtype=bool) if obs is None else _obs_mask(obs, np.shape(Y))
    Of = O.astype(f)
    Yz = np.where(O, np.asarray(Y), 0)
    ltz_in = np.where(O, np.asarray(logT, dtype=np.float64), 0.0) if t.rt else None
    Yf = Yz.astype(f)
    N, J = Yf.shape
    n = O.sum(axis=1)
    lt = ltz_in.astype(f) if t.rt else None
    rows2 = np.atleast_2d(np.asarray(rows, dtype=np.float64))
    log2pi = np.log(2 * np.arccos(f(-1)))
    LZ, PY, LTZ, PT, l, S = ([] for _ in range(6))
    for (_, z, law, _), row in zip(_marginal_rows_host(model, Yz, ltz_in, X, rows2, Q), rows2):
        mu, sd, m0, m1, v = law
        a, b, lam, sg = (row[k * J:(k + 1) * J].astype(f) for k in range(4))
        rho = row[4 * J:5 * J].astype(f) if t.rho else np.zeros(J, dtype=f)
        z = z.astype(f)
        h = f(12) / (Q - 1)
        th = np.asarray(mu, dtype=f)[:, None] + f(sd) * z[None, :]                           # (N, Q)
        eta = a[None, None, :] * (th[:, :, None] - b[None, None, :])                          # (N, Q, J)
        tt = np.exp(-np.abs(eta))
        lse = np.maximum(eta, 0) + np.log1p(tt)
        r = np.where((Yz[:, None, :] == 1) == (eta >= 0), tt / (1 + tt), 1 / (1 + tt))
        Oq = Of[:, None, :]
        W = np.sum(Oq * (2 * Yf[:, None, :] - 1) * r * eta, axis=2)
        Vw = np.sum(Oq * eta * eta * tt / ((1 + tt) * (1 + tt)), axis=2)
        with np.errstate(divide="ignore", invalid="ignore"):
            lz = np.where(Vw > 0, W / np.sqrt(Vw), f(0))
        e = np.log(h) - log2pi / 2 - z[None, :] ** 2 / 2 + np.sum(Oq * (Yf[:, None, :] * eta - lse), axis=2)
        ltz = tail = np.full((N, Q), np.nan, dtype=f)
        if t.rt:
            vv = f(max(v, 0.0))
            g = Of / sg[None, :]                                                              # (N, J): g_j at the observed cells, 0 elsewhere
            d = lam[None, None, :] - lt[:, None, :] - rho[None, None, :] * th[:, :, None]
            P, R, D = np.sum(g, axis=1)[:, None], np.sum(g[:, None, :] * d, axis=2), np.sum(g[:, None, :] * d * d, axis=2)
            L = np.sum(Of * np.log(sg)[None, :], axis=1)[:, None]
            m = (np.asarray(m0, dtype=f)[:, None] if np.ndim(m0) else f(m0)) + f(m1) * th
            quad = D + (P * m * m - 2 * R * m - vv * R * R) / (1 + vv * P)
            e = e - n[:, None] * log2pi / 2 - L / 2 - np.log1p(vv * P) / 2 - quad / 2
            Qf = np.maximum(quad, 0)
            tail, ltz = chi2TailHost(Qf, n[:, None], dtype=f), wilsonHilfertyHost(Qf, n[:, None], dtype=f)
        M = np.max(e, axis=1, keepdims=True)
        p = np.exp(e - M)
        s = np.sum(p, axis=1)
        py = (erfc((-lz / np.sqrt(f(2))).astype(np.float64)) / 2).astype(f)
        for lst, val in zip((LZ, PY, LTZ, PT), (lz, py, ltz, tail)):
            lst.append(np.sum(p * np.where(n[:, None] > 0, val, f(0)), axis=1) / s)
        l.append(M[:, 0] + np.log(s))
        S.append(s)
    LZ, PY, LTZ, PT, l, S = (np.array(a_) for a_ in (LZ, PY, LTZ, PT, l, S))                 # (R, N)
    om = np.exp(l - np.max(l, axis=0, keepdims=True)) if wt == _lib.SCORE_LIKELIHOOD else np.ones_like(l)
    Wt = np.sum(om, axis=0)
    nan = np.full(N, np.nan)
    mean = lambda a_, on: np.where(on, np.sum(om * a_, axis=0) / Wt, nan)
    coarse = np.any(S < 2.0, axis=0)
    out = OutputPersonFit(lz=mean(LZ, n > 0), pResp=mean(PY, n > 0), ltz=mean(LTZ, n > 0) if t.rt else nan, pTime=mean(PT, n > 0) if t.rt else nan,
                          rowEss=Wt * Wt / np.sum(om * om, axis=0), coarse=coarse, nRows=LZ.shape[0], nNodes=Q, nCoarse=int(np.sum(coarse)),
                          weighting="likelihood" if wt else "equal")
    if obs is not None:
        out.nObs = n.astype(np.int32)
    return (out, S) if with_S else out


# ------------------------------------------------------------------------------------------------------------------
# Item fit and drift: itemFit's twin beside personFitHost, on _marginal_rows_host's law
# ------------------------------------------------------------------------------------------------------------------
def itemFitHost(model, Y, logT, X, rows, nodes=_lib.MARGINAL_NODES, obs=None, dtype=np.float64, with_cells=False, with_S=False) -> OutputItemFit:
    """itemFit with numpy (the test twin of item_fit_kernel and its reduction), written beside personFitHost: the population law of every row from
    _marginal_rows_host; then the definition of include/ertirt.h restated as masked sums -- at every node of an observed cell r, c, z^2 and the signed residual
    e from eta, the leave-one-item-out response-time residual d from the subject's observed times, e_q from the same sums; the six means under the rule's weights
    at the row; their equal-weight means over the rows; the sums over the subjects that observed the item.  obs (N, J), 0/1: the observed mask (the masked call
    never reduces the data and calls itself).  dtype=np.longdouble: the same arithmetic in extended precision.  with_cells: also the (N, J, 6) table of the
    per-cell means E[e], E[r^2], E[c], E[z^2], E[d], E[d^2] (0 at unobserved cells); with_S: also S (R, N), the rule's sum at every row."""
    if model not in _lib.MARGINAL_MODELS:
        raise ValueError("itemFitHost serves the five models without quantile weights")
    Q = _lib.marginal_nodes(nodes)
    t = _lib.MODEL_TRAITS[model]
    f = dtype
    O = np.ones(np.shape(Y), dtype=bool) if obs is None else _obs_mask(obs, np.shape(Y))
    Yz = np.where(O, np.asarray(Y), 0)
    ltz_in = np.where(O, np.asarray(logT, dtype=np.float64), 0.0) if t.rt else None
    N, J = Yz.shape
    rows2 = np.atleast_2d(np.asarray(rows, dtype=np.float64))
    R = rows2.shape[0]
    log2pi = np.log(2 * np.arccos(f(-1)))
    h = f(12) / (Q - 1)
    cells = np.zeros((N, J, 6), dtype=f)
    S = np.empty((R, N), dtype=f)
    step = 256                                                                                # subjects at a time: the (n, Q, J) arrays stay small
    for k, ((_, z, law, _), row) in enumerate(zip(_marginal_rows_host(model, Yz, ltz_in, X, rows2, Q), rows2)):
        mu, sd, m0, m1, v = law
        a, b, lam, sg = (row[c * J:(c + 1) * J].astype(f) for c in range(4))
        rho = row[4 * J:5 * J].astype(f) if t.rho else np.zeros(J, dtype=f)
        z = z.astype(f)
        vv = f(max(v, 0.0))
        for lo in range(0, N, step):
            sl = slice(lo, min(lo + step, N))
            Of = O[sl].astype(f)
            Oq = Of[:, None, :]
            Yf = Yz[sl].astype(f)
            y1 = (Yz[sl] == 1)[:, None, :]
            n = O[sl].sum(axis=1)
            th = np.asarray(mu, dtype=f)[sl, None] + f(sd) * z[None, :]                       # (n, Q)
            eta = a[None, None, :] * (th[:, :, None] - b[None, None, :])                      # (n, Q, J)
            ab = np.abs(eta)
            tt = np.exp(-ab)
            agree = y1 == (eta >= 0)
            r = np.where(agree, tt / (1 + tt), 1 / (1 + tt))
            c = tt / ((1 + tt) * (1 + tt))
            z2 = np.where(agree, tt, np.exp(np.minimum(ab, f(700))))
            sgn = 2 * Yf[:, None, :] - 1
            e = np.log(h) - log2pi / 2 - z[None, :] ** 2 / 2 + np.sum(Oq * (Yf[:, None, :] * eta - (np.maximum(eta, 0) + np.log1p(tt))), axis=2)
            vals = [sgn * r, r * r, c, z2]
            if t.rt:
                lt = ltz_in[sl].astype(f)
                g = Of / sg[None, :]                                                          # (n, J): g_j at the observed cells, 0 elsewhere
                u = lam[None, None, :] - rho[None, None, :] * th[:, :, None] - lt[:, None, :]
                P, Rs, D = np.sum(g, axis=1)[:, None], np.sum(g[:, None, :] * u, axis=2), np.sum(g[:, None, :] * u * u, axis=2)
                L = np.sum(Of * np.log(sg)[None, :], axis=1)[:, None]
                m = (np.asarray(m0, dtype=f)[sl, None] if np.ndim(m0) else f(m0)) + f(m1) * th
                e = e - n[:, None] * log2pi / 2 - L / 2 - np.log1p(vv * P) / 2 - (D + (P * m * m - 2 * Rs * m - vv * Rs * Rs) / (1 + vv * P)) / 2
                gj = (1 / sg)[None, None, :]
                Pi = 1 + vv * (P[:, :, None] - gj)
                with np.errstate(invalid="ignore", divide="ignore"):                          # (an unobserved cell's g_j is not in P: its values are dropped below)
                    d = -(u - (m[:, :, None] + vv * (Rs[:, :, None] - gj * u)) / Pi) / np.sqrt(sg[None, None, :] + vv / Pi)
                vals += [d, d * d]
            M = np.max(e, axis=1, keepdims=True)
            p = np.exp(e - M)
            s = np.sum(p, axis=1)
            S[k, sl] = s
            w = (p / s[:, None])[:, :, None]
            for col, val in enumerate(vals):
                cells[sl, :, col] += np.where(O[sl], np.sum(w * val, axis=1), f(0))
    cells /= R
    sums = cells.sum(axis=0)                                                                  # (J, 6)
    n_j = O.sum(axis=0).astype(f)
    with np.errstate(divide="ignore", invalid="ignore"):
        nan = np.full(J, np.nan)
        on = n_j > 0
        pick = lambda val, ok=True: np.where(on, val, nan).astype(np.float64) if ok else nan
        coarse = np.any(S < 2.0, axis=0)
        out = OutputItemFit(infit=pick(sums[:, 1] / sums[:, 2]), outfit=pick(sums[:, 3] / n_j), respZ=pick(sums[:, 0] / np.sqrt(sums[:, 2])),
                            rtMsq=pick(sums[:, 5] / n_j, t.rt), rtZ=pick(sums[:, 4] / np.sqrt(n_j), t.rt), nObs=O.sum(axis=0).astype(np.int64), nRows=R, nNodes=Q,
                            nCoarse=int(np.sum(coarse)), nSubj=N)
    extra = ([cells] if with_cells else []) + ([S] if with_S else [])
    return (out, *extra) if extra else out


def pvRow(k, K, n_rows):
    """The row of draw k: ((2 k + 1) n_rows) // (2 K) (pv_row of csrc/erm_pv.hpp)."""
    return ((2 * np.asarray(k, dtype=np.int64) + 1) * np.int64(n_rows)) // np.int64(2 * K)


def pvGumbel(w):
    """The Gumbel variate of a 32-bit word: -log(-log((w + 1/2) 2^-32)) (pv_gumbel)."""
    return -np.log(-np.log(_ppc_uniform(np.asarray(w, dtype=np.uint64))))


def pvFinish(E, V, mu, sd, c0, c1, u, q, h, w0, w1, w2):
    """(theta, zeta) of a draw at node q of a row with moments E, V, law (mu, sd) and zeta conditional (c0, c1, u), from the finishing block's words (pv_finish)."""
    cell = sd * h
    star = (mu + sd * (-6.0 + q * h)) + cell * (_ppc_uniform(w0) - 0.5)
    c = np.where(V > 0.0, np.sqrt(V / (V + cell * cell / 12.0)), 0.0)
    theta = E + c * (star - E)
    return theta, (c0 + c1 * theta) + np.sqrt(u) * _ppc_normal(w1, w2)


def plausibleValuesHost(model, Y, logT, X, rows, K=_lib.PV_DRAWS, seed=_lib.PV_SEED, nodes=_lib.MARGINAL_NODES, i_base=0, with_gap=False, with_rows=False, obs=None):
    """drawPlausibleValues with numpy (the test twin of pv_kernel), written beside scoresHost on _marginal_rows_host and _philox4x32_10.  i_base: the data-set index
    of Y's first subject.  with_gap=True also returns, per draw, the difference of the two largest keys (N, K): a draw whose gap is below the rounding of e_q is
    undecidable between two implementations.  with_rows=True also returns the rows r_k (K,) and the row moments E, V (N, K) each draw was made from.
    obs (N, J), 0/1: the observed mask of incomplete patterns; the result then carries nObs (N,)."""
    if model not in _lib.MARGINAL_MODELS:
        raise ValueError("plausibleValuesHost serves the five models without quantile weights")
    Q, K, seed = _lib.marginal_nodes(nodes), _lib.pv_draws(K), _lib.pv_seed(seed)
    rt = _lib.MODEL_TRAITS[model].rt
    rows = np.atleast_2d(np.asarray(rows, dtype=np.float64))
    rk = pvRow(np.arange(K), K, rows.shape[0])
    used = np.unique(rk)
    N = np.shape(Y)[0]
    h = 12.0 / (Q - 1)
    ii = (np.arange(N, dtype=np.uint64) + np.uint64(i_base))
    site = _ppc_stream_word3(0, _lib.PV_SITE)
    theta, zeta, node, gap = np.empty((N, K)), np.full((N, K), np.nan), np.empty((N, K), dtype=np.int32), np.empty((N, K))
    Ek, Vk = np.empty((N, K)), np.empty((N, K))
    coarse = np.zeros(N, dtype=bool)
    for r, (e, z, law, sums) in zip(used, _marginal_rows_host(model, Y, logT, X, rows[used], Q, obs=obs)):
        (mu, sd), (E, V, c0, c1, u, _, s) = law[:2], _row_moments(e, z, law, sums, rt)
        coarse |= s < 2.0
        ks = np.nonzero(rk == r)[0]
        w0 = _philox4x32_10(ii[:, None, None], ks[None, :, None], np.arange(Q)[None, None, :], site, seed, seed >> 32)[0]      # (N, draws, Q)
        key = e[:, None, :] + pvGumbel(w0)
        q = np.argmax(key, axis=2)                                                                                           # the first of equal keys: the smaller q
        top = np.sort(key, axis=2)
        f0, f1, f2, _ = _philox4x32_10(ii[:, None], ks[None, :], 0xFFFFFFFF, site, seed, seed >> 32)                        # (N, draws)
        col = lambda a: a[:, None] if np.ndim(a) else a
        th, ze = pvFinish(col(E), col(V), col(mu), sd, col(c0), col(c1), col(u), q, h, f0, f1, f2)
        theta[:, ks], node[:, ks], gap[:, ks] = th, q, top[:, :, -1] - top[:, :, -2]
        Ek[:, ks], Vk[:, ks] = col(E), col(V)
        if rt:
            zeta[:, ks] = ze
    out = OutputPv(theta=theta, zeta=zeta, node=node, coarse=coarse, nRows=rows.shape[0], nNodes=Q, nCoarse=int(np.sum(coarse)), seed=seed)
    if obs is not None:
        out.nObs = _obs_mask(obs, np.shape(Y)).sum(axis=1).astype(np.int32)
    extra = ((gap,) if with_gap else ()) + ((rk, Ek, Vk),) * bool(with_rows)
    return (out, *extra) if extra else out


_PPC_SITE = 14          # the replicate draws' stream site (erm_predictive_kernels.hpp: SITE_PRED)


def _philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 (Salmon et al. 2011) on broadcastable arrays of 32-bit counter and key words; returns the four output words as uint64 arrays < 2^32."""
    m32 = np.uint64(0xFFFFFFFF)
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) & m32 for c in np.broadcast_arrays(c0, c1, c2, c3))
    k0, k1 = np.uint64(int(k0) & 0xFFFFFFFF), np.uint64(int(k1) & 0xFFFFFFFF)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & m32, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & m32
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & m32, (k1 + np.uint64(0xBB67AE85)) & m32
    return c0, c1, c2, c3


def _ppc_uniform(w):
    return (w.astype(np.float64) + 0.5) * 2.0 ** -32


def _ppc_normal(wa, wb):
    return np.sqrt(-2.0 * np.log(_ppc_uniform(wa))) * np.cos(2.0 * np.pi * _ppc_uniform(wb))


def _ppc_stream_word3(chain, site=_PPC_SITE, k=0):
    return (site << 24) | ((chain & 0xFF) << 16) | k


def getPpcHost(MCMC: _GibbsBase, thin=1, sweep0=1, *, seed=None, chain=None, row_base=0) -> OutputPpc:
    """getPpc evaluated with numpy on the host from MCMC.Data and the full Post traces (the test twin of the device path): the same replicate draws -- one
    Philox4x32-10 block per cell at (site 14, subject, item, sweep, chain) -- and the same discrepancies.  sweep0: the global sweep index of trace row 0 (1 on a
    fresh engine or after setSeed; it goes on counting over erm_reset_trace).  The result also carries `margin`: per unit and component the smallest non-zero
    |D_rep - D_obs| over the replicate rows relative to the magnitudes compared (a count is decided beyond rounding when its margin is far above 1e-16)."""
    C, D, P, m = MCMC.Cond, MCMC.Data, MCMC.Post, MCMC._model
    N, J = C.nSubj, C.nItem
    if thin < 1:
        raise ValueError("thin must be at least 1")
    if np.ndim(P.ra) != 3:
        raise ValueError("getPpcHost needs the full Post traces (trace='full' and fill=True)")
    seed = int(MCMC.seed if seed is None else seed)
    chain = int(getattr(MCMC, "chain_id", 0) if chain is None else chain)
    Y = np.asarray(D.Y, dtype=np.float64)
    rt_model = m != _lib.MODEL_MLIRT
    logT = np.asarray(D.logT, dtype=np.float64) if rt_model else None
    if m == _lib.MODEL_CROSSQR and P.qr.shape[1] != J + 4 + N * J:
        raise ValueError("getPpcHost needs the per-sweep nu trace of GibbsRtIrtCrossQr in Post.qr")
    ii, jj = np.arange(N, dtype=np.uint64)[:, None] + np.uint64(row_base), np.arange(J, dtype=np.uint64)[None, :]
    item, subj, total = np.zeros((3, 4, J)), np.zeros((2, 4, N)), np.zeros((2, 4))
    margin = dict(item=np.full((3, J), np.inf), subject=np.full((2, N), np.inf), total=np.full(2, np.inf))
    if not rt_model:
        item[1], subj[1], total[1] = np.nan, np.nan, np.nan

    def update(acc, mar, obs, rep, diff, scale):
        acc[0] += diff >= 0
        acc[1] += diff > 0
        acc[2] += obs
        acc[3] += rep
        with np.errstate(divide="ignore", invalid="ignore"):
            rel = np.where(diff != 0, np.abs(diff) / scale, np.inf)
        np.minimum(mar, rel, out=mar)

    R = 0
    post = [(it, l) for it in range(C.nBurnin, C.nIter) for l in range(C.nChain)]
    for k, (it, l) in enumerate(post):
        if k % thin:
            continue
        R += 1
        sweep = sweep0 + it * C.nChain + l
        ra = P.ra[it, :, l]
        th, a, b = ra[:N], ra[N:N + J], ra[N + J:N + 2 * J]
        eta = a[None, :] * (th[:, None] - b[None, :])
        with np.errstate(over="ignore"):
            p = 1.0 / (1.0 + np.exp(-eta))
        w0, w1, w2, _ = _philox4x32_10(ii, jj, sweep, _ppc_stream_word3(chain), seed, seed >> 32)
        yrep = (_ppc_uniform(w0) < p).astype(np.float64)
        lobs = Y * eta - _log1pexp(eta)
        dcell = (Y - yrep) * eta                        # l(y) - l(y_rep): D_rep - D_obs = 2 sum dcell
        for ax, acc, mar in ((1, subj, margin["subject"]), (0, item, margin["item"]), (None, total, margin["total"])):
            dobs, dlt = -2.0 * lobs.sum(axis=ax), dcell.sum(axis=ax)
            update(acc[0], mar[0] if ax is not None else mar[0:1], dobs, dobs + 2.0 * dlt, dlt, np.abs(dcell).sum(axis=ax))
        tobs, trep = Y.sum(axis=0), yrep.sum(axis=0)
        update(item[2], margin["item"][2], tobs, trep, trep - tobs, 1.0)
        if rt_model:
            mu, var = _rt_cell_law(MCMC, it, l, th)
            z = _ppc_normal(w1, w2)                     # logT_rep = mu + sqrt(var) z: its standardised square is z^2
            cobs, crep = (logT - mu) ** 2 / var, z * z
            for ax, acc, mar in ((1, subj, margin["subject"]), (0, item, margin["item"]), (None, total, margin["total"])):
                o, r_ = cobs.sum(axis=ax), crep.sum(axis=ax)
                update(acc[1], mar[1] if ax is not None else mar[1:2], o, r_, r_ - o, o + r_)
    if R == 0:
        raise ValueError("posterior predictive checks need at least one replicate row")
    for acc in (item, subj, total):
        acc[:, 2:4] /= R
    out = OutputPpc(R=R, thin=thin, item=item, subj=subj, total=total)
    out.margin = margin
    return out


def ess_rhat(x: np.ndarray):
    """Split-R-hat and effective sample size (Geyer's initial monotone sequence over the split chains; BDA3 sec. 11.4-11.5, the
    non-rank-normalised estimator) of draws x[(iteration, chain)] -- the host twin of the device kernel `diag_kernel`, used by its
    tests and for traces that are not resident on the device.  A column that never moves -- every used draw (the first and last
    floor(T / 2) of every chain) equal to the first one -- gets (nan, nan); a column whose first pair sum rho_0 + rho_1 is not positive gets
    ess = -M n (M = 2 * chains sequences of n draws): the sum of pair sums stops before it (and pair sums that add up to less than 1 / 2 give a negative ess)."""
    x = np.asarray(x, dtype=np.float64)
    if x.ndim == 1:
        x = x[:, None]
    T, C = x.shape
    n = T // 2
    seq = np.stack([x[:n, l] if h == 0 else x[T - n:, l] for l in range(C) for h in (0, 1)])      # (M, n)
    M = seq.shape[0]
    if not np.any(seq != seq[0, 0]):          # decided on the draws: the rounded mean of n copies of 0.1 is not 0.1, and W > 0 would be rounding noise
        return float("nan"), float("nan")
    mu = seq.mean(axis=1)
    d = seq - mu[:, None]
    W = np.mean(np.sum(d * d, axis=1) / (n - 1))
    Bn = np.sum((mu - mu.mean()) ** 2) / (M - 1)
    varp = W * (n - 1) / n + Bn

    def rho(t):
        return 1.0 - (W - np.mean(np.sum(d[:, :n - t] * d[:, t:], axis=1) / n)) / varp

    total, prev, t = 0.0, np.inf, 0
    while t + 1 < n:
        P = rho(t) + rho(t + 1)
        if not P > 0:
            break
        P = min(P, prev)
        prev = P
        total += P
        t += 2
    return M * n / (-1.0 + 2.0 * total), float(np.sqrt(varp / W))


def rank_ess_rhat(x: np.ndarray):
    """(ess_bulk, ess_tail, rhat_rank) of draws x[(iteration, chain)]: the rank-normalised diagnostics of Vehtari et al. (2021) as include/ertirt.h defines them
    for erm_get_rank_diagnostics -- the host twin of the device kernel `rank_diag_kernel`, on numpy / scipy.  The used draws are ess_rhat's (the first and last
    floor(T / 2) of every chain), pooled: z = ndtri((average rank - 3/8) / (S + 1/4)), ess_bulk = E(z); f = |x - med| with med the mean of the two middle order
    statistics, rhat_rank = the larger of R(z) and R(z(f)) (R(z) alone when f is constant); with k = ceil(S / 20), ess_tail = the smaller of E([x <= x_(k)]) and
    E([x >= x_(S+1-k)]), NaN if either indicator is constant.  E and R are ess_rhat's.  A column that never moves gets three NaN."""
    from scipy.special import ndtri
    from scipy.stats import rankdata
    x = np.asarray(x, dtype=np.float64)
    if x.ndim == 1:
        x = x[:, None]
    T, C = x.shape
    n = T // 2
    u = np.concatenate([x[:n], x[T - n:]], axis=0)                # the used draws [2 n, chain]: ess_rhat splits them exactly as it splits x
    S = u.size
    nan = float("nan")
    if not np.any(u != u[0, 0]):
        return nan, nan, nan

    def scores(v):
        return ndtri((rankdata(v.ravel(), method="average").reshape(v.shape) - 0.375) / (S + 0.25))

    srt = np.sort(u.ravel())
    k = (S + 19) // 20
    ess_bulk, rz = ess_rhat(scores(u))
    med = 0.5 * (srt[S // 2 - 1] + srt[S // 2])
    _, rf = ess_rhat(scores(np.abs(u - med)))
    el, _ = ess_rhat((u <= srt[k - 1]).astype(np.float64))
    eu, _ = ess_rhat((u >= srt[S - k]).astype(np.float64))
    ess_tail = nan if (np.isnan(el) or np.isnan(eu)) else min(el, eu)
    return ess_bulk, ess_tail, (rf if (not np.isnan(rf) and rf > rz) else rz)



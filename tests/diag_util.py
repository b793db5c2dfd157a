"""An independent reference for the convergence diagnostics (erm_get_diagnostics / erm_get_convergence, twins.ess_rhat): split-R-hat and the effective sample
size by Geyer's initial monotone sequence, written from the definition in include/ertirt.h and above `diag_kernel` -- nothing is imported from the package.

The definition.  The post-burn-in draws of a column are x[i, l], i = 0 .. Tn - 1, for the chains l = 0 .. C - 1.  With n = floor(Tn / 2), every chain is split
into its first n and its last n draws (rows 0 .. n - 1 and Tn - n .. Tn - 1: an odd Tn leaves the middle draw out), M = 2 C sequences of n draws.  With mu_c the
mean of sequence c and d_ci = x_ci - mu_c:
    W      = mean_c  sum_i d_ci^2 / (n - 1)                         the mean within-sequence variance
    B / n  = sum_c (mu_c - mean_c mu_c)^2 / (M - 1)                 the variance of the sequence means
    var+   = (n - 1) / n  W + B / n
    rhat   = sqrt(var+ / W)
    rho_t  = 1 - (W - mean_c (1 / n) sum_{i < n - t} d_ci d_c,i+t) / var+
    P_k    = rho_2k + rho_2k+1       for 2 k + 1 < n
    ess    = M n / (-1 + 2 sum_k min(P_0 .. P_k))   summed over k = 0, 1, ... as long as P_k > 0: the sum stops BEFORE the first P_k that is not positive
A column whose used draws are all equal never moves and has neither statistic (NaN).  A column whose FIRST pair sum is not positive has an empty sum and gets -M n.

Two implementations:
  reference(x)        np.longdouble (64-bit significand), direct lag sums, every column of a trace at once
  exact(x)            fractions.Fraction, one column of integers: rhat^2 and ess as rationals, and the pair sums the loop evaluated
"""
from __future__ import annotations

from fractions import Fraction

import numpy as np

ESS_RTOL = 1e-6          # the project's tolerances for the device against a host estimator (tests/test_gpu_golden.py)
RHAT_ATOL = 1e-9
MARGIN_MIN = 1e-9        # a stop rule decided by less than this may stop elsewhere in another correct implementation
SKIP_CAP = 1e-3          # at most one column in 1000 of a trace may be left out of a comparison for that reason


def _require_longdouble():
    if np.finfo(np.longdouble).nmant < 63:
        raise RuntimeError("np.longdouble is not wider than fp64 on this platform")


def split(x):
    """x[iteration, column, chain] -> the M = 2 * chains split sequences [sequence, draw, column] (sequence 2 l: first half of chain l, 2 l + 1: its last half)."""
    x = np.asarray(x)
    if x.ndim != 3:
        raise ValueError("x must be [iteration, column, chain]")
    Tn, K, C = x.shape
    n = Tn // 2
    if n < 2:
        raise ValueError("need at least four draws")
    return np.stack([x[:n, :, l] if h == 0 else x[Tn - n:, :, l] for l in range(C) for h in (0, 1)]), n


def reference(x):
    """x[iteration, column, chain]: the post-burn-in part of a trace in Julia layout.  Returns dict(ess, rhat, constant, margin, p0, terms, M, n):
    ess / rhat per column as np.longdouble (NaN where `constant`), constant = the used draws of the column are all equal (their maximum equals their minimum),
    margin = the smallest |P_k| over the pair sums the loop evaluated, the one that stopped it included (inf for a constant column), p0 = the first pair sum,
    terms = the number of pair sums that entered the sum."""
    _require_longdouble()
    seq, n = split(x)
    M, _, K = seq.shape
    constant = seq.max(axis=(0, 1)) == seq.min(axis=(0, 1))
    s = seq.astype(np.longdouble)
    ln, lM = np.longdouble(n), np.longdouble(M)
    mu = s.sum(axis=1) / ln                                     # (M, K)
    d = s - mu[:, None, :]
    W = ((d * d).sum(axis=1) / (ln - 1)).sum(axis=0) / lM
    mbar = mu.sum(axis=0) / lM
    Bn = ((mu - mbar[None, :]) ** 2).sum(axis=0) / (lM - 1)
    varp = (ln - 1) / ln * W + Bn
    live = ~constant
    with np.errstate(divide="ignore", invalid="ignore"):
        rhat = np.sqrt(varp / W)

        def rho(t):
            acov = (d[:, :n - t, :] * d[:, t:, :]).sum(axis=1) / ln          # (M, K)
            return 1 - (W - acov.sum(axis=0) / lM) / varp

        total = np.zeros(K, dtype=np.longdouble)
        prev = np.full(K, np.inf, dtype=np.longdouble)
        margin = np.full(K, np.inf, dtype=np.longdouble)
        terms = np.zeros(K, dtype=np.int64)
        p0 = np.full(K, np.nan, dtype=np.longdouble)
        run = live.copy()
        t = 0
        while t + 1 < n and run.any():
            P = rho(t) + rho(t + 1)
            if t == 0:
                p0 = np.where(live, P, p0)
            margin = np.where(run, np.minimum(margin, np.abs(P)), margin)
            run = run & (P > 0)
            P = np.minimum(P, prev)
            prev = np.where(run, P, prev)
            total = np.where(run, total + P, total)
            terms += run
            t += 2
        ess = lM * ln / (-1 + 2 * total)
    nan = np.longdouble("nan")
    return dict(ess=np.where(live, ess, nan), rhat=np.where(live, rhat, nan), constant=constant, margin=margin, p0=p0, terms=terms, M=M, n=n)


def exact(x):
    """One column of INTEGER draws x[iteration, chain] (or x[iteration]) in exact rational arithmetic.  Returns None for a column that never moves, else
    dict(rhat2, ess, P, M, n): rhat^2 = var+ / W and ess as Fractions, P = the pair sums the loop evaluated (the one that stopped it included)."""
    x = np.asarray(x)
    if x.ndim == 1:
        x = x[:, None]
    if not np.all(x == np.round(x)):
        raise ValueError("exact() takes integer-valued draws")
    Tn, C = x.shape
    n = Tn // 2
    seq = []
    for l in range(C):
        col = [Fraction(int(v)) for v in x[:, l]]
        seq += [col[:n], col[Tn - n:]]
    M = len(seq)
    if all(v == seq[0][0] for s in seq for v in s):
        return None
    mu = [sum(s) / n for s in seq]
    d = [[v - m for v in s] for s, m in zip(seq, mu)]
    W = sum(sum(v * v for v in dc) / (n - 1) for dc in d) / M
    mbar = sum(mu) / M
    Bn = sum((m - mbar) ** 2 for m in mu) / (M - 1)
    varp = Fraction(n - 1, n) * W + Bn
    if W == 0:
        raise ValueError("every sequence is constant but they differ: W = 0, R-hat is infinite")

    def rho(t):
        acov = sum(sum(dc[i] * dc[i + t] for i in range(n - t)) / n for dc in d) / M
        return 1 - (W - acov) / varp

    total, prev, P_seen = Fraction(0), None, []
    t = 0
    while t + 1 < n:
        P = rho(t) + rho(t + 1)
        P_seen.append(P)
        if not P > 0:
            break
        if prev is not None and P > prev:
            P = prev
        prev = P
        total += P
        t += 2
    return dict(rhat2=varp / W, ess=Fraction(M * n) / (-1 + 2 * total), P=P_seen, M=M, n=n)


def compare(ess, rhat, ref, *, ess_rtol=ESS_RTOL, rhat_atol=RHAT_ATOL, margin_min=MARGIN_MIN):
    """An estimator's (ess, rhat) per column against reference(x).  Constant columns must be NaN in both statistics and no other column may be; columns whose stop
    rule was decided by less than `margin_min` are left out of the value comparison and counted.  Returns dict(ess_err, rhat_err: the worst |ess - e| / |e| and
    |rhat - r| over the compared columns, skipped, compared, bad: indices of the columns that miss a tolerance or the NaN pattern)."""
    ess, rhat = np.asarray(ess, dtype=np.float64), np.asarray(rhat, dtype=np.float64)
    const = ref["constant"]
    if ess.shape != const.shape or rhat.shape != const.shape:
        raise ValueError(f"{ess.shape} / {rhat.shape} values for {const.shape} columns")
    nan_ok = (np.isnan(ess) == const) & (np.isnan(rhat) == const)
    use = ~const & (ref["margin"] >= margin_min)
    e, r = ref["ess"], ref["rhat"]
    with np.errstate(invalid="ignore", divide="ignore"):
        ee = np.where(use, np.abs(ess.astype(np.longdouble) - e) / np.abs(e), 0).astype(np.float64)
        re = np.where(use, np.abs(rhat.astype(np.longdouble) - r), 0).astype(np.float64)
    bad = ~nan_ok | (use & ~((ee <= ess_rtol) & (re <= rhat_atol)))
    return dict(ess_err=float(ee.max(initial=0.0)), rhat_err=float(re.max(initial=0.0)), skipped=int(np.sum(~const & ~use)), compared=int(np.sum(use)),
                bad=np.flatnonzero(bad))


def counts(ess, rhat, ess_min=400.0, rhat_max=1.1):
    """checkConvergence's four counts from the vectors: columns with a defined ESS, of those ESS > ess_min, columns with a defined R-hat, of those R-hat < rhat_max."""
    ess, rhat = np.asarray(ess, dtype=np.float64), np.asarray(rhat, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        return (int(np.sum(~np.isnan(ess))), int(np.sum(ess > ess_min)), int(np.sum(~np.isnan(rhat))), int(np.sum(rhat < rhat_max)))

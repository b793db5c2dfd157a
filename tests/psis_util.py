"""Helpers shared by the PSIS-LOO tests (tests/test_psis_host.py, tests/test_gpu_psis_loo.py): the synthetic columns of log-likelihoods, the comparison metric and
the tolerance measured from the twin's own conditioning (psisLooHost in fp64 against the same code in np.longdouble)."""
import functools

import numpy as np

import parity_util as pu

S_CPU = (25, 26, 224, 225, 226, 4097, 8192)
S_GPU = (25, 26, 127, 225, 1000, 4097, 8192)
N_GPU = 67
FLOOR = 1e-13
KINDS = ("gauss", "underflow", "ties", "constant", "heavy", "consttail", "span300")


def pkg():
    return pu.ge.load_package()


def tail_len(S):
    return int(min(np.ceil(S / 5.0), np.ceil(3.0 * np.sqrt(S))))


def column(kind, S, g):
    """One unit's l_s, s = 1..S."""
    M = tail_len(S)
    if kind == "gauss":                       # well-behaved Gaussian log-likelihoods
        return g.normal(-30.0, 1.5, S)
    if kind == "underflow":                   # one row 700 below the rest: its ratio is 1, exp of every other log ratio is about 1e-304
        l = g.normal(-30.0, 1.0, S)
        l[int(g.integers(S))] = l.min() - 700.0
        return l
    if kind == "ties":                        # a coarse lattice: exact ties across the cutoff
        return -30.0 + np.round(g.normal(0.0, 1.5, S) * 2.0) / 2.0
    if kind == "constant":
        return np.full(S, -12.5)
    if kind == "heavy":                       # ratios exp(-l) Pareto with shape 1: k^ > 0.7
        return -20.0 - g.exponential(1.0, S)
    if kind == "consttail":                   # the M largest ratios all equal: the tail cannot be fitted
        l = g.normal(-30.0, 1.0, S)
        l[np.argsort(l)[:M + 2]] = l.min() - 1.0
        return l
    if kind == "span300":                     # exceedances from about 1e-300 to 1
        lw = np.full(S, -720.0) - g.uniform(0.0, 1.0, S)
        lw[g.permutation(S)[:M]] = np.linspace(-690.0, 0.0, M)
        return -5.0 - lw
    raise KeyError(kind)


@functools.lru_cache(maxsize=None)
def table(S, N=N_GPU, seed=7):
    """(S, N) table: the kinds in turn, every column its own draw; read-only (shared among the tests)."""
    g = np.random.default_rng(seed * 100003 + S)
    L = np.stack([column(KINDS[u % len(KINDS)], S, g) for u in range(N)], axis=1)
    L.setflags(write=False)
    return L


def kind_of(u):
    return KINDS[u % len(KINDS)]


def rel(a, b):
    """max |a - b| / max(|b|, 1) over the entries where both are finite; the non-finite patterns must agree exactly."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    fa, fb = np.isfinite(a), np.isfinite(b)
    assert np.array_equal(fa, fb), "finite patterns differ"
    assert np.array_equal(a[~fa], b[~fb], equal_nan=True), "non-finite values differ"
    if not np.any(fa):
        return 0.0
    return float(np.max(np.abs(a[fa] - b[fb]) / np.maximum(np.abs(b[fb]), 1.0)))


FIELDS = ("elpd_u", "p_u", "khat", "nEff")


def twin_difference(L):
    """The largest rel() between psisLooHost in fp64 and in np.longdouble over the pointwise columns and the log-weights of the table L."""
    P = pkg()
    lo, lw_lo = P.psisLooHost(L, with_lw=True)
    hi, lw_hi = P.psisLooHost(L, dtype=np.longdouble, with_lw=True)
    return max([rel(getattr(lo, f), getattr(hi, f)) for f in FIELDS] + [rel(lw_lo, lw_hi)])


@functools.lru_cache(maxsize=None)
def measured(sizes):
    """{S: twin_difference(table(S))}"""
    return {S: twin_difference(table(S)) for S in sizes}


def bound(sizes):
    """64 x the largest twin difference over the tables of `sizes`, floored at 1e-13."""
    return max(FLOOR, 64.0 * max(measured(tuple(sizes)).values()))

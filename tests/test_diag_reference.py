"""The convergence diagnostics on the CPU: the longdouble reference of tests/diag_util.py against its own exact-rational twin, and the package's host estimator
`ess_rhat` (the statement-by-statement twin of the device kernel `diag_kernel`) against that reference -- split lengths 8, 9, 17 and 60, 1 to 16 chains, random,
autocorrelated and offset draws, constant columns at dyadic and non-dyadic values, the alternating sequence, scale and shift invariance."""
from fractions import Fraction

import numpy as np
import pytest

import diag_util as du
import parity_util as pu

pkg = pu.ge.load_package()

T_CASES = (8, 9, 17, 60)
SHAPES = [(T, C) for T in T_CASES for C in (1, 2, 3, 16)]
LD_EPS = float(np.finfo(np.longdouble).eps)


def _ar1(g, T, K, C, phi):
    """K columns of C chains of an AR(1) with coefficient phi[column] (negative: antithetic), unit innovation variance."""
    x = np.empty((T, K, C))
    x[0] = g.standard_normal((K, C))
    for t in range(1, T):
        x[t] = phi[:, None] * x[t - 1] + g.standard_normal((K, C))
    return x


def _ld(q):
    """A Fraction as a longdouble: numerator and denominator rounded, then one division."""
    return np.longdouble(q.numerator) / np.longdouble(q.denominator)


def _twin(x):
    """ess_rhat column by column on x[iteration, column, chain]."""
    out = np.array([pkg.ess_rhat(x[:, k, :]) for k in range(x.shape[1])])
    return out[:, 0], out[:, 1]


@pytest.mark.parametrize("T,C", SHAPES)
def test_longdouble_reference_equals_exact_arithmetic(T, C):
    """Small integers: the data, the means times n and every lag sum are exact in both, so the longdouble result is the rational one rounded a few times."""
    g = np.random.default_rng(100 * T + C)
    K = 12
    x = g.integers(-9, 10, size=(T, K, C)).astype(np.float64)
    x[:, 0, :] = np.cumsum(g.integers(-1, 2, size=(T, C)), axis=0)          # a random walk: many positive pair sums
    x[:, 1, :] = (np.arange(T) % 3)[:, None]                                # a periodic column
    x[:, 2, :] = 7.0                                                        # a constant one
    ref = du.reference(x)
    assert ref["M"] == 2 * C and ref["n"] == T // 2
    for k in range(K):
        ex = du.exact(x[:, k, :])
        if ex is None:
            assert ref["constant"][k] and np.isnan(ref["ess"][k]) and np.isnan(ref["rhat"][k]) and k == 2
            continue
        assert not ref["constant"][k]
        assert abs(ref["p0"][k] - _ld(ex["P"][0])) <= 64 * LD_EPS
        assert ref["terms"][k] == len(ex["P"]) - (0 if ex["P"][-1] > 0 else 1)
        # ess = M n / (-1 + 2 sum): a relative error of the denominator; its terms are O(1) and there are at most n / 2 of them
        den = abs(float(-1 + 2 * sum(min(ex["P"][:j + 1]) for j in range(ref["terms"][k]))))
        tol = 64 * LD_EPS * (1 + T) / den
        assert abs(ref["ess"][k] / _ld(ex["ess"]) - 1) <= tol, (k, ref["ess"][k], ex["ess"])
        assert abs(ref["rhat"][k] ** 2 / _ld(ex["rhat2"]) - 1) <= 64 * LD_EPS, (k, ref["rhat"][k], ex["rhat2"])


@pytest.mark.parametrize("T", T_CASES)
@pytest.mark.parametrize("C", (1, 2))
def test_alternating_sequence_gets_minus_M_n(T, C):
    """x_i = (-1)^i: every n here is even, so each split sequence has mean 0, W = n / (n - 1), var+ = 1, rho_0 = 1 - 1 / (n - 1),
    rho_1 = 1 - n / (n - 1) - (n - 1) / n and P_0 = -(n + 1) / (n (n - 1)) < 0.  The sum stops before its first term: ess = M n / (-1) = -M n, a defined and
    negative value (-16 for two chains of 8 or 9, -120 for two chains of 60).  The estimator is kept as it is; this test pins the behaviour so that a later
    change is deliberate."""
    n, M = T // 2, 2 * C
    assert n % 2 == 0
    x = np.repeat(((-1.0) ** np.arange(T))[:, None], C, axis=1)
    p0 = Fraction(-(n + 1), n * (n - 1))
    ex = du.exact(x)
    assert ex["P"] == [p0] and ex["ess"] == -M * n and ex["rhat2"] == Fraction(n - 1, n)
    ref = du.reference(x[:, None, :])
    assert abs(ref["p0"][0] - _ld(p0)) <= 8 * LD_EPS and ref["terms"][0] == 0 and not ref["constant"][0]
    assert float(ref["ess"][0]) == -M * n and abs(float(ref["rhat"][0]) - np.sqrt((n - 1) / n)) <= 1e-15
    assert abs(ref["margin"][0] - _ld(-p0)) <= 8 * LD_EPS          # the stop is decided far from rounding
    e, r = pkg.ess_rhat(x)
    assert e == -M * n and abs(r - np.sqrt((n - 1) / n)) <= du.RHAT_ATOL
    e5, r5 = pkg.ess_rhat(3.0 + 0.25 * x)                                   # the same column shifted and scaled
    assert e5 == -M * n and abs(r5 - r) <= du.RHAT_ATOL


def _inputs(T, C, seed):
    """Columns of every kind: white noise, AR(1) from strongly antithetic to strongly persistent, chains with different means (R-hat well above 1), and the same
    kinds at an offset of 1e6 and at a scale of 1e-3."""
    g = np.random.default_rng(seed)
    phi = np.array([0.0, 0.0, 0.3, 0.6, 0.9, 0.97, -0.3, -0.6, -0.9, 0.5, 0.8, 0.0])
    x = _ar1(g, T, phi.size, C, phi)
    x[:, 9:, :] += 1.5 * g.standard_normal((1, 3, C))                        # chain-specific levels
    return np.concatenate([x, 1e6 + x, 1e-3 * x, -2.5e3 + 40.0 * x], axis=1)


@pytest.mark.parametrize("T,C", SHAPES)
def test_host_twin_matches_the_reference(T, C):
    x = _inputs(T, C, seed=7 * T + C)
    ref = du.reference(x)
    assert not ref["constant"].any()
    ess, rhat = _twin(x)
    cmp_ = du.compare(ess, rhat, ref)
    assert cmp_["bad"].size == 0, (cmp_, ess[cmp_["bad"]], ref["ess"][cmp_["bad"]])
    assert cmp_["skipped"] == 0 and cmp_["compared"] == x.shape[1]


@pytest.mark.parametrize("value", [0.0, 1.0, 0.1, 1.0 / 3.0])
@pytest.mark.parametrize("T,C", [(8, 1), (9, 2), (17, 3), (61, 3), (60, 16)])
def test_a_column_that_never_moves_is_nan(value, T, C):
    """"Never moves" is decided on the draws.  The mean of n rounded copies of 0.1 or 1/3 is not that value for most n, which leaves deviations of one ulp and a
    W > 0 of rounding noise: (61, 3) at 0.1 gave (5.128..., 1.121...) before the rule was changed."""
    x = np.full((T, 1, C), value)
    ref = du.reference(x)
    assert ref["constant"][0] and np.isnan(ref["ess"][0]) and np.isnan(ref["rhat"][0]) and ref["margin"][0] == np.inf
    e, r = pkg.ess_rhat(x[:, 0, :])
    assert np.isnan(e) and np.isnan(r), (e, r)
    if T % 2:                                   # the middle draw of an odd length is not used: it does not make the column move
        x[T // 2] = value + 1.0
        assert du.reference(x)["constant"][0] and np.isnan(pkg.ess_rhat(x[:, 0, :])[0])
    x[T - 1, 0, C - 1] = value + 1.0            # the very last used draw does
    e, r = pkg.ess_rhat(x[:, 0, :])
    assert not du.reference(x)["constant"][0] and np.isfinite(e) and np.isfinite(r)


@pytest.mark.parametrize("T,C", [(9, 1), (17, 3), (60, 2), (60, 16)])
def test_scale_and_shift_invariance(T, C):
    """x -> 4 x multiplies every intermediate by a power of two: nothing rounds differently, the results are bit-identical.  x -> x + c changes the roundings of
    the deviations only: within the tolerances."""
    x = _inputs(T, C, seed=900 + T + C)[:, :12, :]
    e1, r1 = _twin(x)
    e4, r4 = _twin(4.0 * x)
    assert np.array_equal(e1, e4) and np.array_equal(r1, r4)
    ref, ref4 = du.reference(x), du.reference(4.0 * x)
    assert np.array_equal(ref["ess"], ref4["ess"]) and np.array_equal(ref["rhat"], ref4["rhat"])
    for c in (1.0, -37.5, 1e4):
        ec, rc = _twin(x + c)
        refc = du.reference(x + c)
        for got in ((ec, rc), (np.asarray(refc["ess"], dtype=float), np.asarray(refc["rhat"], dtype=float))):
            cmp_ = du.compare(got[0], got[1], ref)
            assert cmp_["bad"].size == 0 and cmp_["skipped"] == 0, (c, cmp_)


def test_margin_reports_the_closest_stop_decision():
    g = np.random.default_rng(5)
    x = _ar1(g, 60, 40, 2, np.linspace(-0.9, 0.95, 40))
    ref = du.reference(x)
    for k in range(0, 40, 7):
        xi = np.round(x[:, k, :] * 64)                                      # integers: the exact twin sees the same column
        ex, rf = du.exact(xi), du.reference(xi[:, None, :])
        assert abs(rf["margin"][0] - _ld(min(abs(p) for p in ex["P"]))) <= 64 * LD_EPS
    assert np.all(ref["margin"] > 0) and np.all(np.isfinite(np.asarray(ref["margin"], dtype=float)))
    cmp_ = du.compare(np.asarray(ref["ess"], dtype=float), np.asarray(ref["rhat"], dtype=float), ref, margin_min=float(np.sort(ref["margin"])[3]))
    assert cmp_["skipped"] == 3 and cmp_["compared"] == 37 and cmp_["bad"].size == 0


def test_counts_follow_check_convergence():
    nan = float("nan")
    ess = np.array([nan, 400.0, 400.0000001, -120.0, 1e9, np.inf, 3.0])
    rhat = np.array([nan, 1.1, 1.0999999, 0.9, np.inf, 1.0, nan])
    assert du.counts(ess, rhat) == (6, 3, 5, 3)


def _oracle_traces(model, N, J, n_iter, n_chain):
    """The CPU oracle's chain of n_iter * n_chain sweeps as Post.ra / rt / qr in Julia layout (sweep (m, l) is trace row m * n_chain + l)."""
    Y, logT, X, init, _ = pu.make_problem(model, N, J, 3)
    op = pu.OracleProblem(model, Y, logT, X, init, qRt=0.85, cov2one=model not in ("latentqr", "latent"))
    o = op.run(n_iter * n_chain, with_nu=model in ("latentqr", "crossqr"))
    return {k: o[k].reshape(n_iter, n_chain, o[k].shape[1]).transpose(0, 2, 1) for k in ("ra", "qr") + (() if model == "mlirt" else ("rt",))}


@pytest.mark.parametrize("model,N,J,n_iter,n_burnin,n_chain", [
    ("rtirt", 300, 8, 240, 120, 2), ("crossqr", 120, 5, 240, 120, 2), ("null", 300, 8, 240, 120, 2), ("mlirt", 300, 8, 240, 120, 2),
    ("rtirt", 300, 8, 8, 0, 1), ("rtirt", 300, 8, 9, 0, 1), ("latentqr", 300, 8, 30, 13, 3), ("latentqr", 300, 8, 20, 4, 16), ("rtirt", 300, 8, 64, 0, 1),
    ("rtirt", 300, 8, 600, 300, 2), ("crossqr", 120, 5, 600, 300, 2)])
def test_sampler_traces_of_the_gpu_tests_shapes_stay_within_the_skip_cap(model, N, J, n_iter, n_burnin, n_chain):
    """Chains of the CPU oracle at the shapes tests/test_gpu_diagnostics.py runs on the device: the reference leaves out no more than one column in 1000 of a trace
    (none, in fact), the host twin agrees with it on every column, no column of a chain with n >= 60 has a non-positive ESS (the short ones do: see below), and at nIter = 600 (M n = 600) the ra trace has
    columns on both sides of the threshold ESS > 400 (270 above and 46 below for GibbsRtIrt, 79 and 51 for GibbsRtIrtCrossQr)."""
    for name, tr in _oracle_traces(model, N, J, n_iter, n_chain).items():
        x = tr[n_burnin:]
        ref = du.reference(x)
        skipped = int(np.sum(~ref["constant"] & (ref["margin"] < du.MARGIN_MIN)))
        assert skipped <= du.SKIP_CAP * x.shape[1], (name, skipped)
        ess, rhat = _twin(x)
        cmp_ = du.compare(ess, rhat, ref)
        assert cmp_["bad"].size == 0 and cmp_["skipped"] == skipped, (name, cmp_)
        # ess = M n / (-1 + 2 sum P_k) is negative whenever the pair sums add up to less than 1 / 2: -M n when the first one is not positive (an empty sum), any
        # negative value otherwise.  Chains of 4 and 8 draws per sequence have such columns (136 of GibbsRtIrt's 316 ra columns at n = 4); longer ones do not.
        neg = np.flatnonzero(ess <= 0)
        print(f"{model} {n_iter}/{n_burnin}/{n_chain} {name}: {neg.size} of {ess.size} columns with a negative ESS, {int(np.sum(ref['terms'][neg] == 0))} of them -M n")
        empty = neg[ref["terms"][neg] == 0]
        assert np.all(ess[empty] == -ref["M"] * ref["n"]) and np.all(ref["p0"][empty] <= 0) and np.all(ref["ess"][neg] < 0)
        assert neg.size == 0 or ref["n"] < 60, (name, neg)
        if n_iter == 600 and name == "ra":
            e = np.asarray(ref["ess"], dtype=np.float64)
            assert np.sum(e > 400.0 * (1 + du.ESS_RTOL)) >= 10 and np.sum(e < 400.0 * (1 - du.ESS_RTOL)) >= 10

"""The rank-normalised convergence diagnostics on the CPU: the package's host twin `rank_ess_rhat` (numpy / scipy transforms, then `ess_rhat`) against the
independent reference of tests/rank_diag_util.py (the same transforms written from the definition, then diag_util's long-double estimator), on the synthetic sets
the GPU tests use and on the edge columns of the definition; invariance under strictly increasing maps; checkConvergence's default output."""
import types

import numpy as np
import pytest

import diag_util as du
import parity_util as pu
import rank_diag_util as ru

pkg = pu.ge.load_package()
SEED = 1


def _twin(x):
    """rank_ess_rhat column by column on x[iteration, column, chain]."""
    with np.errstate(divide="ignore", invalid="ignore"):
        out = np.array([pkg.rank_ess_rhat(x[:, k, :]) for k in range(x.shape[1])], dtype=np.float64).reshape(x.shape[1], 3)
    return out[:, 0], out[:, 1], out[:, 2]


@pytest.fixture(scope="module")
def sets():
    """(n_draw, n_chain, precision) -> (x, reference(x)) for 65 columns of the synthetic generator"""
    out = {}
    for nd, nc in ru.PAIRS:
        x = ru.synthetic(nd, nc, 65, SEED)
        for prec in ("f64", "f32"):
            xp = x if prec == "f64" else x.astype(np.float32).astype(np.float64)
            out[nd, nc, prec] = (xp, ru.reference(xp))
    return out


@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("nd,nc", ru.PAIRS)
def test_host_twin_against_the_reference(sets, nd, nc, prec):
    x, ref = sets[nd, nc, prec]
    assert ref["S"] == 2 * nc * (nd // 2) and ref["k"] == -(-ref["S"] // 20)
    assert float(ref["margin"].min()) >= ru.MARGIN_MIN, "the reference alone must skip no column of the synthetic sets"
    assert ref["fold_wins"].any() and not ref["fold_wins"].all(), "both branches of the max must occur"
    res = ru.compare(*_twin(x), ref)
    print(f"{nd} x {nc} {prec}: bulk {res['bulk_err']:.2e} tail {res['tail_err']:.2e} rhat {res['rhat_err']:.2e}, skipped {res['skipped']}")
    assert res["skipped"] == 0 and res["bad"].size == 0, res


def test_constant_column_has_no_statistic():
    for v in (0.0, 1.0, 0.1, -3.7):
        x = np.full((20, 1, 2), v)
        assert all(np.isnan(t[0]) for t in _twin(x))
        ref = ru.reference(x)
        assert ref["constant"][0] and np.isnan(ref["ess_bulk"][0]) and np.isnan(ref["ess_tail"][0]) and np.isnan(ref["rhat_rank"][0])


@pytest.mark.parametrize("nd", [20, 21])
def test_two_valued_evenly_split_column_takes_rhat_of_z(nd):
    """Half of the USED draws at each value: the median lies half-way, f is constant, R(z') is undefined and rhat_rank = R(z).  (nd = 21: the middle draw is unused.)"""
    g = np.random.default_rng(5)
    x = np.empty((nd, 1, 2))
    n = nd // 2
    rows = np.r_[0:n, nd - n:nd]
    vals = np.where(g.permutation(4 * n) % 2 == 0, 1.5, -0.5).reshape(2 * n, 2)
    x[:, 0, :] = 99.0
    x[rows, 0, :] = vals
    ref = ru.reference(x)
    assert np.isnan(ref["rf"][0]) and not np.isnan(ref["rz"][0]) and ref["rhat_rank"][0] == ref["rz"][0]
    b, t, r = _twin(x)
    assert abs(r[0] - float(ref["rz"][0])) <= ru.RHAT_ATOL and not np.isnan(b[0])
    assert ru.compare(b, t, r, ref)["bad"].size == 0


def test_all_ties_but_one():
    """S - 1 equal draws and one larger: with k >= 2 the upper order statistic is the common value, U is constant and the tail ESS undefined, the others defined."""
    x = np.full((20, 1, 2), 3.0)
    x[1, 0, 0] = 7.0
    ref = ru.reference(x)
    assert ref["k"] == 2 and np.isnan(ref["ess_tail"][0]) and not np.isnan(ref["ess_bulk"][0]) and not np.isnan(ref["rhat_rank"][0])
    assert ru.compare(*_twin(x), ref)["bad"].size == 0
    x8 = np.full((8, 1, 1), 3.0)                      # S = 8: k = 1, both indicators mark single draws or all but one
    x8[2, 0, 0] = 7.0
    ref8 = ru.reference(x8)
    assert ref8["k"] == 1 and not np.isnan(ref8["ess_tail"][0])
    assert ru.compare(*_twin(x8), ref8)["bad"].size == 0


def test_odd_length_drops_the_middle_draw():
    g = np.random.default_rng(11)
    x = g.standard_normal((17, 5, 2))
    y = x.copy()
    y[8] = 1e6 * g.standard_normal((5, 2))             # the unused draw
    a, b = _twin(x), _twin(y)
    assert all(np.array_equal(u, v) for u, v in zip(a, b))
    assert ru.compare(*a, ru.reference(x))["bad"].size == 0


def test_s_equals_eight():
    g = np.random.default_rng(12)
    x = g.standard_normal((8, 40, 1))
    ref = ru.reference(x)
    assert ref["S"] == 8 and ref["k"] == 1
    res = ru.compare(*_twin(x), ref)
    assert res["bad"].size == 0 and res["skipped"] <= 1


def test_strictly_increasing_maps_keep_bulk_and_tail_bit_for_bit():
    """The ranks and the two indicator columns depend on the order of the draws only: x, 2 x and x^3 + 10 (checked here to keep order and ties) give identical
    bulk and tail ESS.  (The folded series is not invariant under a non-linear map, so R-hat is compared for 2 x only.)"""
    x = ru.synthetic(64, 2, 30, SEED)
    base = _twin(x)
    for name, y in (("2x", 2.0 * x), ("cube", x ** 3 + 10.0)):
        flat, fy = ru.used(x).transpose(0, 2, 1).reshape(-1, 30), ru.used(y).transpose(0, 2, 1).reshape(-1, 30)
        from scipy.stats import rankdata
        assert np.array_equal(rankdata(flat, method="average", axis=0), rankdata(fy, method="average", axis=0)), name
        got = _twin(y)
        assert np.array_equal(base[0], got[0]) and np.array_equal(base[1], got[1], equal_nan=True), name
        if name == "2x":
            assert np.array_equal(base[2], got[2])


class _FakeEngine:
    def diagnostics(self, which):
        return np.array([500.0, 300.0, np.nan]), np.array([1.01, 1.2, np.nan])

    def convergence(self, which):
        return (2, 1, 2, 1)


def test_check_convergence_default_output_is_unchanged():
    mc = types.SimpleNamespace(_engine=_FakeEngine(), _traits=types.SimpleNamespace(rt=True))
    want = dict(ess=50.0, rhat=50.0, essN="3 / 6", rhatN="3 / 6")
    for kw in ({}, {"kind": "basic"}):
        res = pkg.checkConvergence(mc, detail=False, **kw)
        assert res == want and list(res) == ["ess", "rhat", "essN", "rhatN"]
        res = pkg.checkConvergence(mc, detail=True, **kw)
        assert list(res) == ["ess", "rhat", "essN", "rhatN", "detail"] and sorted(res["detail"]) == ["qr", "ra", "rt"]
        assert {k: res[k] for k in want} == want
    with pytest.raises(ValueError):
        pkg.checkConvergence(mc, kind="ranked")

"""The preconditions of tests/test_gpu_item_pass_limits.py, checked on the CPU with the numpy twins alone, so that no GPU case can pass or fail on an
input that two correct implementations may answer differently.  For every case of item_pass_util's WIDE_CASES (896 items and the two sides of the 64 KB line of
dynamic LDS), MASKED_CASES (obs_util's patterns at 896 items) and the engine cases (the oracle's chain standing for the fp64 engine's), nothing left out:
  - every twin S lies at least S_MARGIN = 0.1 from MARG_COARSE_S = 2: the coarse flags and nCoarse are decidable.  Measured at Q = 255, the smallest distance:
    complete 0.286 (cross, 896 items), masked 0.294 (cross), LatentQr 0.789; on the oracle's chain 1.11 (cross) or more;
  - every plausible-value draw has its two best keys at least pv_util.GAP_MIN = 1e-8 apart: the nodes are decidable.  Measured at K = 5: 1.55e-4 (cross, 585
    items) or more;
  - every value of every twin product is finite.
The node-count and fourteen-covariate cases (J = 9) are held to the same conditions in one test: S at least 4.8, the smallest gap 2.75e-4.
The default of 61 nodes is too coarse for a long form: at 586, 683 and 896 items it flags every one of the 40 subjects (S between 1 and 2), which
test_default_node_count_is_coarse_for_a_long_form holds as the figure INTEGRATION.md quotes.  The LDS straddle is computed, and pinned here against the literal
item counts of this tree's layout so that a change of layout is seen."""
import numpy as np
import pytest

import item_pass_util as ip
import marginal_util as mu
import pv_util as pvu

pkg = ip._pkg()
CASES = ip.WIDE_CASES + ip.MASKED_CASES


@pytest.fixture(scope="module", autouse=True)
def twins():
    ip.warm_twins(CASES)


def _finite(o, cols):
    return all(np.all(np.isfinite(np.asarray(getattr(o, c), dtype=np.float64))) for c in cols)


def _assert_decidable(p, get, what):
    """The three conditions for the products the model of p has; get(product) is the product's twin."""
    rt = p.model != "mlirt"
    cols = ("theta", "thetaSd", "rowEss") + (("zeta", "zetaSd", "cov") if rt else ())
    for product in ip.products(p.model):
        if product in ("loglik", "qloglik"):
            l, S = get(product)
            print(f"{what} {product}: S in [{S.min():.4g}, {S.max():.4g}], margin {ip.coarse_margin(S):.3g}; l in [{l.min():.5g}, {l.max():.5g}]")
            assert l.shape == (p.rows.shape[0], p.Y.shape[0]) and np.all(np.isfinite(l)) and np.all(np.isfinite(S))
            assert ip.coarse_margin(S) >= ip.S_MARGIN
        elif product == "score":
            for w in ("equal", "likelihood"):
                sc = get(f"score.{w}")
                assert _finite(sc, cols), (what, w)
        else:
            pv, gap = get("pv")
            print(f"{what} pv: smallest gap {gap.min():.3g}")
            assert gap.shape == (p.Y.shape[0], p.K) and gap.min() >= pvu.GAP_MIN
            assert _finite(pv, ("theta",) + (("zeta",) if rt else ()))


def test_lds_straddle_is_computed_and_stands_on_both_sides_of_the_line():
    assert ip.lds_straddle("cross", 3) == (584, 585) and ip.lds_straddle("rtirt", 3) == (680, 681)      # this tree's layout: ld = 5 J + 4 and 4 J + 12
    for model in ("cross", "rtirt"):
        lo, hi = ip.lds_straddle(model, 3)
        assert ip.marg_lds_bytes(model, lo, 3) <= ip.LDS_LINE < ip.marg_lds_bytes(model, hi, 3)
        assert ("wide", model, lo) in ip.WIDE_CASES and ("wide", model, hi) in ip.WIDE_CASES
    assert ip.marg_lds_bytes("cross", ip.J_MAX, 3) == 2 * (5 * 896 + 4 + 2 * 896) * 8 == 100416
    assert ip.marg_lds_bytes("mlirt", 9, 3) == 16 * (4 * 9 + 4 + 18) and ip.marg_lds_bytes("latentqr", 9, 14) == ip.marg_lds_bytes("latent", 9, 14)
    assert [m for _, m, J in ip.WIDE_CASES if J == ip.J_MAX] == mu.MODELS + ["latentqr"]


@pytest.mark.parametrize("case", CASES, ids=ip.case_id)
def test_case_is_decidable(case):
    p = ip.problem(case)
    if case[0] == "masked":
        n = p.obs.sum(axis=1)
        assert {0, 1, ip.J_MAX - 8, ip.J_MAX // 2, ip.J_MAX} <= set(n[:6]) and p.Y.shape == (ip.MASKED_N, ip.J_MAX)
    else:
        assert p.Y.shape == (ip.WIDE_N, case[2]) and p.obs is None
    assert p.rows.shape[0] == ip.ROWS and p.Q == ip.WIDE_Q
    _assert_decidable(p, lambda product: ip.twin(case, product), ip.case_id(case))


def test_small_cases_are_decidable():
    """The node-count and fourteen-covariate cases (J = 9): cheap, so all of them in one test.  Measured: S at least 4.8, the smallest gap 2.75e-4."""
    worst_S, worst_gap = np.inf, np.inf
    for case in ip.NODE_CASES + ip.FEAT_CASES:
        p = ip.problem(case)
        assert p.Y.shape == (ip.SMALL_N, ip.SMALL_J) and (p.X is None or p.X.shape[1] == (ip.F_MAX if case[0] == "feat" else 3))
        l, S = ip.twin(case, ip.products(case[1])[0])
        assert np.all(np.isfinite(l)) and ip.coarse_margin(S) >= ip.S_MARGIN, case
        worst_S = min(worst_S, S.min())
        if case[1] != "latentqr" and (case[0] == "feat" or case[1] in ("rtirt", "cross")):
            pv, gap = ip.twin(case, "pv")
            assert gap.min() >= pvu.GAP_MIN and np.all(np.isfinite(pv.theta)), case
            worst_gap = min(worst_gap, gap.min())
    print(f"J = 9 cases: S at least {worst_S:.3g}, smallest gap {worst_gap:.3g}")


@pytest.mark.parametrize("model", ip.ENGINE_MODELS)
def test_engine_case_is_decidable_on_the_oracles_chain(model):
    p = ip.oracle_problem(model, ip.ENGINE_SWEEPS, ip.ENGINE_BURNIN)
    assert p.rows.shape == (ip.ENGINE_SWEEPS - ip.ENGINE_BURNIN, pkg._lib.item_trace_width(p.code, ip.J_MAX, 3)) and p.Y.shape == (ip.ENGINE_N, ip.J_MAX)
    got = ip.twins_of(p, [k for _, k in ip.twin_keys([("engine", model)])])
    _assert_decidable(p, got.__getitem__, f"engine {model}")


def test_loo_case_is_decidable_on_the_oracles_chain():
    p = ip.oracle_problem("rtirt", ip.LOO_SWEEPS, ip.LOO_BURNIN)
    l, S = ip.twin_loglik_by_rows(p)
    print(f"LOO rtirt: {l.shape[0]} rows, S in [{S.min():.4g}, {S.max():.4g}], margin {ip.coarse_margin(S):.3g}")
    assert l.shape == (25, ip.ENGINE_N) and np.all(np.isfinite(l)) and ip.coarse_margin(S) >= ip.S_MARGIN
    loo = pkg.psisLooHost(l)
    assert np.isfinite(loo.elpd) and not np.any(np.isnan(loo.khat))


@pytest.mark.parametrize("model,J", [("cross", 586), ("rtirt", 683), ("mlirt", 683), ("rtirt", 896)])
def test_default_node_count_is_coarse_for_a_long_form(model, J):
    """marginal_util's rows and data, N = 40, 2 rows, seed 7.  At the default Q = 61 every S lies between 1 and 2 (GibbsMlIrt at 683 items has one subject at 2.0004
    in both rows: a flag that two implementations may set differently, which is why no GPU case runs a long form at 61 nodes), so at least 39 of the 40 subjects
    are flagged; Q = 255 flags none, with S at least 2.65.  Measured: cross 586 [1.0008, 1.9565] and 2.6592; rtirt 683 [1.0700, 1.9953] and 4.0736; mlirt 683
    [1.0258, 2.0004] and 3.5962; rtirt 896 [1.0122, 1.9565] and 3.2925."""
    rows = mu.make_rows(model, J, 3, 2, seed=7)
    Y, logT, X = mu.make_data(model, 40, J, 3, seed=7)
    S = {Q: pkg.marginalLogLikHost(mu.CODE[model], Y, logT, ip._kernel_x(model, X), rows, Q, with_S=True)[1] for Q in (61, 255)}
    flagged = int(np.sum(np.any(S[61] < ip.COARSE_S, axis=0)))
    print(f"{model} J={J}: Q=61 S in [{S[61].min():.4f}, {S[61].max():.4f}], {flagged} of 40 flagged; Q=255 S >= {S[255].min():.4f}")
    assert S[61].min() >= 1.0 and S[61].max() <= ip.COARSE_S + 1e-3 and flagged >= 39
    assert np.all(S[255] >= ip.COARSE_S + ip.S_MARGIN)

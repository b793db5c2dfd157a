"""The item-trace passes at the limits their entries accept: 896 items, 1025 nodes, 14 covariates.  marginal_kernel, score_kernel, pv_kernel,
their MASKED instantiations and marginal_kernel<LATENTQR> against the numpy twins, at the cases of item_pass_util's table, whose inputs
tests/test_item_pass_limits_host.py has shown decidable on the CPU (every twin S at least 0.1 from MARG_COARSE_S, every draw's two best keys 1e-8 apart).
  a. wide items: N = 40, 3 rows, F = 3, Q = 255 (the default of 61 nodes flags every subject of a form this long).  896 items for the five Gaussian models and
     LatentQr, and for Cross and RtIrt the two item counts of lds_straddle -- (584, 585) and (680, 681) -- between which a launch's dynamic LDS crosses 64 KB, the
     size above which marg_tile_launch's attribute is meant to matter (see the end of this text); each case asserts its own LDS size.  Every product the model has.
  b. the masked entries at 896 items: obs_util's patterns (n_i = 896, 0, 1, 888, 448, about 448 in one wave), N = 33, rtirt, cross and mlirt, against the masked
     twins; a mask of all ones and poisoned unobserved cells bit for bit; every pattern subject against the same subject in the data set of its observed items
     alone (1, 448 and 888 items: launches on both sides of the 64 KB line), bit for bit.
  c. independence at 896 items: subjects 5 and 39 of the 40 alone give the bits they give among the others (the draws at the same index).
  d. node counts at J = 9, N = 37: Q = 63, 65, 513, 1025; the refusals of 1027, 1026, 2 and 1 by every caller-data entry, 1025 accepted.
  e. 14 covariates on the entries tests/test_gpu_covariate_width.py has no case for: score, plausible values, the masked entries, LatentQr; F = 15 refused.
  f. engine-resident data at 896 items: 70 subjects, fp64 and fp32 engines, 6 sweeps with 2 burn-in, against the caller-data entries on erm_get_data's data set and
     the post-burn-in rows of erm_get_item_trace with the helpers and bounds of the engine-entry tests; the chain, the traces and the state unchanged; one
     PSIS-LOO case of 25 rows.  The fp32 chain is not the oracle's, but its flags are compared between two launches of the same kernel family on the same rows and,
     up to the rounding of logT + cm, the same data: a flag could differ only for an S within 1e-12 of 2, and on the oracle's chain no S is below 3.1.
Bounds.  Every quantity under the existing 1e-10, in the form the product's own test uses (relative to |ref| for l, p_i and the totals, with LPPD_FLOOR for
lppd_i; relative to max(|ref|, 1) for the score columns, the draws and every masked product); counts, flags and nodes exactly.  p_i and the likelihood-weighted
score columns are functions of differences of l across rows; their measured errors stay under 1e-10 as well (below), so they keep it and no propagated bound is
needed.
Measured on an MI355X (the worst over the cases of a section; pytest -s prints every figure).  |l| reaches 2 159 and a subject's rows lie up to 143 apart:
  a. l 1.5e-15, lppd_i 3.7e-16, p_i 6.5e-13, totals 1.2e-14 (se); LatentQr l 6.6e-16, p_i 1.5e-13; score columns 2.4e-14 under equal and 3.6e-14 under likelihood
     weights, row_ess 2.2e-13; draws 2.3e-15, every node equal.  No figure differs between the two sides of the 64 KB line.
  b. l 1.1e-15, lppd_i 6.3e-16, p_i 2.2e-13; score columns 1.5e-14 / 3.7e-14, row_ess 7.1e-14; draws 2.1e-15; all ones, poison and the reduced subjects
     (896, 1, 888, 448 and 438 items): every bit.
  d. l 6.1e-16, p_i 1.8e-14; score columns 2.0e-15, row_ess 3.2e-15; draws 6.9e-16.            e. l 8.9e-16, p_i 8.2e-15; score columns 1.5e-15, row_ess 2.5e-15; draws 1.5e-15.
  f. the engine entries equal the caller-data entries in every bit of lppd_i, p_i, the totals, the score columns and the draws, fp64 and fp32; the draws against
     the twin 1.3e-14; PSIS-LOO over 25 rows: k-hat 1.05e-10, n_eff 1.5e-10, elpd_i 4.0e-13 against the bound 2.48e-10 (59 of the 70 k-hat exceed 0.7: four and
     twenty-five rows of an 896-item chain that has not converged are an ill-conditioned input, which is what the bound of tests/test_gpu_psis_loo.py measures).
What the straddle cases do and do not pin (tried on a scratch build, nothing of it committed): an item-sum loop bound of J - 1 fails all of a. and d. (85 of the
111 tests); a node-loop guard of qq <= Q fails d. at Q = 63 with b., e. and f. (26); MARG_MAXF lowered to 13 fails e. (17).  Taking the
hipFuncSetAttribute(MaxDynamicSharedMemorySize) call out of marg_tile_launch fails NOTHING: the HIP runtime of ROCm on gfx950 launched 66 KB to 98 KB of dynamic
LDS without it, with the same bits.  The cases therefore pin that launches above 64 KB work and compute the same values, not that the attribute call is there."""
import numpy as np
import pytest

import item_pass_util as ip
import marginal_util as mu
import obs_util as ou
import psis_util as ps
import pv_util as pvu
import score_util as su
from item_pass_util import _bytes, _engine, _pkg

pytestmark = pytest.mark.gpu

TOL = 1e-10
LPPD_FLOOR = 1e-3
TOTALS = ("elpd", "pWaic", "WAIC", "se", "lppd")
WEIGHTINGS = ("equal", "likelihood")
SCORE_KEYS = su.COLS + ("coarse",)
PV_KEYS = ("theta", "zeta", "node", "coarse")
ERM_ERR_ARG = -1


@pytest.fixture(scope="module", autouse=True)
def twins():
    ip.warm_twins(ip.WIDE_CASES + ip.MASKED_CASES)


def _code(e):
    return int(str(e.value).split()[2].rstrip(":"))


# ------------------------------------------------------------------------------------------------------------ a product against its twin
def _device(p, product, **kw):
    L = _pkg()._lib
    obs = {} if p.obs is None else dict(obs=p.obs)
    if product == "loglik":
        return L.marginal_loglik(p.code, *p.data, p.rows, nodes=p.Q, **obs)
    if product == "qloglik":
        return L.quantile_marginal_loglik(p.code, *p.data, p.rows, ip.Q_RT, nodes=p.Q)
    if product.startswith("score."):
        return L.score(p.code, *p.data, p.rows, nodes=p.Q, weighting=product[6:], **obs)
    return L.plausible_values(p.code, *p.data, p.rows, K=p.K, seed=p.seed, nodes=p.Q, **obs)


def _check_loglik(p, dev, ref, what):
    """tests/test_gpu_marginal_waic.py's _assert_equals_twin (LatentQr: tests/test_gpu_quantile_marginal.py's) on a twin computed once; a masked case in the form of
    tests/test_gpu_incomplete.py, relative to max(|ref|, 1) -- a subject without cells has l = -1.7e-9."""
    Lh, S = ref
    host = _pkg().twins.waicFromLogLik(Lh)
    t = dev["totals"]
    if p.obs is None:
        err = dict(l=np.max(np.abs(dev["l"].T - Lh) / np.abs(Lh)), lppd=np.max(np.abs(dev["lppd"] - host.lppd_u) / np.maximum(np.abs(host.lppd_u), LPPD_FLOOR)),
                   p=np.max(np.abs(dev["p"] - host.p_u) / np.abs(host.p_u)))
        err.update({k: abs(t[k] - getattr(host, k)) / abs(getattr(host, k)) for k in TOTALS})
    else:
        err = dict(l=ou.rel(dev["l"], Lh.T), lppd=ou.rel(dev["lppd"], host.lppd_u), p=ou.rel(dev["p"], host.p_u), elpd=ou.rel([t["elpd"]], [host.elpd]))
        assert np.array_equal(dev["nObs"], p.obs.sum(axis=1)) and dev["nObs"].dtype == np.int32
    print(f"{what}: " + ", ".join(f"{k} {v:.3g}" for k, v in err.items()) + f"; l in [{Lh.min():.5g}, {Lh.max():.5g}], largest spread of a subject's rows "
          f"{np.max(Lh.max(axis=0) - Lh.min(axis=0)):.4g}; coarse {t['nCoarse']}")
    assert np.all(np.isfinite(dev["l"])) and all(v <= TOL for v in err.values()), err
    assert (t["nUnits"], t["nRows"], t["nNodes"], t["nHighVar"]) == (p.Y.shape[0], p.rows.shape[0], p.Q, host.nHighVar)
    assert t["nCoarse"] == int(np.sum(np.any(S < ip.COARSE_S, axis=0)))
    return err


def _check_score(p, dev, host, weighting, what):
    """tests/test_gpu_scores.py's _assert_equals_twin: every column relative to max(|ref|, 1); the flags, row_ess under equal weights and out4 exactly."""
    rt = p.model != "mlirt"
    err = {}
    for c in su.COLS:
        d, r = np.asarray(dev[c], dtype=np.float64), np.asarray(getattr(host, c), dtype=np.float64)
        if not rt and c in ("zeta", "zetaSd", "cov"):
            assert np.all(np.isnan(d)) and np.all(np.isnan(r)), c
            continue
        assert np.all(np.isfinite(d)), c
        err[f"{weighting[0]}.{c}"] = float(np.max(np.abs(d - r) / np.maximum(np.abs(r), 1.0)))
    print(f"{what} {weighting}: " + ", ".join(f"{c} {e:.3g}" for c, e in err.items()) + f"; smallest rowEss {np.min(host.rowEss):.4g}, coarse {dev['nCoarse']}")
    assert all(e <= TOL for e in err.values()), err
    assert np.array_equal(dev["coarse"], host.coarse) and dev["nCoarse"] == host.nCoarse == int(np.sum(dev["coarse"]))
    assert (dev["nSubj"], dev["nRows"], dev["nNodes"]) == (p.Y.shape[0], p.rows.shape[0], p.Q)
    if weighting == "equal":
        assert np.all(dev["rowEss"] == p.rows.shape[0])
    if p.obs is not None:
        assert np.array_equal(dev["nObs"], p.obs.sum(axis=1))
    return err


def _check_pv(p, dev, ref, what):
    """tests/test_gpu_plausible_values.py's test_plausible_values_equal_twin: equal nodes and flags, theta and zeta relative to max(|ref|, 1)."""
    host, gap = ref
    assert gap.min() >= pvu.GAP_MIN                                                       # the condition on the inputs: every draw is decidable
    assert np.array_equal(dev["node"], host.node) and np.array_equal(dev["coarse"], host.coarse), what
    err = dict(theta=ou.rel(dev["theta"], host.theta), zeta=ou.rel(dev["zeta"], host.zeta))
    print(f"{what}: theta {err['theta']:.3g}, zeta {err['zeta']:.3g}; smallest gap {gap.min():.3g}, coarse {dev['nCoarse']}")
    assert all(e <= TOL for e in err.values()) and np.all(np.isfinite(dev["theta"])), err
    assert (dev["nSubj"], dev["nRows"], dev["nNodes"], dev["nCoarse"], dev["seed"]) == (p.Y.shape[0], p.rows.shape[0], p.Q, host.nCoarse, p.seed)
    assert dev["nCoarse"] == int(np.sum(dev["coarse"])) and dev["node"].dtype == np.int32 and dev["node"].min() >= 0 and dev["node"].max() < p.Q
    if p.obs is not None:
        assert np.array_equal(dev["nObs"], p.obs.sum(axis=1))
    return err


def _check(case, product):
    """One product of a case against its twin: the errors by quantity."""
    p, what = ip.problem(case), f"{ip.case_id(case)} {product}"
    if product in ("loglik", "qloglik"):
        return _check_loglik(p, _device(p, product), ip.twin(case, product), what)
    if product == "pv":
        return _check_pv(p, _device(p, "pv"), ip.twin(case, "pv"), what)
    err = {}
    for w in WEIGHTINGS:
        err.update(_check_score(p, _device(p, f"score.{w}"), ip.twin(case, f"score.{w}"), w, what))
    return err


def _ids(pairs):
    return [f"{ip.case_id(c)}-{pr}" for c, pr in pairs]


def _with_products(cases, only=None):
    return [(c, pr) for c in cases for pr in ip.products(c[1]) if only is None or only(c, pr)]


# ------------------------------------------------------------------------------------------------------------ a. wide items
WIDE = _with_products(ip.WIDE_CASES)


@pytest.mark.parametrize("case,product", WIDE, ids=_ids(WIDE))
def test_wide_items_equal_twin(case, product):
    _, model, J = case
    if J != ip.J_MAX:                                                                      # a straddle case says on which side of the line it stands
        lo, hi = ip.lds_straddle(model, 3)
        assert J in (lo, hi) and ip.marg_lds_bytes(model, lo, 3) <= ip.LDS_LINE < ip.marg_lds_bytes(model, hi, 3)
    elif model in ("cross", "rtirt"):
        assert ip.marg_lds_bytes(model, J, 3) > ip.LDS_LINE
    p = ip.problem(case)
    assert p.Y.shape == (ip.WIDE_N, J) and p.rows.shape[0] == ip.ROWS and p.Q == ip.WIDE_Q
    _check(case, product)


# ------------------------------------------------------------------------------------------------------------ b. the masked entries at 896 items
MASKED = _with_products(ip.MASKED_CASES)


@pytest.mark.parametrize("case,product", MASKED, ids=_ids(MASKED))
def test_masked_entries_equal_twin_at_896_items(case, product):
    p = ip.problem(case)
    n = p.obs.sum(axis=1)
    assert {0, 1, ip.J_MAX - 8, ip.J_MAX // 2, ip.J_MAX} <= set(n[:6]) and n.max() - 1 == ip.J_MAX - 1      # the uint16 index runs up to 895
    _check(case, product)


def _products(p, Y=None, logT=None, obs=None, sl=None):
    """The three products as one dict of arrays (tests/test_gpu_incomplete.py's _products): l, the score columns under both weightings, the draws."""
    L = _pkg()._lib
    Y, logT = p.Y if Y is None else Y, p.logT if logT is None else logT
    cut = lambda a: None if a is None else a if sl is None else a[sl]
    Y, logT, X, obs = cut(Y), None if p.logT is None else cut(logT), cut(p.X), cut(obs)
    out = {"l": L.marginal_loglik(p.code, Y, logT, X, p.rows, nodes=p.Q, want_waic=False, obs=obs)["l"]}
    for w in WEIGHTINGS:
        sc = L.score(p.code, Y, logT, X, p.rows, nodes=p.Q, weighting=w, obs=obs)
        out.update({f"{w}.{c}": sc[c] for c in SCORE_KEYS})
    pv = L.plausible_values(p.code, Y, logT, X, p.rows, K=p.K, seed=p.seed, nodes=p.Q, obs=obs)
    out.update({f"pv.{c}": pv[c] for c in PV_KEYS})
    return out


def _worst_difference(got, ref, what):
    """Prints the worst relative difference of two results and the keys that differ, then asserts that every bit is equal."""
    worst, differing = 0.0, []
    for k in ref:
        g, r = np.asarray(got[k]), np.asarray(ref[k])
        if not np.array_equal(g, r, equal_nan=True):
            differing.append(k)
        if g.dtype.kind == "f":
            worst = max(worst, ou.rel(g, r))
    print(f"{what}: worst relative difference {worst:.3g}; differing {differing[:8]}")
    assert not differing and worst == 0.0


@pytest.mark.parametrize("case", ip.MASKED_CASES, ids=ip.case_id)
def test_mask_of_all_ones_is_the_unmasked_entry_bit_for_bit_at_896_items(case):
    p = ip.problem(case)
    _worst_difference(_products(p, obs=np.ones_like(p.Y)), _products(p), f"{ip.case_id(case)} all ones against unmasked")


@pytest.mark.parametrize("case", ip.MASKED_CASES, ids=ip.case_id)
def test_unobserved_cells_are_never_read_at_896_items(case):
    p = ip.problem(case)
    Yp, lp = ou.poison(p.Y, p.logT, p.obs)
    assert np.any(Yp == 255) and (lp is None or np.any(np.isnan(lp)))
    _worst_difference(_products(p, Y=Yp, logT=lp, obs=p.obs), _products(p, obs=p.obs), f"{ip.case_id(case)} poisoned against clean")


@pytest.mark.parametrize("model", ["rtirt", "cross"])
def test_pattern_subject_equals_the_reduced_subject_bit_for_bit_at_896_items(model):
    """One subject per pattern (N = 6).  The reduced data sets have 896, 1, 888, 448 and about 448 items: the launches of the two sides ask for 98 KB of LDS against
    as little as 176 bytes, and every floating-point operation stands in the same order in both."""
    p = ip.problem(("masked", model))
    six = slice(0, 6)
    got = _products(p, obs=p.obs, sl=six)
    L = _pkg()._lib
    worst, differing, sizes = 0.0, [], []
    for i in range(6):
        red = ou.reduced_subject(model, p.Y[six], p.logT[six], None if p.X is None else p.X[six], p.rows, p.obs[six], i)
        if red is None:
            continue
        Yr, lr, Xr, rr = red
        sizes.append(Yr.shape[1])
        tile = lambda a: None if a is None else np.repeat(a, i + 1, axis=0)                # the subject at index i of the reduced data set as well: the draws' counter
        q = ip.Problem(model=model, code=p.code, Y=tile(Yr), logT=tile(lr), X=tile(Xr), rows=rr, obs=None, Q=p.Q, K=p.K, seed=p.seed)
        ref = _products(q)
        for k in ref:
            g, r = np.asarray(got[k])[i], np.asarray(ref[k])[i]
            if not np.array_equal(g, r, equal_nan=True):
                differing.append((i, k))
            if np.asarray(g).dtype.kind == "f":
                worst = max(worst, ou.rel(g, r))
    print(f"{model}: reduced data sets of {sizes} items; worst relative difference from the reduced subject {worst:.3g}; differing {differing[:8]}")
    assert sizes[:4] == [ip.J_MAX, 1, ip.J_MAX - 8, ip.J_MAX // 2] and len(sizes) == 5
    assert ip.marg_lds_bytes(model, 1, 3) < ip.LDS_LINE < ip.marg_lds_bytes(model, ip.J_MAX - 8, 3) and ip.marg_lds_bytes(model, ip.J_MAX // 2, 3) < ip.LDS_LINE
    assert not differing and worst == 0.0


# ------------------------------------------------------------------------------------------------------------ c. independence at 896 items
def test_a_subjects_result_depends_on_its_own_data_only_at_896_items():
    p = ip.problem(("wide", "rtirt", ip.J_MAX))
    whole = _products(p)
    keys_ls = [k for k in whole if not k.startswith("pv.")]
    for i in (5, 39):                                                                      # a subject of the full tile, and the last of the part tile
        alone = _products(p, sl=slice(i, i + 1))
        for k in keys_ls:
            assert np.all(np.isfinite(alone[k])) and np.array_equal(alone[k][0], whole[k][i]), (i, k)
        idx = np.full(i + 1, i)                                                            # the same subject at the same index: the draws' counter
        tiled = _products(p, sl=idx)
        for k in whole:
            assert np.array_equal(np.asarray(tiled[k])[i], np.asarray(whole[k])[i], equal_nan=True), (i, k)


# ------------------------------------------------------------------------------------------------------------ d. node counts
NODES = _with_products(ip.NODE_CASES, only=lambda c, pr: pr in ("loglik", "qloglik") or c[1] in ("rtirt", "cross"))


@pytest.mark.parametrize("case,product", NODES, ids=_ids(NODES))
def test_node_counts_equal_twin(case, product):
    l, S = ip.twin(case, ip.products(case[1])[0])
    assert ip.coarse_margin(S) >= ip.S_MARGIN                                              # the flags are decidable
    _check(case, product)


def test_node_count_refusals_of_every_caller_data_entry():
    """1027, 1026, 2 and 1 nodes return ERM_ERR_ARG with the message of marg_nodes; 1025 is accepted; the device runs on."""
    L = _pkg()._lib
    lib = L.load()
    err = lambda: lib.erm_last_error().decode()
    N, J, R, K = 5, ip.SMALL_J, 3, 5
    ptr = lambda a: a.ctypes.data
    l, out10, lppd, pp = np.empty((N, R), order="F"), np.empty(10), np.empty(N), np.empty(N)
    sc, o4, n_obs = np.empty((7, N)), np.empty(4), np.empty(N, dtype=np.int32)
    pv, node, coarse = np.empty((2, K, N)), np.empty((K, N), dtype=np.int32), np.empty(N, dtype=np.int32)
    Y, logT, X, rows, obs = ou.problem("rtirt", N, J, R, seed=800)
    arrays, dims = L._caller_data(1, Y, logT, X, rows)
    O, _ = L._caller_obs(obs, N, J)
    head, mhead = L._caller_head(0, 1, arrays, dims), L._caller_head(0, 1, arrays, dims, O)
    rq = ip.qu.make_rows(J, 3, R, seed=800)
    qarrays, qdims = L._caller_data(ip.qu.CODE, Y, logT, X, rq)
    qhead = L._caller_head(0, ip.qu.CODE, qarrays, qdims)
    entries = {
        "erm_marginal_loglik": lambda Q: lib.erm_marginal_loglik(*head, Q, ptr(l), ptr(out10), ptr(lppd), ptr(pp)),
        "erm_score": lambda Q: lib.erm_score(*head, Q, 0, ptr(sc), ptr(o4)),
        "erm_plausible_values": lambda Q: lib.erm_plausible_values(*head, Q, K, 11, ptr(pv), ptr(node), ptr(coarse), ptr(o4)),
        "erm_marginal_loglik_masked": lambda Q: lib.erm_marginal_loglik_masked(*mhead, Q, ptr(l), ptr(out10), ptr(lppd), ptr(pp), ptr(n_obs)),
        "erm_score_masked": lambda Q: lib.erm_score_masked(*mhead, Q, 1, ptr(sc), ptr(o4), ptr(n_obs)),
        "erm_plausible_values_masked": lambda Q: lib.erm_plausible_values_masked(*mhead, Q, K, 11, ptr(pv), ptr(node), ptr(coarse), ptr(o4), ptr(n_obs)),
        "erm_quantile_marginal_loglik": lambda Q: lib.erm_quantile_marginal_loglik(*qhead, ip.Q_RT, Q, ptr(l), ptr(out10), ptr(lppd), ptr(pp)),
    }
    for name, call in entries.items():
        for bad in (1027, 1026, 2, 1):
            assert call(bad) == ERM_ERR_ARG and "odd and in 3 .. 1025" in err(), (name, bad)
        l[:], sc[:], pv[:] = np.nan, np.nan, np.nan
        assert call(ip.Q_MAX) == 0, (name, err())                                          # the limit itself is accepted, and the device runs on
        got = l if "loglik" in name else sc[:2] if "score" in name else pv
        assert np.all(np.isfinite(got)), name
        assert (out10[8] if "loglik" in name else o4[2]) == ip.Q_MAX, name


# ------------------------------------------------------------------------------------------------------------ e. fourteen covariates
FEAT = _with_products(ip.FEAT_CASES, only=lambda c, pr: pr != "loglik" or c[2])            # (the complete erm_marginal_loglik: tests/test_gpu_covariate_width.py)


@pytest.mark.parametrize("case,product", FEAT, ids=_ids(FEAT))
def test_fourteen_covariates_equal_twin(case, product):
    p = ip.problem(case)
    assert p.X.shape == (ip.SMALL_N, ip.F_MAX) and (p.obs is not None) == case[2]
    _check(case, product)


def test_fifteen_covariates_are_refused():
    L = _pkg()._lib
    N, J, R, F = 5, ip.SMALL_J, 3, ip.F_MAX + 1
    for model in ip.X_MODELS:
        Y, logT, X, rows, obs = ou.problem(model, N, J, R, seed=801, F=F)
        calls = [lambda: L.score(mu.CODE[model], Y, logT, X, rows), lambda: L.score(mu.CODE[model], Y, logT, X, rows, weighting="likelihood"),
                 lambda: L.plausible_values(mu.CODE[model], Y, logT, X, rows), lambda: L.marginal_loglik(mu.CODE[model], Y, logT, X, rows, obs=obs),
                 lambda: L.score(mu.CODE[model], Y, logT, X, rows, obs=obs), lambda: L.plausible_values(mu.CODE[model], Y, logT, X, rows, obs=obs)]
        for k, call in enumerate(calls):
            with pytest.raises(L.ErmError, match=r"n_feat \(0 \.\. 14\) out of range") as e:
                call()
            assert _code(e) == ERM_ERR_ARG, (model, k)
    rows = ip.qu.make_rows(J, F, R, seed=801)
    Y, logT, X = ip.qu.make_data(N, J, F, seed=801)
    with pytest.raises(L.ErmError, match=r"n_feat \(0 \.\. 14\) out of range") as e:
        L.quantile_marginal_loglik(ip.qu.CODE, Y, logT, X, rows, ip.Q_RT)
    assert _code(e) == ERM_ERR_ARG
    ok = ip.problem(("feat", "rtirt", False))
    assert np.all(np.isfinite(_device(ok, "score.equal")["theta"]))                        # and the device runs on


# ------------------------------------------------------------------------------------------------------------ f. engine-resident data at 896 items
def _everything(eng):
    L = _pkg()._lib
    parts = [eng.item_trace(), eng.trace(L.TRACE_LOGLIKE), eng.trace(L.TRACE_RA), eng.trace(L.TRACE_RT), eng.trace(L.TRACE_QR)]
    for d in (eng.get_mean(), eng.get_state()):
        parts += [v for _, v in sorted(d.items()) if v is not None]
    return [np.ascontiguousarray(v).tobytes() for v in parts], eng.post_count, eng.rows_done


@pytest.mark.parametrize("precision", ["f64", "f32"])
@pytest.mark.parametrize("model", ip.ENGINE_MODELS)
def test_engine_entries_at_896_items(model, precision):
    """70 x 896, F = 3, full trace, 6 sweeps with 2 burn-in: the four post-burn-in rows of the item trace, Q = 255."""
    import test_gpu_marginal_waic as t_waic
    import test_gpu_plausible_values as t_pv
    import test_gpu_quantile_marginal as t_q
    import test_gpu_scores as t_sc
    Y, logT, X, init = ip.engine_inputs(model)
    eng = _engine(model, Y, logT, X, init, n_iter=ip.ENGINE_SWEEPS, n_burnin=ip.ENGINE_BURNIN, precision=precision, full=True, q_rt=ip.Q_RT)
    eng.run(ip.ENGINE_SWEEPS)
    before = _everything(eng)
    data, rows = eng.get_data(), eng.item_trace()[ip.ENGINE_BURNIN:]
    what, Q = f"{model} {precision} 70 x 896", ip.WIDE_Q
    assert rows.shape[0] == eng.post_count == ip.ENGINE_SWEEPS - ip.ENGINE_BURNIN
    if model == "latentqr":
        got = eng.quantile_marginal_waic(nodes=Q, pointwise=True)
        t_q._assert_result_equals_loglik(got, data, rows, ip.Q_RT, Q=Q, what=what)
        assert _bytes(eng.quantile_marginal_waic(nodes=Q, pointwise=True)) == _bytes(got)
    else:
        got = eng.marginal_waic(nodes=Q, pointwise=True)
        t_waic._assert_result_equals_loglik(got, model, data, rows, Q=Q, what=what)
        sc = eng.scores(nodes=Q)
        t_sc._assert_result_equals_score(sc, model, data, rows, Q=Q, what=what)
        pv = eng.plausible_values(ip.K_DRAWS, 77, nodes=Q)
        t_pv._assert_result_equals_standalone(pv, model, data, rows, ip.K_DRAWS, 77, Q=Q, what=what)
        assert _bytes(eng.marginal_waic(nodes=Q, pointwise=True)) == _bytes(got) and _bytes(eng.scores(nodes=Q)) == _bytes(sc)
        assert _bytes(eng.plausible_values(ip.K_DRAWS, 77, nodes=Q)) == _bytes(pv)
    assert got[0]["nUnits"] == ip.ENGINE_N and got[0]["nNodes"] == Q and got[0]["nCoarse"] == 0
    assert _everything(eng) == before                                                      # the calls only read the engine
    eng.close()


def test_engine_loo_at_896_items():
    """GibbsRtIrt fp64, 70 x 896, 30 sweeps with 5 burn-in: erm_get_marginal_loo at Q = 255 against psisLooHost on the twin's l of the 25 rows."""
    import test_gpu_psis_loo as t_loo
    pkg = _pkg()
    Y, logT, X, init = ip.engine_inputs("rtirt")
    eng = _engine("rtirt", Y, logT, X, init, n_iter=ip.LOO_SWEEPS, n_burnin=ip.LOO_BURNIN, precision="f64", full=True)
    eng.run(ip.LOO_SWEEPS)
    before = _everything(eng)
    got = eng.marginal_loo(nodes=ip.WIDE_Q, pointwise=True)
    assert got["nRows"] == eng.post_count == 25 and got["nUnits"] == ip.ENGINE_N and got["nNodes"] == ip.WIDE_Q and got["tailLen"] == 5
    data, rows = eng.get_data(), eng.item_trace()[ip.LOO_BURNIN:]
    p = ip.Problem(model="rtirt", code=1, Y=data[0], logT=data[1], X=data[2], rows=rows, obs=None, Q=ip.WIDE_Q, K=ip.K_DRAWS, seed=ip.PV_SEED)
    Lh, Sh = ip.twin_loglik_by_rows(p)
    assert ip.coarse_margin(Sh) >= ip.S_MARGIN
    t_loo._assert_equals_host(got, pkg.psisLooHost(Lh), ps.bound(ps.S_GPU) + 1e-10, "rtirt f64 70 x 896, 25 rows")
    assert got["nCoarse"] == int(np.sum(np.any(Sh < ip.COARSE_S, axis=0))) == 0
    assert _bytes(eng.marginal_loo(nodes=ip.WIDE_Q, pointwise=True)) == _bytes(got) and _everything(eng) == before
    eng.close()

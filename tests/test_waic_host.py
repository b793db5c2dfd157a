"""WAIC on the host (no GPU): getWaicHost, the numpy twin the device path is tested against, on hand-built traces with known answers and on an oracle chain
against a brute-force loop over cells; compareWaic; the 2pl-against-1pl comparison fixed with the oracle chain; argument checks of the public interface."""
import math
import types

import numpy as np
import pytest

import parity_util as pu
import waic_util as wu

pkg = pu.ge.load_package()


def test_hand_built_mlirt_post():
    """Two subjects, one item, a = 1, b = 0, two post-burn-in rows: l = y theta - log(1 + e^theta)."""
    Y = np.array([[1], [0]], dtype=np.uint8)
    th = np.array([[9.0, 9.0], [9.0, 9.0], [0.5, -1.0], [1.5, 0.25]])       # rows 0, 1 are burn-in
    ra = np.concatenate([th, np.ones((4, 1)), np.zeros((4, 1))], axis=1)
    M = wu.as_sampler("mlirt", Y, None, wu.rows_to_julia(ra), np.zeros(0), np.zeros(0), nIter=4, nChain=1, nBurnin=2)
    w = pkg.getWaicHost(M, "subject")
    l = lambda y, t: y * t - math.log1p(math.exp(t))
    l0, l1 = (l(1, 0.5), l(1, 1.5)), (l(0, -1.0), l(0, 0.25))
    lppd = [math.log((math.exp(a) + math.exp(b)) / 2) for a, b in (l0, l1)]
    p = [(a - b) ** 2 / 2 for a, b in (l0, l1)]
    assert np.allclose(w.lppd_u, lppd, rtol=1e-14, atol=0) and np.allclose(w.p_u, p, rtol=1e-13, atol=0)
    el = [lppd[0] - p[0], lppd[1] - p[1]]
    assert abs(w.elpd - sum(el)) <= 1e-14 and abs(w.WAIC + 2 * sum(el)) <= 1e-14 and abs(w.pWaic - sum(p)) <= 1e-15
    assert abs(w.se - 2 * math.sqrt(2 * (el[0] - el[1]) ** 2 / 2)) <= 1e-13        # U Var_u with U = 2, ddof = 1
    assert w.nUnits == 2 and w.nRows == 2 and w.nHighVar == sum(v > 0.4 for v in p)
    c = pkg.getWaicHost(M, "cell")                       # one item: the cells are the subjects
    assert c.lppd_u.shape == (2, 1) and np.array_equal(c.lppd_u[:, 0], w.lppd_u) and c.elpd == w.elpd


def test_hand_built_crossqr_cell():
    """One cell of GibbsRtIrtCrossQr: the response term plus log N(logT; lambda - zeta - theta rho + k1 nu, sig2t k2 nu)."""
    q = 0.85
    k1, k2 = (1 - 2 * q) / (q * (1 - q)), 2 / (q * (1 - q))
    Y, logT = np.array([[1]], dtype=np.uint8), np.array([[0.7]])
    rows = [dict(th=0.3, a=1.2, b=-0.4, ze=0.2, lam=0.9, sg=0.5, rho=0.1, nu=1.7), dict(th=-0.6, a=0.8, b=0.1, ze=-0.3, lam=1.1, sg=0.7, rho=-0.2, nu=0.4)]
    ra = np.array([[r["th"], r["a"], r["b"]] for r in rows])
    rt = np.array([[r["ze"], r["lam"], r["sg"]] for r in rows])
    qr = np.array([[r["rho"], 1, 0, 0, 1, r["nu"]] for r in rows])
    M = wu.as_sampler("crossqr", Y, logT, wu.rows_to_julia(ra), wu.rows_to_julia(rt), wu.rows_to_julia(qr), nIter=2, nChain=1, nBurnin=0, qRt=q)
    ls = []
    for r in rows:
        eta = r["a"] * (r["th"] - r["b"])
        mu, var = r["lam"] - r["ze"] - r["th"] * r["rho"] + k1 * r["nu"], r["sg"] * k2 * r["nu"]
        ls.append(eta - math.log1p(math.exp(eta)) - 0.5 * math.log(2 * math.pi * var) - 0.5 * (0.7 - mu) ** 2 / var)
    w = pkg.getWaicHost(M, "cell")
    assert abs(w.lppd - math.log((math.exp(ls[0]) + math.exp(ls[1])) / 2)) <= 1e-14 and abs(w.pWaic - (ls[0] - ls[1]) ** 2 / 2) <= 1e-14
    assert w.se == 0.0 and w.nUnits == 1


@pytest.mark.parametrize("model", ["rtirt", "crossqr", "latentqr"])
def test_twin_totals_equal_a_brute_force_loop_over_the_cells_of_an_oracle_chain(model):
    N, J, T = 30, 5, 10
    Y, logT, X, init, tp = pu.make_problem(model, N, J, 3, seed=9)
    M = wu.oracle_sampler(model, Y, logT, X, init, T)
    q = 0.85
    k1, k2 = ((1 - 2 * q) / (q * (1 - q)), 2 / (q * (1 - q))) if model == "crossqr" else (0.0, 1.0)
    P = M.Post
    S = range(T // 2, T)
    lc = np.zeros((len(S), N, J))
    for s, it in enumerate(S):
        for i in range(N):
            for j in range(J):
                th, a, b = P.ra[it, i, 0], P.ra[it, N + j, 0], P.ra[it, N + J + j, 0]
                ze, lam, sg = P.rt[it, i, 0], P.rt[it, N + j, 0], P.rt[it, N + J + j, 0]
                eta = a * (th - b)
                l = (eta if Y[i, j] else 0.0) - (eta + math.log1p(math.exp(-eta)) if eta > 0 else math.log1p(math.exp(eta)))
                mu, var = lam - ze, sg
                if model == "crossqr":
                    nu = P.qr[it, J + 4 + i + N * j, 0]
                    mu += -th * P.qr[it, j, 0] + k1 * nu
                    var *= k2 * nu
                lc[s, i, j] = l - 0.5 * math.log(2 * math.pi) - 0.5 * math.log(var) - 0.5 * (logT[i, j] - mu) ** 2 / var
    for unit, L in (("cell", lc.reshape(len(S), -1)), ("subject", lc.sum(axis=2))):
        U = L.shape[1]
        lppd = np.array([math.log(sum(math.exp(v) for v in L[:, u]) / len(S)) for u in range(U)])
        p = np.array([sum((v - L[:, u].mean()) ** 2 for v in L[:, u]) / (len(S) - 1) for u in range(U)])
        el = lppd - p
        w = pkg.getWaicHost(M, unit)
        tot = dict(elpd=el.sum(), pWaic=p.sum(), WAIC=-2 * el.sum(), lppd=lppd.sum(), se=2 * math.sqrt(U * sum((v - el.mean()) ** 2 for v in el) / (U - 1)))
        for k, v in tot.items():
            assert abs(getattr(w, k) - v) <= 1e-12 * abs(v), (unit, k, getattr(w, k), v)
        assert w.nHighVar == int((p > 0.4).sum()) and w.nUnits == U and w.nRows == len(S)
        got = w.lppd_u.reshape(N, J)[3, 2] if unit == "cell" else w.lppd_u[3]      # cells come back as (nSubj, nItem)
        assert abs(got - (lppd.reshape(N, J)[3, 2] if unit == "cell" else lppd[3])) <= 1e-12 * abs(got)


def test_oracle_chain_prefers_2pl_on_spread_discriminations_by_more_than_4_se():
    """Fixes the size and chain length of tests/test_gpu_waic.py's comparison on the CPU: 600 subjects x 12 items with true discriminations 0.25 ... 3,
    200 sweeps (100 post-burn-in), subject unit.  Measured with the oracle chain: elpd_diff = 276.1, se_diff = 20.85, a margin of 13.2 se_diff."""
    Y, X, init = wu.spread_problem()
    w = {onepl: pkg.getWaicHost(wu.oracle_sampler("mlirt", Y, None, X, init, wu.SPREAD_ITER, onepl=onepl), "subject") for onepl in (False, True)}
    c = pkg.compareWaic(w[False], w[True])
    print(f"2pl - 1pl: elpd_diff {c['elpd_diff']:.4f}, se_diff {c['se_diff']:.4f}, margin {c['elpd_diff'] / c['se_diff']:.2f} se_diff")
    assert c["elpd_diff"] >= 4.0 * c["se_diff"] > 0.0
    back = pkg.compareWaic(w[True], w[False])
    assert back["elpd_diff"] == -c["elpd_diff"] and back["se_diff"] == c["se_diff"]


def test_comparewaic_refuses_fits_that_do_not_match():
    W = pkg.OutputWaic
    a = W(unit="subject", lppd_u=np.zeros(5), p_u=np.zeros(5))
    with pytest.raises(ValueError, match="different units"):
        pkg.compareWaic(a, W(unit="cell", lppd_u=np.zeros(5), p_u=np.zeros(5)))
    with pytest.raises(ValueError, match="different numbers of units"):
        pkg.compareWaic(a, W(unit="subject", lppd_u=np.zeros(6), p_u=np.zeros(6)))
    with pytest.raises(ValueError, match="pointwise"):
        pkg.compareWaic(a, W(unit="subject"))
    d = pkg.compareWaic(W(unit="subject", lppd_u=np.array([-1.0, -2.0, -4.0]), p_u=np.array([0.5, 0.5, 0.5])), W(unit="subject", lppd_u=np.array([-2.0, -2.0, -2.0]), p_u=np.zeros(3)))
    assert d["elpd_diff"] == -2.5 and abs(d["se_diff"] - math.sqrt(3 * np.var([0.5, -0.5, -2.5], ddof=1))) <= 1e-15


def test_public_interface_checks_its_arguments_before_touching_a_device():
    Cond = pkg.setCond(nSubj=10, nItem=3, nFeat=1, nIter=4, nChain=1)
    M = pkg.GibbsMlIrt(Cond)
    with pytest.raises(ValueError, match="waic must be"):
        pkg.sample_b(M, waic="item")
    with pytest.raises(ValueError, match="chain farm"):
        pkg.sample_b(M, waic="subject", devices=[0])
    with pytest.raises(ValueError, match="run sample"):
        pkg.getWaic(M)
    M.farm = types.SimpleNamespace(close=lambda: None)
    with pytest.raises(ValueError, match="devices="):
        pkg.getWaic(M)
    M.farm = None
    L = pkg._lib
    assert (L.POINTWISE_OFF, L.POINTWISE_SUBJECT, L.POINTWISE_CELL) == (0, 1, 2)
    for name in ("erm_set_pointwise", "erm_get_waic", "erm_pointwise_units", "erm_get_pointwise"):
        assert name in L.EXPORTS and hasattr(L.load(), name)

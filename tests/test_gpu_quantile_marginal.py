"""LatentQr's marginal WAIC and PSIS-LOO on the device: theta, zeta and the quantile weight nu integrated out (erm_get_quantile_marginal_waic / _loo, their farm
entries, erm_quantile_marginal_loglik).
  1. erm_quantile_marginal_loglik against quantileMarginalLogLikHost, the numpy twin (itself pinned to scipy's dblquad and quad and to 60-digit mpmath in
     tests/test_qmarginal_host.py): every l_i^(s), lppd_i, p_i and the totals to 1e-10 relative, with tests/test_gpu_marginal_waic.py's LPPD_FLOOR rule -- the
     tolerance of this kernel family -- at 37 x 9, 3 rows, F = 3, q in {0.5, 0.85}, Q in {3, 61, 127}; the edges J = 1, J = 65, N = 1, F = 0; the extremes
     m = +-30, s in {0.001, 50}, one subject's logT 22 off, J = 1, at the same 1e-10.  (Were an extreme to miss it, its bound would be ten times the error of the
     header's HOST build against the 60-digit value, which tests/test_qmarginal_host.py prints: 7.6e-15, 1.9e-14, 3.1e-14, 1.6e-14 in the order of
     qmarginal_util.extreme_cases() -- never a figure taken from the kernel.)  The coarse count equals the twin's.  Measured on an MI355X, for the record: l within
     8.5e-16 of the twin at the ordinary shapes, within 2.4e-14 at the extremes.
  2. independence: a subject's outputs are bit-identical whether it is computed among 600 subjects, among a part of them or alone (tile tails at 256 and 599).
  3. the engine entries: a LatentQr engine, 200 x 7, F = 3, 40 sweeps as two interleaved chains of 20 with 10 burn-in sweeps (5 iterations per chain: 30 post-burn-in
     rows, enough for PSIS-LOO's 25); fp64 and fp32, both trace modes.  erm_get_quantile_marginal_waic equals erm_quantile_marginal_loglik on erm_get_data's data
     set, the post-burn-in rows of erm_get_item_trace and the engine's q_rt; bit-identical when called twice and when the sweeps are split 17 + 23; the chain, the
     traces and the state are unchanged by the call; the LOO entry equals erm_psis_loo on that l bit for bit.
  4. the farm: two chains on one device against the chain-major table; one chain equals its engine bit for bit.
  5. every refusal returns its code, and the engine or farm runs on afterwards; erm_get_marginal_waic still refuses a LatentQr engine.
  6. getWaicMarginalQr and getLooMarginalQr on a run sampler: finite, nCoarse == 0, equal to the host twin; compareWaic accepts (Latent, LatentQr) fitted to the same
     data -- the difference is printed, not asserted: no chain-level margin has been measured."""
import numpy as np
import pytest

import parity_util as pu
import qmarginal_util as qu
from item_pass_util import _bytes, _engine, _farm, _pkg

pytestmark = pytest.mark.gpu

TOL = 1e-10
LPPD_FLOOR = 1e-3
TOTALS = ("elpd", "pWaic", "WAIC", "se", "lppd")
_loo_bytes = _bytes          # the dict of a LOO entry: its twelve totals and four columns


def _assert_equals_twin(Y, logT, X, rows, q, Q, what=""):
    pkg = _pkg()
    dev = pkg._lib.quantile_marginal_loglik(qu.CODE, Y, logT, X, rows, q, nodes=Q)
    Lh, S = pkg.quantileMarginalLogLikHost(qu.CODE, Y, logT, X, rows, q, Q, with_S=True)
    host = pkg.twins.waicFromLogLik(Lh)
    el = np.max(np.abs(dev["l"].T - Lh) / np.abs(Lh))
    elp = np.max(np.abs(dev["lppd"] - host.lppd_u) / np.maximum(np.abs(host.lppd_u), LPPD_FLOOR))
    ep = np.max(np.abs(dev["p"] - host.p_u) / np.abs(host.p_u))
    t = dev["totals"]
    print(f"{what} N={Y.shape[0]} J={Y.shape[1]} q={q} Q={Q}: max rel err l {el:.3g}, lppd_i {elp:.3g}, p_i {ep:.3g}; l in [{Lh.min():.4g}, {Lh.max():.4g}]; " +
          ", ".join(f"{k} {t[k]!r} / {getattr(host, k)!r}" for k in TOTALS) + f"; coarse {t['nCoarse']}")
    assert np.all(np.isfinite(dev["l"])) and el <= TOL and elp <= TOL and ep <= TOL
    for k in TOTALS:
        assert abs(t[k] - getattr(host, k)) <= TOL * abs(getattr(host, k)), k
    assert t["nUnits"] == Y.shape[0] and t["nRows"] == rows.shape[0] and t["nNodes"] == Q and t["nHighVar"] == host.nHighVar
    assert t["nCoarse"] == int(np.sum(np.any(S < 2.0, axis=0)))
    return dev


# ------------------------------------------------------------------------------------------------------------ the kernel against the twin
@pytest.mark.parametrize("Q", [3, 61, 127])
@pytest.mark.parametrize("q", [0.5, 0.85])
def test_loglik_equals_twin(q, Q):
    rows = qu.make_rows(9, 3, 3, seed=11)
    Y, logT, X = qu.make_data(37, 9, 3, seed=11)
    _assert_equals_twin(Y, logT, X, rows, q, Q)


@pytest.mark.parametrize("N,J,F", [(37, 1, 3), (37, 65, 3), (1, 9, 3), (37, 9, 0)])
def test_loglik_equals_twin_at_the_edges_of_the_shapes(N, J, F):
    rows = qu.make_rows(J, F, 3, seed=5)
    Y, logT, X = qu.make_data(N, J, F, seed=5)
    _assert_equals_twin(Y, logT, X, rows, 0.85, 61)


def test_loglik_equals_twin_at_the_extremes():
    for name, Y, logT, rows, q in qu.extreme_cases():
        _assert_equals_twin(Y, logT, None, rows, q, 61, what=name)


# ------------------------------------------------------------------------------------------------------------ independence
def test_a_subjects_result_depends_on_its_own_data_only():
    L = _pkg()._lib
    rows = qu.make_rows(9, 3, 4, seed=31)
    Y, logT, X = qu.make_data(600, 9, 3, seed=31)
    whole = L.quantile_marginal_loglik(qu.CODE, Y, logT, X, rows, 0.85)
    for lo, hi in ((0, 256), (256, 600), (599, 600)):
        part = L.quantile_marginal_loglik(qu.CODE, Y[lo:hi], logT[lo:hi], X[lo:hi], rows, 0.85)
        for k in ("l", "lppd", "p"):
            assert np.all(np.isfinite(part[k])) and np.array_equal(part[k], whole[k][lo:hi]), (k, lo, hi)


# ------------------------------------------------------------------------------------------------------------ the engine entries
def _assert_result_equals_loglik(got, data, rows, q, Q=61, what=""):
    """(totals, lppd, p) of an engine or farm entry against erm_quantile_marginal_loglik on the same data, rows and level; returns that call's result."""
    L = _pkg()._lib
    Y, logT, X = data
    w, lppd, p = got
    ref = L.quantile_marginal_loglik(qu.CODE, Y, logT, X, rows, q, nodes=Q)
    elp = np.max(np.abs(lppd - ref["lppd"]) / np.maximum(np.abs(ref["lppd"]), LPPD_FLOOR))
    ep = np.max(np.abs(p - ref["p"]) / np.abs(ref["p"]))
    print(f"{what}: rows {w['nRows']}, max rel err lppd_i {elp:.3g}, p_i {ep:.3g}; " + ", ".join(f"{k} {w[k]!r} / {ref['totals'][k]!r}" for k in TOTALS) + f"; coarse {w['nCoarse']}")
    assert elp <= TOL and ep <= TOL
    for k in TOTALS:
        assert abs(w[k] - ref["totals"][k]) <= TOL * abs(ref["totals"][k]), k
    for k in ("nUnits", "nRows", "nNodes", "nHighVar", "nCoarse"):
        assert w[k] == ref["totals"][k], k
    return ref


def _loo_via_loglik(data, rows, q, Q=61):
    """erm_psis_loo on the l erm_quantile_marginal_loglik returns, with the node count and the coarse count of the marginal kernel's totals."""
    L = _pkg()._lib
    m = L.quantile_marginal_loglik(qu.CODE, *data, rows, q, nodes=Q)
    r = L.psis_loo(m["l"])
    r["nNodes"], r["nCoarse"] = m["totals"]["nNodes"], m["totals"]["nCoarse"]
    return r


@pytest.mark.parametrize("full", [True, False], ids=["full", "summary"])
@pytest.mark.parametrize("precision", ["f64", "f32"])
def test_engine_entries_equal_loglik_on_their_own_data_and_rows(precision, full):
    L = _pkg()._lib
    Y, logT, X, init, tp = pu.make_problem("latentqr", 200, 7, 3, seed=41)
    mk = lambda: _engine("latentqr", Y, logT, X, init, n_iter=20, n_chain=2, n_burnin=5, precision=precision, full=full)
    eng = mk()
    eng.run(40)

    def everything():
        parts = [eng.item_trace()] + ([eng.trace(w) for w in (L.TRACE_LOGLIKE, L.TRACE_RA, L.TRACE_RT, L.TRACE_QR)] if full else [])      # (summary mode keeps no full traces)
        for d in (eng.get_mean(), eng.get_state()):
            parts += [v for _, v in sorted(d.items()) if v is not None]
        return [np.ascontiguousarray(p).tobytes() for p in parts], eng.post_count, eng.rows_done

    before = everything()
    got = eng.quantile_marginal_waic(pointwise=True)
    assert got[0]["nRows"] == eng.post_count == 30 and got[0]["nUnits"] == 200 and got[0]["nNodes"] == 61
    data, rows = eng.get_data(), eng.item_trace()[10:]
    _assert_result_equals_loglik(got, data, rows, 0.85, what=f"latentqr {precision} {'full' if full else 'summary'}")
    assert _bytes(eng.quantile_marginal_waic(pointwise=True)) == _bytes(got)              # twice
    assert eng.quantile_marginal_waic() == got[0]                                         # without the pointwise vectors: the same totals
    loo = eng.quantile_marginal_loo(pointwise=True)
    assert loo["nRows"] == 30 and loo["nUnits"] == 200 and loo["tailLen"] == 6
    assert _loo_bytes(loo) == _loo_bytes(_loo_via_loglik(data, rows, 0.85))               # bit for bit
    assert _loo_bytes(eng.quantile_marginal_loo(pointwise=True)) == _loo_bytes(loo)
    assert everything() == before                                                         # the calls only read the engine
    split = mk()
    split.run(17)
    split.run(23)
    assert _bytes(split.quantile_marginal_waic(pointwise=True)) == _bytes(got)
    assert _loo_bytes(split.quantile_marginal_loo(pointwise=True)) == _loo_bytes(loo)
    eng.close()
    split.close()


def test_engine_entry_reads_the_engines_own_level():
    """Two engines that differ in q_rt alone, each against erm_quantile_marginal_loglik at its own level; the levels give different results."""
    Y, logT, X, init, tp = pu.make_problem("latentqr", 200, 7, 3, seed=41)
    elpd = {}
    for q in (0.85, 0.3):
        eng = _engine("latentqr", Y, logT, X, init, n_iter=12, n_burnin=4, q_rt=q)
        eng.run(12)
        got = eng.quantile_marginal_waic(pointwise=True)
        _assert_result_equals_loglik(got, eng.get_data(), eng.item_trace()[4:], q, what=f"q_rt {q}")
        elpd[q] = got[0]["elpd"]
        eng.close()
    assert elpd[0.85] != elpd[0.3]


# ------------------------------------------------------------------------------------------------------------ the farm
def test_farm_equals_loglik_on_the_chain_major_rows():
    Y, logT, X, init, tp = pu.make_problem("latentqr", 200, 7, 3, seed=47)
    farm = _farm("latentqr", [0, 0], Y, logT, X, init, n_iter=20, n_burnin=6)
    farm.run(20)
    rows = np.concatenate([farm.engine(l).item_trace()[6:] for l in range(2)], axis=0)
    got = farm.quantile_marginal_waic(pointwise=True)
    assert got[0]["nRows"] == farm.post_count == 28
    data = farm.engine(0).get_data()
    _assert_result_equals_loglik(got, data, rows, 0.85, what="farm of 2")
    assert _bytes(farm.quantile_marginal_waic(pointwise=True)) == _bytes(got)
    assert _loo_bytes(farm.quantile_marginal_loo(pointwise=True)) == _loo_bytes(_loo_via_loglik(data, rows, 0.85))
    farm.close()


def test_farm_of_one_chain_equals_its_engine_bit_for_bit():
    Y, logT, X, init, tp = pu.make_problem("latentqr", 200, 7, 3, seed=49)
    farm = _farm("latentqr", [0], Y, logT, X, init, n_iter=40, n_burnin=12)
    farm.run(40)
    assert _bytes(farm.quantile_marginal_waic(pointwise=True)) == _bytes(farm.engine(0).quantile_marginal_waic(pointwise=True))
    assert _loo_bytes(farm.quantile_marginal_loo(pointwise=True)) == _loo_bytes(farm.engine(0).quantile_marginal_loo(pointwise=True))
    farm.close()


# ------------------------------------------------------------------------------------------------------------ refusals
def test_every_refusal_returns_its_code_and_leaves_the_engine_usable():
    L = _pkg()._lib
    lib = L.load()
    err = lambda: lib.erm_last_error().decode()
    out, out12 = np.zeros(10), np.zeros(12)
    waic = lambda e, n=0: lib.erm_get_quantile_marginal_waic(e._h, n, out.ctypes.data, None, None)
    loo = lambda e, n=0: lib.erm_get_quantile_marginal_loo(e._h, n, out12.ctypes.data, None)
    Y, logT, X, init, tp = pu.make_problem("latentqr", 200, 7, 3, seed=31)
    eng = _engine("latentqr", Y, logT, X, init, n_iter=6, n_burnin=2)
    assert waic(eng) == -3 and "two post-burn-in rows" in err()                          # ERM_ERR_STATE: nothing recorded
    eng.run(3)                                                                           # rows 0, 1 burn-in, one post-burn-in row
    assert waic(eng) == -3 and "two post-burn-in rows" in err()
    eng.run(3)
    for bad in (60, 1, 1027, -3):
        assert waic(eng, bad) == -1 and "odd" in err()                                   # ERM_ERR_ARG
        assert loo(eng, bad) == -1 and "odd" in err()
    assert lib.erm_get_quantile_marginal_waic(eng._h, 0, None, None, None) == -1 and lib.erm_get_quantile_marginal_loo(eng._h, 0, None, None) == -1
    assert loo(eng) == -1 and "at least 25 rows" in err()                                # four rows: too few for PSIS-LOO
    assert waic(eng) == 0 and out[5] == 200 and out[6] == 4 and out[8] == 61
    assert waic(eng, 3) == 0 and out[8] == 3 and out[9] == 200                           # three nodes: every unit is coarse
    # the entries that were there still refuse a LatentQr engine
    assert lib.erm_get_marginal_waic(eng._h, 0, out.ctypes.data, None, None) == -1 and "quantile" in err()
    assert lib.erm_get_marginal_loo(eng._h, 0, out12.ctypes.data, None) == -1 and "quantile" in err()
    eng.close()
    # the five models without quantile weights, and CrossQr
    for model in ("mlirt", "rtirt", "null", "cross", "latent", "crossqr"):
        Ym, lm, Xm, im, _ = pu.make_problem(model, 200, 7, 3, seed=33)
        e = _engine(model, Ym, lm, Xm, im, n_iter=6, n_burnin=2)
        e.run(4)
        for call in (waic, loo):
            assert call(e) == -1 and ("asymmetric Laplace" if model == "crossqr" else "erm_get_marginal_waic") in err(), model
        e.run(2)
        e.close()
    # a subject-sharded engine
    sh = L.Engine(model=L.MODEL_LATENTQR, n_item=7, n_subj=200, n_feat=3, n_iter=6, n_chain=1, n_burnin=2, cov2one=0, q_rt=0.85, seed=1, precision=L.PREC_F64, trace_mode=0)
    sh.set_shard(0, 1, 200, 0, lambda s, r, n: lib.erm_copy(r, s, n))
    sh.set_data(Y, logT, X)
    sh.set_state(**init)
    sh.run(4)
    assert waic(sh) == -3 and "shard" in err()
    assert loo(sh) == -3 and "shard" in err()
    sh.run(2)
    sh.close()
    # the farm: a model without quantile weights, too few rows, a bad node count -- and it runs on
    Yr, lr, Xr, ir, _ = pu.make_problem("latent", 200, 7, 3, seed=33)
    farm = _farm("latent", [0, 0], Yr, lr, Xr, ir, n_iter=6, n_burnin=2)
    farm.run(6)
    assert lib.erm_farm_get_quantile_marginal_waic(farm._h, 0, out.ctypes.data, None, None) == -1 and "erm_get_marginal_waic" in err()
    assert lib.erm_farm_get_quantile_marginal_loo(farm._h, 0, out12.ctypes.data, None) == -1 and "erm_get_marginal_waic" in err()
    farm.close()
    farm = _farm("latentqr", [0, 0], Y, logT, X, init, n_iter=6, n_burnin=2)
    fcall = lambda n=0: lib.erm_farm_get_quantile_marginal_waic(farm._h, n, out.ctypes.data, None, None)
    farm.run(3)
    assert fcall() == -3 and "chain 0" in err() and "two post-burn-in rows" in err()
    assert fcall(8) == -1
    farm.run(3)
    assert fcall() == 0 and out[6] == 8
    assert lib.erm_farm_get_quantile_marginal_loo(farm._h, 0, out12.ctypes.data, None) == -1 and "at least 25 rows" in err()
    assert lib.erm_farm_get_marginal_waic(farm._h, 0, out.ctypes.data, None, None) == -1 and "quantile" in err()
    farm.close()
    # erm_quantile_marginal_loglik
    rows = qu.make_rows(9, 3, 3, seed=1)
    Ys, ls, Xs = qu.make_data(5, 9, 3, seed=1)
    code = lambda f: int(str(f.value).split()[2].rstrip(":"))
    good = L.quantile_marginal_loglik(qu.CODE, Ys, ls, Xs, rows, 0.85)
    for bad in (0.0, 1.0, -0.3, 1.5, float("nan")):
        with pytest.raises(L.ErmError, match="q_rt") as e:
            L.quantile_marginal_loglik(qu.CODE, Ys, ls, Xs, rows, bad)
        assert code(e) == -1
    for bad_s in (0.0, -0.2):
        with pytest.raises(L.ErmError, match=r"row 1: Sigma_p\[2,2\] must be positive") as e:
            bad = rows.copy(); bad[1, -1] = bad_s
            L.quantile_marginal_loglik(qu.CODE, Ys, ls, Xs, bad, 0.85)
        assert code(e) == -1
    with pytest.raises(L.ErmError, match=r"row 0: Sigma_p\[1,1\]") as e:
        bad = rows.copy(); bad[0, -4] = 0.0
        L.quantile_marginal_loglik(qu.CODE, Ys, ls, Xs, bad, 0.85)
    assert code(e) == -1
    with pytest.raises(L.ErmError, match="row 2: sig2t") as e:
        bad = rows.copy(); bad[2, 3 * 9 + 1] = 0.0
        L.quantile_marginal_loglik(qu.CODE, Ys, ls, Xs, bad, 0.85)
    assert code(e) == -1
    with pytest.raises(L.ErmError, match="NaN in row 1") as e:
        bad = rows.copy(); bad[1, 4] = np.nan
        L.quantile_marginal_loglik(qu.CODE, Ys, ls, Xs, bad, 0.85)
    assert code(e) == -4                                                                 # ERM_ERR_NONFINITE
    with pytest.raises(L.ErmError, match="NaN in logT") as e:
        lb = ls.copy(); lb[2, 3] = np.nan
        L.quantile_marginal_loglik(qu.CODE, Ys, lb, Xs, rows, 0.85)
    assert code(e) == -4
    with pytest.raises(L.ErmError, match="n_rows") as e:
        L.quantile_marginal_loglik(qu.CODE, Ys, ls, Xs, rows[:1], 0.85)                  # the WAIC outputs need two rows
    assert code(e) == -1
    with pytest.raises(L.ErmError, match="odd") as e:                                    # (the binding checks the node count itself: call the library)
        Yf, lf, Xf = np.asfortranarray(Ys), np.asfortranarray(ls), np.asfortranarray(Xs)
        L.check(lib.erm_quantile_marginal_loglik(0, qu.CODE, 5, 9, 3, Yf.ctypes.data, lf.ctypes.data, Xf.ctypes.data, rows.ctypes.data, 3, 0.85, 60, None, out.ctypes.data, None, None))
    assert code(e) == -1
    one = L.quantile_marginal_loglik(qu.CODE, Ys, ls, Xs, rows[:1], 0.85, want_waic=False)  # l alone does not
    assert one["l"].shape == (5, 1) and np.array_equal(one["l"][:, 0], good["l"][:, 0])
    for model in (L.MODEL_MLIRT, L.MODEL_RTIRT, L.MODEL_NULL, L.MODEL_CROSS, L.MODEL_LATENT):
        with pytest.raises(L.ErmError, match="erm_get_marginal_waic") as e:
            L.quantile_marginal_loglik(model, Ys, ls, Xs, np.ones((2, L.item_trace_width(model, 9, L.kernel_feat(model, 3)))), 0.85)
        assert code(e) == -1
    with pytest.raises(L.ErmError, match="asymmetric Laplace") as e:
        L.quantile_marginal_loglik(L.MODEL_CROSSQR, Ys, ls, None, np.zeros((2, 5 * 9 + 4)), 0.85)
    assert code(e) == -1
    with pytest.raises(L.ErmError, match="quantile") as e:
        L.marginal_loglik(qu.CODE, Ys, ls, Xs, rows)                                     # the Gaussian entry keeps refusing LatentQr rows
    assert code(e) == -1


# ------------------------------------------------------------------------------------------------------------ the public interface
def test_get_waic_and_loo_marginal_qr_on_samplers_and_compare_waic():
    """GibbsRtIrtLatent and GibbsRtIrtLatentQr fitted to the same 300 x 9 data set, 60 sweeps (30 post-burn-in rows), through the public interface."""
    pkg = _pkg()
    Y, logT, X, init, tp = pu.make_problem("latentqr", 300, 9, 3, seed=51)
    Cond = pkg.setCond(nSubj=300, nItem=9, nFeat=3, nIter=60, nChain=1, qRt=0.85)
    D = pkg.InputData(Y=Y, T=np.exp(logT), X=X)
    Mq = pkg.GibbsRtIrtLatentQr(Cond, Data=D, trace="summary")
    pkg.sample_b(Mq)
    w, host = pkg.getWaicMarginalQr(Mq, pointwise=True), pkg.getWaicMarginalQrHost(Mq)
    assert w.unit == host.unit == "subject-marginal" and w.nNodes == 61 and w.nCoarse == host.nCoarse == 0 and w.nRows == host.nRows == 30 and w.nUnits == 300
    assert np.isfinite(w.elpd) and np.isfinite(w.se) and np.all(np.isfinite(w.lppd_u)) and np.all(np.isfinite(w.p_u))
    assert np.max(np.abs(w.lppd_u - host.lppd_u) / np.maximum(np.abs(host.lppd_u), LPPD_FLOOR)) <= TOL and abs(w.elpd - host.elpd) <= TOL * abs(host.elpd)
    assert pkg.getWaicMarginalQr(Mq).elpd == w.elpd and pkg.getWaicMarginalQr(Mq).lppd_u is None
    loo = pkg.getLooMarginalQr(Mq, pointwise=True)
    assert loo.unit == "subject-marginal" and loo.nRows == 30 and loo.nUnits == 300 and loo.nCoarse == 0 and np.isfinite(loo.elpd) and np.all(np.isfinite(loo.elpd_u))
    assert abs(loo.lppd - w.lppd) <= 1e-12 * abs(w.lppd)                                  # lppd_i is the marginal WAIC's
    with pytest.raises(ValueError, match="quantile"):
        pkg.getWaicMarginal(Mq)
    Ml = pkg.GibbsRtIrtLatent(Cond, Data=D, trace="summary")
    pkg.sample_b(Ml)
    wl = pkg.getWaicMarginal(Ml, pointwise=True)
    c = pkg.compareWaic(wl, w)
    print(f"Latent {wl.elpd:.2f} (p {wl.pWaic:.2f}), LatentQr at 0.85 {w.elpd:.2f} (p {w.pWaic:.2f}); Latent - LatentQr: elpd_diff {c['elpd_diff']:.2f}, se_diff {c['se_diff']:.2f}")
    assert c["unit"] == "subject-marginal" and c["nUnits"] == 300 and np.isfinite(c["elpd_diff"]) and c["se_diff"] > 0.0
    cl = pkg.compareLoo(pkg.getLooMarginal(Ml, pointwise=True), loo)
    assert np.isfinite(cl["elpd_diff"])
    with pytest.raises(ValueError, match="no quantile weights"):
        pkg.getWaicMarginalQr(Ml)
    Mq.close()
    Ml.close()

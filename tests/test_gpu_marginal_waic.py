"""Marginal WAIC on the device (erm_get_marginal_waic / erm_farm_get_marginal_waic / erm_marginal_loglik).
  1. erm_marginal_loglik against marginalLogLikHost, the numpy twin (itself pinned to scipy's quad in tests/test_marginal_host.py): every l_i^(s), lppd_i, p_i and
     the totals to 1e-10 relative -- the tolerance tests/test_gpu_waic.py uses between a device log-likelihood (log1pexp_r, its own summation order) and numpy, with
     its LPPD_FLOOR rule for |lppd| < 1e-3 -- for the five models at 37 x 9, Q in {3, 61, 127} (node counts that are no multiple of the eight lanes per subject),
     J = 1, J = 65, N = 1, and three extremes: a subject all correct against a_j = 8, terms down to -1400 through a far-off logT, Sigma_p of correlation exactly 1.
  2. independence: a subject's outputs are bit-identical whether it is computed among 600 subjects, among a part of them or alone (tile tails included).
  3. the engine entry against erm_marginal_loglik on erm_get_data's data set and the post-burn-in rows of erm_get_item_trace: fp64 and fp32 engines, both trace
     modes, two interleaved chains; bit-identical when called twice and when the sweeps are split 17 + 23; the chain, the traces and erm_get_waic's accumulators
     are unchanged by the call.
  4. the farm: two and three chains on one device against erm_marginal_loglik on the chain-major concatenation of the chains' rows; one chain equals its engine bit
     for bit; getWaicMarginal on a devices= sampler, compareWaic on two such results.
  5. every refusal returns its code, and the engine or farm runs on afterwards.
  6. model choice: the marginal elpd prefers 2pl over 1pl on waic_util.spread_problem() by more than 2 se_diff (on the CPU, with the oracle chain and the twin, the
     margin is 8.9 se_diff: elpd_diff 166.3, se_diff 18.8 -- tests/test_marginal_host.py)."""
import numpy as np
import pytest

import marginal_util as mu
import parity_util as pu
import waic_util as wu
from item_pass_util import _bytes, _engine, _farm, _kernel_x, _pkg

pytestmark = pytest.mark.gpu

TOL = 1e-10
LPPD_FLOOR = 1e-3
TOTALS = ("elpd", "pWaic", "WAIC", "se", "lppd")


def _assert_equals_twin(model, Y, logT, X, rows, Q, what=""):
    pkg = _pkg()
    dev = pkg._lib.marginal_loglik(mu.CODE[model], Y, logT, X, rows, nodes=Q)
    Lh, S = pkg.marginalLogLikHost(mu.CODE[model], Y, logT, _kernel_x(model, X), rows, Q, with_S=True)
    host = pkg.twins.waicFromLogLik(Lh)
    el = np.max(np.abs(dev["l"].T - Lh) / np.abs(Lh))
    elp = np.max(np.abs(dev["lppd"] - host.lppd_u) / np.maximum(np.abs(host.lppd_u), LPPD_FLOOR))
    ep = np.max(np.abs(dev["p"] - host.p_u) / np.abs(host.p_u))
    t = dev["totals"]
    print(f"{what or model} N={Y.shape[0]} J={Y.shape[1]} Q={Q}: max rel err l {el:.3g}, lppd_i {elp:.3g}, p_i {ep:.3g}; l in [{Lh.min():.4g}, {Lh.max():.4g}]; " +
          ", ".join(f"{k} {t[k]!r} / {getattr(host, k)!r}" for k in TOTALS) + f"; coarse {t['nCoarse']}")
    assert np.all(np.isfinite(dev["l"])) and el <= TOL and elp <= TOL and ep <= TOL
    for k in TOTALS:
        assert abs(t[k] - getattr(host, k)) <= TOL * abs(getattr(host, k)), k
    assert t["nUnits"] == Y.shape[0] and t["nRows"] == rows.shape[0] and t["nNodes"] == Q and t["nHighVar"] == host.nHighVar
    assert t["nCoarse"] == int(np.sum(np.any(S < 2.0, axis=0)))
    return dev


# ------------------------------------------------------------------------------------------------------------ the kernel against the twin
@pytest.mark.parametrize("Q", [3, 61, 127])
@pytest.mark.parametrize("model", mu.MODELS)
def test_loglik_equals_twin(model, Q):
    F = 0 if (model, Q) == ("rtirt", 127) else 3
    rows = mu.make_rows(model, 9, F, 3, seed=11)
    Y, logT, X = mu.make_data(model, 37, 9, F, seed=11)
    _assert_equals_twin(model, Y, logT, X, rows, Q)


@pytest.mark.parametrize("model,N,J", [("rtirt", 37, 1), ("mlirt", 37, 1), ("cross", 37, 65), ("latent", 37, 65), ("rtirt", 1, 9), ("null", 1, 9)])
def test_loglik_equals_twin_at_the_edges_of_the_shapes(model, N, J):
    rows = mu.make_rows(model, J, 3, 3, seed=5)
    Y, logT, X = mu.make_data(model, N, J, 3, seed=5)
    _assert_equals_twin(model, Y, logT, X, rows, 61)


def test_loglik_equals_twin_at_the_extremes():
    # one subject all correct against a_j = 8: B(theta) runs from -8 J |theta - b| to 0 over the nodes
    rows = mu.make_rows("rtirt", 9, 3, 3, seed=21, a=8.0)
    Y, logT, X = mu.make_data("rtirt", 37, 9, 3, seed=21)
    Y[5, :] = 1
    Y[6, :] = 0
    _assert_equals_twin("rtirt", Y, logT, X, rows, 61, what="all correct against a = 8")
    # terms down to -1400: logT of one subject 22 away from lambda, alternating in sign over the items (a common shift would be taken up by zeta)
    rows = mu.make_rows("cross", 9, 0, 3, seed=22)
    Y, logT, X = mu.make_data("cross", 37, 9, 0, seed=22)
    logT[3, :] += 22.0 * (-1.0) ** np.arange(9)
    dev = _assert_equals_twin("cross", Y, logT, None, rows, 61, what="far-off logT")
    assert dev["l"][3].min() < -1400.0
    # Sigma_p of correlation exactly 1: v = 1 - 2^2 / 4 = 0
    for model in ("rtirt", "null", "cross"):
        rows = mu.make_rows(model, 9, 3, 3, seed=23, sigp=[4.0, 2.0, 2.0, 1.0])
        Y, logT, X = mu.make_data(model, 37, 9, 3, seed=23)
        _assert_equals_twin(model, Y, logT, X, rows, 61, what=f"{model} correlation 1")
    rows = mu.make_rows("latent", 9, 3, 3, seed=23, sigp=[1.5, 0.0, 0.0, 0.0])      # Latent: v = Sigma_p[2,2] = 0
    Y, logT, X = mu.make_data("latent", 37, 9, 3, seed=23)
    _assert_equals_twin("latent", Y, logT, X, rows, 61, what="latent v = 0")


# ------------------------------------------------------------------------------------------------------------ independence
@pytest.mark.parametrize("model", ["rtirt", "cross"])
def test_a_subjects_result_depends_on_its_own_data_only(model):
    L = _pkg()._lib
    rows = mu.make_rows(model, 9, 3, 4, seed=31)
    Y, logT, X = mu.make_data(model, 600, 9, 3, seed=31)
    whole = L.marginal_loglik(mu.CODE[model], Y, logT, X, rows)
    for lo, hi in ((0, 256), (256, 600), (599, 600)):
        part = L.marginal_loglik(mu.CODE[model], Y[lo:hi], logT[lo:hi], X[lo:hi], rows)
        for k in ("l", "lppd", "p"):
            assert np.all(np.isfinite(part[k])) and np.array_equal(part[k], whole[k][lo:hi]), (k, lo, hi)


# ------------------------------------------------------------------------------------------------------------ the engine entry
def _assert_result_equals_loglik(got, model, data, rows, Q=61, what=""):
    """(totals, lppd, p) of an engine or farm entry against erm_marginal_loglik on the same data and rows."""
    L = _pkg()._lib
    Y, logT, X = data
    w, lppd, p = got
    ref = L.marginal_loglik(mu.CODE[model], Y, logT, X, rows, nodes=Q, want_l=False)
    elp = np.max(np.abs(lppd - ref["lppd"]) / np.maximum(np.abs(ref["lppd"]), LPPD_FLOOR))
    ep = np.max(np.abs(p - ref["p"]) / np.abs(ref["p"]))
    print(f"{what}: rows {w['nRows']}, max rel err lppd_i {elp:.3g}, p_i {ep:.3g}; " + ", ".join(f"{k} {w[k]!r} / {ref['totals'][k]!r}" for k in TOTALS) + f"; coarse {w['nCoarse']}")
    assert elp <= TOL and ep <= TOL
    for k in TOTALS:
        assert abs(w[k] - ref["totals"][k]) <= TOL * abs(ref["totals"][k]), k
    for k in ("nUnits", "nRows", "nNodes", "nHighVar", "nCoarse"):
        assert w[k] == ref["totals"][k], k


@pytest.mark.parametrize("full", [True, False], ids=["full", "summary"])
@pytest.mark.parametrize("precision", ["f64", "f32"])
@pytest.mark.parametrize("model", ["rtirt", "cross"])
def test_engine_entry_equals_loglik_on_its_own_data_and_rows(model, precision, full):
    """600 x 9, 40 sweeps as two interleaved chains of 20 with 10 burn-in iterations: the rows are rows >= 20 of the item trace.  Not bit for bit: the engine holds
    logT centred by its column means and adds them back."""
    Y, logT, X, init, tp = pu.make_problem(model, 600, 9, 3, seed=41)
    eng = _engine(model, Y, logT, X, init, n_iter=20, n_chain=2, n_burnin=10, precision=precision, full=full)
    eng.run(40)
    got = eng.marginal_waic(pointwise=True)
    assert got[0]["nRows"] == eng.post_count == 20 and got[0]["nUnits"] == 600
    _assert_result_equals_loglik(got, model, eng.get_data(), eng.item_trace()[20:], what=f"{model} {precision} {'full' if full else 'summary'}")
    assert _bytes(eng.marginal_waic(pointwise=True)) == _bytes(got)                       # twice
    split = _engine(model, Y, logT, X, init, n_iter=20, n_chain=2, n_burnin=10, precision=precision, full=full)
    split.run(17)
    split.run(23)
    assert _bytes(split.marginal_waic(pointwise=True)) == _bytes(got)
    assert eng.marginal_waic() == got[0]                                                  # without the pointwise vectors: the same totals
    eng.close()
    split.close()


def test_engine_entry_only_reads_the_engine():
    L = _pkg()._lib
    Y, logT, X, init, tp = pu.make_problem("rtirt", 600, 9, 3, seed=43)
    eng = _engine("rtirt", Y, logT, X, init, n_iter=12, n_burnin=5, unit="subject")
    eng.run(12)

    def everything():
        parts = [eng.item_trace(), eng.trace(L.TRACE_LOGLIKE), eng.trace(L.TRACE_RA), eng.trace(L.TRACE_RT), eng.trace(L.TRACE_QR), *eng.pointwise()]
        for d in (eng.get_mean(), eng.get_state()):
            parts += [v for _, v in sorted(d.items()) if v is not None]
        return [np.ascontiguousarray(p).tobytes() for p in parts], eng.waic(), eng.post_count, eng.rows_done

    before = everything()
    eng.marginal_waic(pointwise=True)
    eng.marginal_waic(nodes=127)
    assert everything() == before
    eng.close()


# ------------------------------------------------------------------------------------------------------------ the farm
@pytest.mark.parametrize("nch", [2, 3])
def test_farm_equals_loglik_on_the_chain_major_rows(nch):
    Y, logT, X, init, tp = pu.make_problem("rtirt", 600, 9, 3, seed=47)
    farm = _farm("rtirt", [0] * nch, Y, logT, X, init, n_iter=14, n_burnin=6)
    farm.run(14)
    rows = np.concatenate([farm.engine(l).item_trace()[6:] for l in range(nch)], axis=0)
    got = farm.marginal_waic(pointwise=True)
    assert got[0]["nRows"] == farm.post_count == 8 * nch
    _assert_result_equals_loglik(got, "rtirt", farm.engine(0).get_data(), rows, what=f"farm of {nch}")
    assert _bytes(farm.marginal_waic(pointwise=True)) == _bytes(got)
    farm.close()


def test_farm_of_one_chain_equals_its_engine_bit_for_bit():
    Y, logT, X, init, tp = pu.make_problem("latent", 600, 9, 3, seed=49)
    farm = _farm("latent", [0], Y, logT, X, init, n_iter=14, n_burnin=6)
    farm.run(14)
    assert _bytes(farm.marginal_waic(pointwise=True)) == _bytes(farm.engine(0).marginal_waic(pointwise=True))
    farm.close()


def test_get_waic_marginal_on_samplers_and_compare_waic():
    """Through the public interface: a devices= sampler (the farm's entry) and a single-engine sampler (the engine's), each against the numpy twin on its own rows;
    compareWaic accepts two farm results."""
    pkg = _pkg()
    Y, logT, X, init, tp = pu.make_problem("rtirt", 300, 9, 3, seed=51)
    Cond = pkg.setCond(nSubj=300, nItem=9, nFeat=3, nIter=16, nChain=2, qRt=0.85)
    fits = {}
    for cls in ("GibbsRtIrt", "GibbsRtIrtNull"):
        M = getattr(pkg, cls)(Cond, Data=pkg.InputData(Y=Y, T=np.exp(logT), X=X), trace="summary")
        pkg.sample_b(M, devices=[0, 0])
        w = pkg.getWaicMarginal(M, pointwise=True)
        host = pkg.getWaicMarginalHost(M)
        assert w.unit == host.unit == "subject-marginal" and w.nNodes == 61 and w.nCoarse == host.nCoarse == 0 and w.nRows == host.nRows == 16 and w.nUnits == 300
        assert np.max(np.abs(w.lppd_u - host.lppd_u) / np.maximum(np.abs(host.lppd_u), LPPD_FLOOR)) <= TOL and abs(w.elpd - host.elpd) <= TOL * abs(host.elpd)
        assert pkg.getWaicMarginal(M).elpd == w.elpd and pkg.getWaicMarginal(M).lppd_u is None
        with pytest.raises(ValueError, match="devices="):
            pkg.getWaic(M)                                   # the conditional WAIC stays refused for a farm
        fits[cls] = (M, w)
    c = pkg.compareWaic(fits["GibbsRtIrt"][1], fits["GibbsRtIrtNull"][1])
    assert c["unit"] == "subject-marginal" and c["nUnits"] == 300 and np.isfinite(c["elpd_diff"]) and c["se_diff"] > 0.0
    for M, _ in fits.values():
        M.close()
    M = pkg.GibbsRtIrt(Cond, Data=pkg.InputData(Y=Y, T=np.exp(logT), X=X))
    pkg.sample_b(M)
    w, host = pkg.getWaicMarginal(M, nodes=41, pointwise=True), pkg.getWaicMarginalHost(M, nodes=41)
    assert w.nRows == host.nRows == 16 and w.nNodes == host.nNodes == 41 and abs(w.elpd - host.elpd) <= TOL * abs(host.elpd)
    assert np.max(np.abs(w.p_u - host.p_u) / np.abs(host.p_u)) <= TOL
    M.close()


# ------------------------------------------------------------------------------------------------------------ refusals
def test_every_refusal_returns_its_code_and_leaves_the_engine_usable():
    L = _pkg()._lib
    lib = L.load()
    err = lambda: lib.erm_last_error().decode()
    out = np.zeros(10)
    Y, logT, X, init, tp = pu.make_problem("rtirt", 500, 9, 3, seed=31)
    eng = _engine("rtirt", Y, logT, X, init, n_iter=6, n_burnin=2)
    call = lambda e, n=0: lib.erm_get_marginal_waic(e._h, n, out.ctypes.data, None, None)
    assert call(eng) == -3 and "two post-burn-in rows" in err()                          # ERM_ERR_STATE: nothing recorded
    eng.run(3)                                                                           # rows 0, 1 burn-in, one post-burn-in row
    assert call(eng) == -3 and "two post-burn-in rows" in err()
    eng.run(3)
    for bad in (60, 1, 1027, -3):
        assert call(eng, bad) == -1 and "odd" in err()                                   # ERM_ERR_ARG
    assert lib.erm_get_marginal_waic(eng._h, 0, None, None, None) == -1
    assert call(eng) == 0 and out[5] == 500 and out[6] == 4 and out[8] == 61
    assert call(eng, 3) == 0 and out[8] == 3 and out[9] == 500                           # three nodes: every unit is coarse
    eng.close()
    # the quantile models
    for model in ("crossqr", "latentqr"):
        Yq, lq, Xq, iq, _ = pu.make_problem(model, 200, 7, 3, seed=33)
        q = _engine(model, Yq, lq, Xq, iq, n_iter=6, n_burnin=2)
        q.run(4)
        assert call(q) == -1 and "quantile" in err()
        q.run(2)
        q.close()
    # a subject-sharded engine
    sh = L.Engine(model=L.MODEL_RTIRT, n_item=9, n_subj=500, n_feat=3, n_iter=6, n_chain=1, n_burnin=2, cov2one=1, q_rt=0.5, seed=1, precision=L.PREC_F64, trace_mode=0)
    sh.set_shard(0, 1, 500, 0, lambda s, r, n: lib.erm_copy(r, s, n))
    sh.set_data(Y, logT, X)
    sh.set_state(**init)
    sh.run(4)
    assert call(sh) == -3 and "shard" in err()
    sh.run(2)
    sh.close()
    # the farm: a quantile model, too few rows, a bad node count -- and it runs on
    farm = _farm("rtirt", [0, 0], Y, logT, X, init, n_iter=6, n_burnin=2)
    fcall = lambda n=0: lib.erm_farm_get_marginal_waic(farm._h, n, out.ctypes.data, None, None)
    farm.run(3)
    assert fcall() == -3 and "chain 0" in err() and "two post-burn-in rows" in err()
    assert fcall(8) == -1
    farm.run(3)
    assert fcall() == 0 and out[6] == 8
    farm.close()
    # erm_marginal_loglik
    rows = mu.make_rows("rtirt", 9, 3, 3, seed=1)
    Ys, ls, Xs = mu.make_data("rtirt", 5, 9, 3, seed=1)
    code = lambda f: int(str(f.value).split()[2].rstrip(":"))
    with pytest.raises(L.ErmError, match="NaN in row 1") as e:
        bad = rows.copy(); bad[1, 4] = np.nan
        L.marginal_loglik(1, Ys, ls, Xs, bad)
    assert code(e) == -4                                                                 # ERM_ERR_NONFINITE
    with pytest.raises(L.ErmError, match="NaN in logT") as e:
        lb = ls.copy(); lb[2, 3] = np.nan
        L.marginal_loglik(1, Ys, lb, Xs, rows)
    assert code(e) == -4
    with pytest.raises(L.ErmError, match="row 2: sig2t") as e:
        bad = rows.copy(); bad[2, 3 * 9 + 1] = 0.0
        L.marginal_loglik(1, Ys, ls, Xs, bad)
    assert code(e) == -1
    with pytest.raises(L.ErmError, match=r"row 0: Sigma_p\[1,1\]") as e:
        bad = rows.copy(); bad[0, -4] = 0.0
        L.marginal_loglik(1, Ys, ls, Xs, bad)
    assert code(e) == -1
    with pytest.raises(L.ErmError, match="row 1: the conditional variance") as e:
        bad = rows.copy(); bad[1, -4:] = [1.0, 2.0, 2.0, 1.0]
        L.marginal_loglik(1, Ys, ls, Xs, bad)
    assert code(e) == -1
    with pytest.raises(L.ErmError, match="n_rows") as e:
        L.marginal_loglik(1, Ys, ls, Xs, rows[:1])                                      # the WAIC outputs need two rows
    assert code(e) == -1
    one = L.marginal_loglik(1, Ys, ls, Xs, rows[:1], want_waic=False)                     # l alone does not
    assert one["l"].shape == (5, 1) and np.array_equal(one["l"][:, 0], L.marginal_loglik(1, Ys, ls, Xs, rows)["l"][:, 0])
    with pytest.raises(L.ErmError, match="quantile") as e:
        L.marginal_loglik(L.MODEL_CROSSQR, Ys, ls, None, np.zeros((2, 5 * 9 + 4)))
    assert code(e) == -1


# ------------------------------------------------------------------------------------------------------------ it discriminates
def test_marginal_waic_prefers_2pl_over_1pl_on_spread_discriminations():
    """GibbsMlIrt itemtype "2pl" against "1pl" on waic_util.spread_problem() (600 x 12, discriminations 0.25 ... 3), 200 sweeps, through the public interface."""
    pkg = _pkg()
    Y, X, init = wu.spread_problem()
    Cond = pkg.setCond(nSubj=wu.SPREAD_N, nItem=wu.SPREAD_J, nFeat=1, nIter=wu.SPREAD_ITER, nChain=1)
    fits = {}
    for itemtype in ("2pl", "1pl"):
        M = pkg.GibbsMlIrt(Cond, Data=pkg.InputData(Y=Y, X=X), trace="summary")
        pkg.sample_b(M, itemtype=itemtype, fill=False)
        fits[itemtype] = (M, pkg.getWaicMarginal(M, pointwise=True))
        assert fits[itemtype][1].nCoarse == 0 and fits[itemtype][1].nRows == wu.SPREAD_ITER // 2
    c = pkg.compareWaic(fits["2pl"][1], fits["1pl"][1])
    print(f"2pl {fits['2pl'][1]}\n1pl {fits['1pl'][1]}\n2pl - 1pl: elpd_diff {c['elpd_diff']:.4f}, se_diff {c['se_diff']:.4f}, margin {c['elpd_diff'] / c['se_diff']:.2f} se_diff")
    assert c["elpd_diff"] > 2.0 * c["se_diff"] > 0.0
    for M, _ in fits.values():
        M.close()

"""Scores of respondents on the device (erm_get_scores / erm_farm_get_scores / erm_score).
  1. erm_score against scoresHost, the numpy twin (itself pinned to scipy's quad in tests/test_score_host.py), under both weightings: every column to 1e-10 -- the
     project's device-against-numpy tolerance (tests/test_gpu_marginal_waic.py) -- relative to max(|ref|, 1); COARSE, row_ess under equal weights and out4 exactly.
     Five models at 37 x 9 with 3 rows, Q in {3, 61, 127}, F = 3 and one case at F = 0; J = 1, J = 65 (a lane takes nine items), N = 1, one row; and the three
     extremes of tests/test_gpu_marginal_waic.py: all correct against a_j = 8, logT 22 off with alternating sign (under likelihood weights that subject's row_ess is
     finite and below 1.01 x its twin value), v = 0 for RtIrt, Null, Cross and Latent.
  2. independence: a subject's seven outputs are bit-identical whether it is computed among 600 subjects, among a part of them or alone (tile tails included).
  3. the engine entry against erm_score on erm_get_data's data set and the post-burn-in rows of erm_get_item_trace: fp64 and fp32 engines, both trace modes, two
     interleaved chains (1e-10, not bit for bit: the engine holds logT centred); bit-identical when called twice and when the sweeps are split 17 + 23; the state,
     the traces, erm_get_waic's accumulators and the marginal WAIC's result are unchanged by the call.
  4. the farm: two and three chains on one device against erm_score on the chain-major concatenation of the chains' rows; one chain equals its engine bit for
     bit; getScores on a devices= sampler.
  5. every refusal returns its code, and the engine or farm runs on afterwards.
  6. agreement with the chain, GibbsMlIrt only, sampled on the device: the two conditions of tests/test_score_host.py, and r <= 3 x the value measured there on
     the CPU (0.1348; the device draws another stream, the factor covers the change of Monte-Carlo noise)."""
import numpy as np
import pytest

import marginal_util as mu
import parity_util as pu
import score_util as su
import waic_util as wu
from item_pass_util import _bytes, _engine, _farm, _kernel_x, _pkg

pytestmark = pytest.mark.gpu

TOL = 1e-10
R_CPU = 0.1348          # tests/test_score_host.py::test_scores_agree_with_the_chain_for_mlirt
WEIGHTINGS = ("equal", "likelihood")
COLUMNS = su.COLS + ("coarse",)


def _errors(dev, ref, rt):
    """Per column the largest |dev - ref| / max(|ref|, 1); NaN columns (no zeta) must be NaN on the device too."""
    get = lambda o, c: np.asarray(o[c] if isinstance(o, dict) else getattr(o, c), dtype=np.float64)
    err = {}
    for c in su.COLS:
        d, r = get(dev, c), get(ref, c)
        if not rt and c in ("zeta", "zetaSd", "cov"):
            assert np.all(np.isnan(d)) and np.all(np.isnan(r)), c
            continue
        assert np.all(np.isfinite(d)), c
        err[c] = float(np.max(np.abs(d - r) / np.maximum(np.abs(r), 1.0)))
    return err


def _assert_equals_twin(model, Y, logT, X, rows, Q, what=""):
    """erm_score against scoresHost under both weightings; returns {weighting: (device dict, twin)}."""
    pkg = _pkg()
    out = {}
    for weighting in WEIGHTINGS:
        dev = pkg._lib.score(mu.CODE[model], Y, logT, X, rows, nodes=Q, weighting=weighting)
        host = pkg.scoresHost(mu.CODE[model], Y, logT, _kernel_x(model, X), rows, Q, weighting)
        err = _errors(dev, host, model != "mlirt")
        print(f"{what or model} N={Y.shape[0]} J={Y.shape[1]} Q={Q} {weighting}: " + ", ".join(f"{c} {e:.3g}" for c, e in err.items()) + f"; coarse {dev['nCoarse']}")
        assert all(e <= TOL for e in err.values()), err
        assert np.array_equal(dev["coarse"], host.coarse) and dev["nCoarse"] == host.nCoarse == int(np.sum(dev["coarse"]))
        assert (dev["nSubj"], dev["nRows"], dev["nNodes"]) == (Y.shape[0], rows.shape[0], Q)
        if weighting == "equal":
            assert np.all(dev["rowEss"] == rows.shape[0])
        out[weighting] = (dev, host)
    return out


# ------------------------------------------------------------------------------------------------------------ the kernel against the twin
@pytest.mark.parametrize("Q", [3, 61, 127])
@pytest.mark.parametrize("model", mu.MODELS)
def test_scores_equal_twin(model, Q):
    F = 0 if (model, Q) == ("rtirt", 127) else 3
    rows = mu.make_rows(model, 9, F, 3, seed=11)
    Y, logT, X = mu.make_data(model, 37, 9, F, seed=11)
    _assert_equals_twin(model, Y, logT, X, rows, Q)


@pytest.mark.parametrize("model,N,J,R", [("rtirt", 37, 1, 3), ("mlirt", 37, 1, 3), ("cross", 37, 65, 3), ("latent", 37, 65, 3), ("rtirt", 1, 9, 3), ("null", 1, 9, 3),
                                         ("rtirt", 37, 9, 1), ("mlirt", 37, 9, 1), ("cross", 37, 9, 1)])
def test_scores_equal_twin_at_the_edges_of_the_shapes(model, N, J, R):
    rows = mu.make_rows(model, J, 3, R, seed=5)
    Y, logT, X = mu.make_data(model, N, J, 3, seed=5)
    got = _assert_equals_twin(model, Y, logT, X, rows, 61)
    if R == 1:
        assert np.all(got["likelihood"][0]["rowEss"] == 1.0)
        for c in COLUMNS:      # one row: its weight is 1 under either weighting
            assert np.array_equal(got["likelihood"][0][c], got["equal"][0][c], equal_nan=True), c


def test_scores_equal_twin_at_the_extremes():
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
    dev, host = _assert_equals_twin("cross", Y, logT, None, rows, 61, what="far-off logT")["likelihood"]
    assert np.isfinite(dev["rowEss"][3]) and dev["rowEss"][3] < 1.01 * host.rowEss[3]
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
def test_a_subjects_scores_depend_on_its_own_data_only(model):
    L = _pkg()._lib
    rows = mu.make_rows(model, 9, 3, 4, seed=31)
    Y, logT, X = mu.make_data(model, 600, 9, 3, seed=31)
    for weighting in WEIGHTINGS:
        whole = L.score(mu.CODE[model], Y, logT, X, rows, weighting=weighting)
        for lo, hi in ((0, 256), (256, 600), (599, 600)):
            part = L.score(mu.CODE[model], Y[lo:hi], logT[lo:hi], X[lo:hi], rows, weighting=weighting)
            for c in COLUMNS:
                assert np.all(np.isfinite(part[c])) and np.array_equal(part[c], whole[c][lo:hi]), (c, lo, hi, weighting)


# ------------------------------------------------------------------------------------------------------------ the engine entry
def _assert_result_equals_score(got, model, data, rows, Q=61, what=""):
    """The dict of an engine or farm entry against erm_score on the same data and rows, equal weights."""
    Y, logT, X = data
    ref = _pkg()._lib.score(mu.CODE[model], Y, logT, X, rows, nodes=Q)
    err = _errors(got, ref, model != "mlirt")
    print(f"{what}: rows {got['nRows']}, " + ", ".join(f"{c} {e:.3g}" for c, e in err.items()) + f"; coarse {got['nCoarse']}")
    assert all(e <= TOL for e in err.values()), err
    assert np.array_equal(got["coarse"], ref["coarse"])
    for k in ("nSubj", "nRows", "nNodes", "nCoarse"):
        assert got[k] == ref[k], k


@pytest.mark.parametrize("full", [True, False], ids=["full", "summary"])
@pytest.mark.parametrize("precision", ["f64", "f32"])
@pytest.mark.parametrize("model", ["rtirt", "cross"])
def test_engine_entry_equals_score_on_its_own_data_and_rows(model, precision, full):
    """600 x 9, 40 sweeps as two interleaved chains of 20 with 10 burn-in iterations: the rows are rows >= 20 of the item trace."""
    Y, logT, X, init, tp = pu.make_problem(model, 600, 9, 3, seed=41)
    eng = _engine(model, Y, logT, X, init, n_iter=20, n_chain=2, n_burnin=10, precision=precision, full=full)
    eng.run(40)
    got = eng.scores()
    assert got["nRows"] == eng.post_count == 20 and got["nSubj"] == 600 and np.all(got["rowEss"] == 20.0)
    _assert_result_equals_score(got, model, eng.get_data(), eng.item_trace()[20:], what=f"{model} {precision} {'full' if full else 'summary'}")
    assert _bytes(eng.scores()) == _bytes(got)                                            # twice
    split = _engine(model, Y, logT, X, init, n_iter=20, n_chain=2, n_burnin=10, precision=precision, full=full)
    split.run(17)
    split.run(23)
    assert _bytes(split.scores()) == _bytes(got)
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
        w, lppd_i, p_i = eng.marginal_waic(pointwise=True)
        return [np.ascontiguousarray(v).tobytes() for v in parts + [lppd_i, p_i]], w, eng.waic(), eng.post_count, eng.rows_done

    before = everything()
    eng.scores()
    eng.scores(nodes=127)
    assert everything() == before
    eng.close()


# ------------------------------------------------------------------------------------------------------------ the farm
@pytest.mark.parametrize("nch", [2, 3])
def test_farm_equals_score_on_the_chain_major_rows(nch):
    Y, logT, X, init, tp = pu.make_problem("rtirt", 600, 9, 3, seed=47)
    farm = _farm("rtirt", [0] * nch, Y, logT, X, init, n_iter=14, n_burnin=6)
    farm.run(14)
    rows = np.concatenate([farm.engine(l).item_trace()[6:] for l in range(nch)], axis=0)
    got = farm.scores()
    assert got["nRows"] == farm.post_count == 8 * nch
    _assert_result_equals_score(got, "rtirt", farm.engine(0).get_data(), rows, what=f"farm of {nch}")
    assert _bytes(farm.scores()) == _bytes(got)
    farm.close()


def test_farm_of_one_chain_equals_its_engine_bit_for_bit():
    Y, logT, X, init, tp = pu.make_problem("latent", 600, 9, 3, seed=49)
    farm = _farm("latent", [0], Y, logT, X, init, n_iter=14, n_burnin=6)
    farm.run(14)
    assert _bytes(farm.scores()) == _bytes(farm.engine(0).scores())
    farm.close()


def test_get_scores_on_samplers():
    """Through the public interface: a devices= sampler (the farm's entry) and a single-engine sampler (the engine's), each against the numpy twin on its own rows."""
    pkg = _pkg()
    Y, logT, X, init, tp = pu.make_problem("rtirt", 300, 9, 3, seed=51)
    Cond = pkg.setCond(nSubj=300, nItem=9, nFeat=3, nIter=16, nChain=2, qRt=0.85)
    for devices, nodes in (([0, 0], 61), (None, 41)):
        M = pkg.GibbsRtIrt(Cond, Data=pkg.InputData(Y=Y, T=np.exp(logT), X=X), trace="summary")
        pkg.sample_b(M, devices=devices)
        sc = pkg.getScores(M, nodes=nodes)
        host = pkg.scoresHost(M._model, M.Data.Y, M.Data.logT, np.asarray(M.Data.X, dtype=np.float64), pkg.gibbs.marginalRows(M), nodes)
        err = _errors(sc, host, True)
        print(f"getScores devices={devices}: " + ", ".join(f"{c} {e:.3g}" for c, e in err.items()) + f"; {sc}")
        assert all(e <= TOL for e in err.values()), err
        assert sc.nRows == 16 and sc.nNodes == nodes and sc.nCoarse == host.nCoarse == 0 and sc.theta.shape == (300,) and np.all(sc.rowEss == 16.0)
        assert 0.0 < sc.relTheta < 1.0 and 0.0 < sc.relZeta < 1.0 and abs(sc.relTheta - host.relTheta) <= TOL and abs(sc.relZeta - host.relZeta) <= TOL
        M.close()
    sr = pkg.scoreRespondents(1, Y[:5], logT[:5], X[:5], mu.make_rows("rtirt", 9, 3, 3, seed=1), weighting="likelihood")
    assert sr.weighting == "likelihood" and sr.theta.shape == (5,) and np.all((sr.rowEss >= 1.0) & (sr.rowEss <= 3.0))


# ------------------------------------------------------------------------------------------------------------ refusals
def test_every_refusal_returns_its_code_and_leaves_the_engine_usable():
    L = _pkg()._lib
    lib = L.load()
    err = lambda: lib.erm_last_error().decode()
    out, sc = np.zeros(4), np.zeros((7, 500))
    Y, logT, X, init, tp = pu.make_problem("rtirt", 500, 9, 3, seed=31)
    eng = _engine("rtirt", Y, logT, X, init, n_iter=6, n_burnin=2)
    call = lambda e, n=0: lib.erm_get_scores(e._h, n, sc.ctypes.data, out.ctypes.data)
    assert call(eng) == -3 and "one post-burn-in row" in err()                           # ERM_ERR_STATE: nothing recorded
    eng.run(2)                                                                           # rows 0, 1: burn-in
    assert call(eng) == -3 and "one post-burn-in row" in err()
    eng.run(1)                                                                           # one post-burn-in row is enough
    assert call(eng) == 0 and list(out) == [500, 1, 61, out[3]] and np.all(sc[5] == 1.0)
    eng.run(3)
    for bad in (60, 1, 1027, -3):
        assert call(eng, bad) == -1 and "odd" in err()                                   # ERM_ERR_ARG
    assert lib.erm_get_scores(eng._h, 0, None, out.ctypes.data) == -1
    assert lib.erm_get_scores(eng._h, 0, sc.ctypes.data, None) == 0                      # out4 may be NULL
    assert call(eng) == 0 and list(out[:3]) == [500, 4, 61]
    assert call(eng, 3) == 0 and out[2] == 3 and out[3] == 500 and np.all(sc[6] == 1.0)  # three nodes: every unit is coarse
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
    # the farm: no post-burn-in row, a bad node count -- and it runs on
    farm = _farm("rtirt", [0, 0], Y, logT, X, init, n_iter=6, n_burnin=2)
    fcall = lambda n=0: lib.erm_farm_get_scores(farm._h, n, sc.ctypes.data, out.ctypes.data)
    farm.run(2)
    assert fcall() == -3 and "chain 0" in err() and "one post-burn-in row" in err()
    assert fcall(8) == -1
    farm.run(4)
    assert fcall() == 0 and out[1] == 8
    farm.close()
    # erm_score
    rows = mu.make_rows("rtirt", 9, 3, 3, seed=1)
    Ys, ls, Xs = mu.make_data("rtirt", 5, 9, 3, seed=1)
    code = lambda f: int(str(f.value).split()[2].rstrip(":"))
    with pytest.raises(L.ErmError, match="NaN in row 1") as e:
        bad = rows.copy(); bad[1, 4] = np.nan
        L.score(1, Ys, ls, Xs, bad)
    assert code(e) == -4                                                                 # ERM_ERR_NONFINITE
    with pytest.raises(L.ErmError, match="NaN in logT") as e:
        lb = ls.copy(); lb[2, 3] = np.nan
        L.score(1, Ys, lb, Xs, rows)
    assert code(e) == -4
    with pytest.raises(L.ErmError, match="NaN in X") as e:
        xb = Xs.copy(); xb[4, 0] = np.nan
        L.score(1, Ys, ls, xb, rows)
    assert code(e) == -4
    with pytest.raises(L.ErmError, match="row 2: sig2t") as e:
        bad = rows.copy(); bad[2, 3 * 9 + 1] = 0.0
        L.score(1, Ys, ls, Xs, bad)
    assert code(e) == -1
    with pytest.raises(L.ErmError, match="row 1: sig2t") as e:
        bad = rows.copy(); bad[1, 3 * 9 + 8] = -0.25
        L.score(1, Ys, ls, Xs, bad)
    assert code(e) == -1
    with pytest.raises(L.ErmError, match="row 1: the conditional variance") as e:
        bad = rows.copy(); bad[1, -4:] = [1.0, 2.0, 2.0, 1.0]
        L.score(1, Ys, ls, Xs, bad)
    assert code(e) == -1
    with pytest.raises(L.ErmError, match="n_rows") as e:
        L.score(1, Ys, ls, Xs, rows[:0])
    assert code(e) == -1
    with pytest.raises(L.ErmError, match="quantile") as e:
        L.score(L.MODEL_CROSSQR, Ys, ls, None, np.zeros((2, 5 * 9 + 4)))
    assert code(e) == -1
    s5, o4 = np.zeros((7, 5)), np.zeros(4)
    Yf, lf, Xf = np.asfortranarray(Ys), np.asfortranarray(ls), np.asfortranarray(Xs)
    raw = lambda Q, w: lib.erm_score(0, 1, 5, 9, 3, Yf.ctypes.data, lf.ctypes.data, Xf.ctypes.data, rows.ctypes.data, 3, Q, w, s5.ctypes.data, o4.ctypes.data)
    for w in (2, -1, 7):
        assert raw(61, w) == -1 and "weighting" in err()                                 # an unknown weighting
    for Q in (60, 1, 1027):
        assert raw(Q, 0) == -1 and "odd" in err()                                        # an even Q, Q out of range
    assert raw(0, 1) == 0 and list(o4[:3]) == [5, 3, 61] and np.all(np.isfinite(s5))      # and the device runs on


# ------------------------------------------------------------------------------------------------------------ it agrees with the chain where it must
def test_scores_agree_with_the_chain_for_mlirt():
    """GibbsMlIrt on waic_util.spread_problem() (600 x 12), 200 sweeps on the device, through the public interface: getScores against Post.mean and the sample sd
    of theta's post-burn-in draws."""
    pkg = _pkg()
    Y, X, init = wu.spread_problem()
    Cond = pkg.setCond(nSubj=wu.SPREAD_N, nItem=wu.SPREAD_J, nFeat=1, nIter=wu.SPREAD_ITER, nChain=1)
    M = pkg.GibbsMlIrt(Cond, Data=pkg.InputData(Y=Y, X=X), trace="full")
    pkg.sample_b(M)
    sc = pkg.getScores(M)
    draws = M.Post.ra[Cond.nBurnin:, :wu.SPREAD_N, 0]
    assert draws.shape[0] == sc.nRows == wu.SPREAD_ITER // 2 and np.max(np.abs(draws.mean(axis=0) - M.Post.mean.theta)) <= 1e-9
    r, ratio = su.chain_agreement(sc, draws)
    print(f"r = {r:.4f} (CPU {R_CPU}), median sd of the draws / median thetaSd = {ratio:.4f}; relTheta {sc.relTheta:.4f}, coarse {sc.nCoarse}")
    assert sc.nCoarse == 0 and np.all(np.isnan(sc.zeta)) and np.isnan(sc.relZeta)
    assert r <= 0.5 and abs(np.log(ratio)) <= np.log(1.1) and r <= 3.0 * R_CPU
    M.close()

"""Plausible values on the device (erm_get_plausible_values / erm_farm_get_plausible_values / erm_plausible_values).
  1. erm_plausible_values against plausibleValuesHost, the numpy twin (itself pinned to scoresHost in tests/test_pv_host.py), at pv_util.CASES: five models at
     N = 70 (two full tiles and a part tile), J = 5 and 9, Q = 9, 61 and 129, K = 1, 5 and 3 x rows, rows = 1 and 7.  node equal everywhere; theta and zeta to 1e-10
     relative to max(|ref|, 1) -- the project's device-against-numpy tolerance (tests/test_gpu_scores.py); out4 and the coarse flags exactly.  The nodes can be
     demanded equal because at the cases' seeds the twin has no draw whose two best keys lie closer than pv_util.GAP_MIN = 1e-8 (checked on the CPU in
     tests/test_pv_host.py, asserted again here): no draw is left out.
  2. independence: a subject's draws are bit-identical alone and among others, with other subjects behind it, with the chunk cap (ERM_PV_CHUNK) forced to 1, 32
     and 33 subjects, and when called twice; another seed changes them.
  3. the engine entry against erm_plausible_values on erm_get_data's data set and the post-burn-in rows of erm_get_item_trace: fp64 and fp32 engines, both trace
     modes (1e-10 and equal nodes, not bit for bit: the engine holds logT centred); bit-identical when called twice, under a small chunk cap and when the sweeps
     are split 17 + 23; the state, the traces and erm_get_scores are unchanged by the call.
  4. the farm: one chain equals its engine bit for bit; two chains on one device against erm_plausible_values on the chain-major table; getPlausibleValues on a
     devices= sampler and on a single engine, drawPlausibleValues.
  5. every refusal returns its code, and the engine or farm runs on afterwards."""
import numpy as np
import pytest

import marginal_util as mu
import parity_util as pu
import pv_util as pvu
from item_pass_util import _bytes, _engine, _farm, _pkg

pytestmark = pytest.mark.gpu

TOL = 1e-10
ARRAYS = ("theta", "zeta", "node", "coarse")
COUNTS = ("nSubj", "nRows", "nNodes", "nCoarse")


def _get(o, c):
    return np.asarray(o[c] if isinstance(o, dict) else getattr(o, c))


def _assert_equal_draws(dev, ref, rt, what):
    """node and the coarse flags exactly; theta and zeta to TOL relative to max(|ref|, 1), zeta NaN on both sides for a model without zeta."""
    assert np.array_equal(_get(dev, "node"), _get(ref, "node")), what
    assert np.array_equal(_get(dev, "coarse"), _get(ref, "coarse")), what
    err = {}
    for c in ("theta", "zeta"):
        d, r = _get(dev, c), _get(ref, c)
        assert d.shape == r.shape
        if c == "zeta" and not rt:
            assert np.all(np.isnan(d)) and np.all(np.isnan(r)), what
            continue
        assert np.all(np.isfinite(d)), (what, c)
        err[c] = float(np.max(np.abs(d - r) / np.maximum(np.abs(r), 1.0)))
    print(f"{what}: " + ", ".join(f"{c} {e:.3g}" for c, e in err.items()))
    assert all(e <= TOL for e in err.values()), (what, err)


# ------------------------------------------------------------------------------------------------------------ the kernel against the twin
@pytest.mark.parametrize("model,J,Q,K,R", pvu.CASES)
def test_plausible_values_equal_twin(model, J, Q, K, R):
    pkg = _pkg()
    Y, logT, X, rows = pvu.case_problem(model, J, R)
    host, gap = pkg.plausibleValuesHost(mu.CODE[model], Y, logT, X, rows, K, pvu.CASE_SEED, Q, with_gap=True)
    assert gap.min() >= pvu.GAP_MIN                                                       # the condition on the inputs: every draw is decidable
    dev = pkg._lib.plausible_values(mu.CODE[model], Y, logT, X, rows, K=K, seed=pvu.CASE_SEED, nodes=Q)
    _assert_equal_draws(dev, host, model != "mlirt", f"{model} J={J} Q={Q} K={K} R={R} (smallest gap {gap.min():.3g}, coarse {dev['nCoarse']})")
    assert (dev["nSubj"], dev["nRows"], dev["nNodes"], dev["nCoarse"], dev["seed"]) == (pvu.CASE_N, R, Q, host.nCoarse, pvu.CASE_SEED)
    assert dev["nCoarse"] == int(np.sum(dev["coarse"])) and dev["node"].dtype == np.int32 and dev["node"].min() >= 0 and dev["node"].max() < Q
    wrapped = pkg.drawPlausibleValues(mu.CODE[model], Y, logT, X, rows, K, pvu.CASE_SEED, Q)
    assert np.array_equal(wrapped.theta, dev["theta"]) and np.array_equal(wrapped.node, dev["node"]) and wrapped.nCoarse == dev["nCoarse"]


# ------------------------------------------------------------------------------------------------------------ independence
@pytest.mark.parametrize("model", ["rtirt", "cross", "mlirt"])
def test_a_subjects_draws_depend_on_its_own_data_and_index_only(model, monkeypatch):
    L = _pkg()._lib
    Y, logT, X, rows = pvu.case_problem(model, 9, 7)
    sl = lambda a, s: None if a is None else a[s]
    call = lambda s, seed=pvu.CASE_SEED, K=5: L.plausible_values(mu.CODE[model], Y[s], sl(logT, s), sl(X, s), rows, K=K, seed=seed)
    whole = call(slice(None))
    assert _bytes(call(slice(None))) == _bytes(whole)                                      # twice
    alone, head = call(slice(0, 1)), call(slice(0, 33))                                    # N = 1 against N = 70; one tile and one subject of the next
    for c in ARRAYS:
        assert np.array_equal(alone[c], whole[c][:1], equal_nan=True) and np.array_equal(head[c], whole[c][:33], equal_nan=True), c
    perm = np.concatenate([[0], np.arange(69, 0, -1)])                                     # the same subject 0 with the others in another order behind it
    mixed = L.plausible_values(mu.CODE[model], Y[perm], sl(logT, perm), sl(X, perm), rows, K=5, seed=pvu.CASE_SEED)
    for c in ARRAYS:
        assert np.array_equal(mixed[c][:1], whole[c][:1], equal_nan=True), c
    assert not np.array_equal(mixed["theta"][1], whole["theta"][69])                       # the index is part of the stream: subject 69's data at index 1 draws anew
    for cap in ("1", "32", "33"):                                                          # 70 chunks of one; 32, 32, 6; 33, 33, 4: a tile tail inside every chunk
        monkeypatch.setenv("ERM_PV_CHUNK", cap)
        assert _bytes(call(slice(None))) == _bytes(whole), cap
    monkeypatch.delenv("ERM_PV_CHUNK")
    other = call(slice(None), seed=pvu.CASE_SEED + 1)
    assert not np.array_equal(other["theta"], whole["theta"]) and not np.array_equal(other["node"], whole["node"])
    assert np.array_equal(other["coarse"], whole["coarse"])                                # the flags belong to the rows, not to the draws
    wide = call(slice(None), seed=pvu.CASE_SEED + (1 << 32))                               # the high word of the seed is part of the key
    assert not np.array_equal(wide["theta"], whole["theta"])


# ------------------------------------------------------------------------------------------------------------ the engine entry
def _assert_result_equals_standalone(got, model, data, rows, K, seed, Q=61, what=""):
    """The dict of an engine or farm entry against erm_plausible_values on the same data and rows; decidable by the twin's gaps on those inputs."""
    pkg = _pkg()
    Y, logT, X = data
    host, gap = pkg.plausibleValuesHost(mu.CODE[model], Y, logT, pvu.kernel_x(model, X), rows, K, seed, Q, with_gap=True)
    assert gap.min() >= pvu.GAP_MIN, f"{what}: a draw of this chain is undecidable (gap {gap.min():.3g}); take another seed for the draws"
    ref = pkg._lib.plausible_values(mu.CODE[model], Y, logT, X, rows, K=K, seed=seed, nodes=Q)
    _assert_equal_draws(got, ref, model != "mlirt", f"{what} against erm_plausible_values")
    _assert_equal_draws(got, host, model != "mlirt", f"{what} against the twin")
    for k in COUNTS:
        assert got[k] == ref[k], k


@pytest.mark.parametrize("full", [True, False], ids=["full", "summary"])
@pytest.mark.parametrize("precision", ["f64", "f32"])
def test_engine_entry_equals_standalone_on_its_own_data_and_rows(precision, full, monkeypatch):
    """300 x 9, 40 sweeps as two interleaved chains of 20 with 10 burn-in iterations: the rows are rows >= 20 of the item trace."""
    Y, logT, X, init, tp = pu.make_problem("rtirt", 300, 9, 3, seed=41)
    eng = _engine("rtirt", Y, logT, X, init, n_iter=20, n_chain=2, n_burnin=10, precision=precision, full=full)
    eng.run(40)
    got = eng.plausible_values(5, 77)
    assert got["nRows"] == eng.post_count == 20 and got["nSubj"] == 300 and got["theta"].shape == (300, 5)
    _assert_result_equals_standalone(got, "rtirt", eng.get_data(), eng.item_trace()[20:], 5, 77, what=f"rtirt {precision} {'full' if full else 'summary'}")
    assert _bytes(eng.plausible_values(5, 77)) == _bytes(got)                              # twice
    monkeypatch.setenv("ERM_PV_CHUNK", "47")
    assert _bytes(eng.plausible_values(5, 77)) == _bytes(got)                              # 47 x 6 and a tail of 18
    monkeypatch.delenv("ERM_PV_CHUNK")
    split = _engine("rtirt", Y, logT, X, init, n_iter=20, n_chain=2, n_burnin=10, precision=precision, full=full)
    split.run(17)
    split.run(23)
    assert _bytes(split.plausible_values(5, 77)) == _bytes(got)
    eng.close()
    split.close()


def test_engine_entry_only_reads_the_engine():
    L = _pkg()._lib
    Y, logT, X, init, tp = pu.make_problem("cross", 300, 9, 3, seed=43)
    eng = _engine("cross", Y, logT, X, init, n_iter=12, n_burnin=5, unit="subject")
    eng.run(12)

    def everything():
        parts = [eng.item_trace(), eng.trace(L.TRACE_LOGLIKE), eng.trace(L.TRACE_RA), eng.trace(L.TRACE_RT), eng.trace(L.TRACE_QR), *eng.pointwise()]
        for d in (eng.get_mean(), eng.get_state()):
            parts += [v for _, v in sorted(d.items()) if v is not None]
        sc = eng.scores()
        return [np.ascontiguousarray(v).tobytes() for v in parts + [sc[c] for c in L.SCORE_COLUMNS]], eng.waic(), eng.post_count, eng.rows_done

    before = everything()
    a = eng.plausible_values()
    eng.plausible_values(21, 5, nodes=127)
    assert everything() == before
    assert a["theta"].shape == (300, 5) and a["nRows"] == eng.post_count == 7 and a["seed"] == L.PV_SEED
    eng.close()


# ------------------------------------------------------------------------------------------------------------ the farm
def test_farm_of_one_chain_equals_its_engine_and_two_chains_the_chain_major_table():
    Y, logT, X, init, tp = pu.make_problem("latent", 300, 9, 3, seed=49)
    one = _farm("latent", [0], Y, logT, X, init, n_iter=14, n_burnin=6)
    one.run(14)
    assert _bytes(one.plausible_values(5, 9)) == _bytes(one.engine(0).plausible_values(5, 9))
    one.close()
    two = _farm("latent", [0, 0], Y, logT, X, init, n_iter=14, n_burnin=6)
    two.run(14)
    rows = np.concatenate([two.engine(l).item_trace()[6:] for l in range(2)], axis=0)
    got = two.plausible_values(5, 9)
    assert got["nRows"] == two.post_count == 16
    _assert_result_equals_standalone(got, "latent", two.engine(0).get_data(), rows, 5, 9, what="farm of 2")
    assert _bytes(two.plausible_values(5, 9)) == _bytes(got)
    two.close()


def test_get_plausible_values_on_samplers():
    """Through the public interface: a devices= sampler (the farm's entry) and a single-engine sampler (the engine's), each against the numpy twin on its own rows."""
    pkg = _pkg()
    Y, logT, X, init, tp = pu.make_problem("rtirt", 200, 9, 3, seed=51)
    Cond = pkg.setCond(nSubj=200, nItem=9, nFeat=3, nIter=16, nChain=2, qRt=0.85)
    for devices, nodes in (([0, 0], 61), (None, 41)):
        M = pkg.GibbsRtIrt(Cond, Data=pkg.InputData(Y=Y, T=np.exp(logT), X=X), trace="summary")
        pkg.sample_b(M, devices=devices)
        pv = pkg.getPlausibleValues(M, K=5, seed=3, nodes=nodes)
        host, gap = pkg.plausibleValuesHost(M._model, M.Data.Y, M.Data.logT, np.asarray(M.Data.X, dtype=np.float64), pkg.gibbs.marginalRows(M), 5, 3, nodes, with_gap=True)
        assert gap.min() >= pvu.GAP_MIN
        _assert_equal_draws(pv, host, True, f"getPlausibleValues devices={devices}")
        assert (pv.nRows, pv.nNodes, pv.nCoarse, pv.seed) == (16, nodes, host.nCoarse, 3) and pv.theta.shape == pv.zeta.shape == pv.node.shape == (200, 5)
        sc = pkg.getScores(M, nodes=nodes)                                                 # five draws against the score: every subject within 6 sd, and not all alike
        assert np.all(np.abs(pv.theta - sc.theta[:, None]) <= 6.0 * sc.thetaSd[:, None]) and np.all(pv.theta.std(axis=1) > 0.0)
        M.close()


# ------------------------------------------------------------------------------------------------------------ refusals
def test_every_refusal_returns_its_code_and_leaves_the_engine_usable():
    L = _pkg()._lib
    lib = L.load()
    err = lambda: lib.erm_last_error().decode()
    N, K = 200, 5
    out, pv, node, coarse = np.zeros(4), np.zeros((2, K, N)), np.zeros((K, N), dtype=np.int32), np.zeros(N, dtype=np.int32)
    Y, logT, X, init, tp = pu.make_problem("rtirt", N, 9, 3, seed=31)
    eng = _engine("rtirt", Y, logT, X, init, n_iter=6, n_burnin=2)
    call = lambda e, n=0, k=K: lib.erm_get_plausible_values(e._h, n, k, 11, pv.ctypes.data, node.ctypes.data, coarse.ctypes.data, out.ctypes.data)
    assert call(eng) == -3 and "one post-burn-in row" in err()                           # ERM_ERR_STATE: nothing recorded
    eng.run(2)                                                                           # rows 0, 1: burn-in
    assert call(eng) == -3 and "one post-burn-in row" in err()
    eng.run(1)                                                                           # one post-burn-in row is enough
    assert call(eng) == 0 and list(out) == [N, 1, 61, out[3]] and np.all(np.isfinite(pv))
    eng.run(3)
    for bad in (60, 1, 1027, -3):
        assert call(eng, bad) == -1 and "odd" in err()                                   # ERM_ERR_ARG
    for bad in (0, -1, 4097):
        assert call(eng, 0, bad) == -1 and "n_draws" in err()
    assert lib.erm_get_plausible_values(eng._h, 0, K, 11, None, node.ctypes.data, coarse.ctypes.data, out.ctypes.data) == -1
    assert lib.erm_get_plausible_values(eng._h, 0, K, 11, pv.ctypes.data, None, None, None) == 0      # node, coarse and out4 may be NULL
    assert call(eng) == 0 and list(out[:3]) == [N, 4, 61]
    assert call(eng, 3) == 0 and out[2] == 3 and out[3] == N and np.all(coarse == 1)     # three nodes: every subject is coarse
    big = np.zeros((2, 4096, N))
    assert lib.erm_get_plausible_values(eng._h, 0, 4096, 11, big.ctypes.data, None, None, out.ctypes.data) == 0 and np.all(np.isfinite(big))      # the largest K
    eng.close()
    # the quantile models
    for model in ("crossqr", "latentqr"):
        Yq, lq, Xq, iq, _ = pu.make_problem(model, N, 7, 3, seed=33)
        q = _engine(model, Yq, lq, Xq, iq, n_iter=6, n_burnin=2)
        q.run(4)
        assert call(q) == -1 and "quantile" in err()
        q.run(2)
        q.close()
    # a subject-sharded engine
    sh = L.Engine(model=L.MODEL_RTIRT, n_item=9, n_subj=N, n_feat=3, n_iter=6, n_chain=1, n_burnin=2, cov2one=1, q_rt=0.5, seed=1, precision=L.PREC_F64, trace_mode=0)
    sh.set_shard(0, 1, N, 0, lambda s, r, n: lib.erm_copy(r, s, n))
    sh.set_data(Y, logT, X)
    sh.set_state(**init)
    sh.run(4)
    assert call(sh) == -3 and "shard" in err()
    sh.run(2)
    sh.close()
    # the farm: no post-burn-in row, a bad node count, a bad K -- and it runs on
    farm = _farm("rtirt", [0, 0], Y, logT, X, init, n_iter=6, n_burnin=2)
    fcall = lambda n=0, k=K: lib.erm_farm_get_plausible_values(farm._h, n, k, 11, pv.ctypes.data, node.ctypes.data, coarse.ctypes.data, out.ctypes.data)
    farm.run(2)
    assert fcall() == -3 and "chain 0" in err() and "one post-burn-in row" in err()
    assert fcall(8) == -1 and fcall(0, 0) == -1
    farm.run(4)
    assert fcall() == 0 and out[1] == 8
    farm.close()
    # erm_plausible_values
    rows = mu.make_rows("rtirt", 9, 3, 3, seed=1)
    Ys, ls, Xs = mu.make_data("rtirt", 5, 9, 3, seed=1)
    code = lambda f: int(str(f.value).split()[2].rstrip(":"))
    with pytest.raises(L.ErmError, match="NaN in row 1") as e:
        bad = rows.copy(); bad[1, 4] = np.nan
        L.plausible_values(1, Ys, ls, Xs, bad)
    assert code(e) == -4                                                                 # ERM_ERR_NONFINITE
    with pytest.raises(L.ErmError, match="NaN in logT") as e:
        lb = ls.copy(); lb[2, 3] = np.nan
        L.plausible_values(1, Ys, lb, Xs, rows)
    assert code(e) == -4
    with pytest.raises(L.ErmError, match="NaN in X") as e:
        xb = Xs.copy(); xb[4, 0] = np.nan
        L.plausible_values(1, Ys, ls, xb, rows)
    assert code(e) == -4
    with pytest.raises(L.ErmError, match="row 2: sig2t") as e:
        bad = rows.copy(); bad[2, 3 * 9 + 1] = 0.0
        L.plausible_values(1, Ys, ls, Xs, bad)
    assert code(e) == -1
    with pytest.raises(L.ErmError, match="row 1: the conditional variance") as e:
        bad = rows.copy(); bad[1, -4:] = [1.0, 2.0, 2.0, 1.0]
        L.plausible_values(1, Ys, ls, Xs, bad)
    assert code(e) == -1
    with pytest.raises(L.ErmError, match="n_rows") as e:
        L.plausible_values(1, Ys, ls, Xs, rows[:0])
    assert code(e) == -1
    with pytest.raises(L.ErmError, match="quantile") as e:
        L.plausible_values(L.MODEL_CROSSQR, Ys, ls, None, np.zeros((2, 5 * 9 + 4)))
    assert code(e) == -1
    p5, n5, c5, o4 = np.zeros((2, K, 5)), np.zeros((K, 5), dtype=np.int32), np.zeros(5, dtype=np.int32), np.zeros(4)
    Yf, lf, Xf = np.asfortranarray(Ys), np.asfortranarray(ls), np.asfortranarray(Xs)
    raw = lambda Q, k: lib.erm_plausible_values(0, 1, 5, 9, 3, Yf.ctypes.data, lf.ctypes.data, Xf.ctypes.data, rows.ctypes.data, 3, Q, k, 11, p5.ctypes.data, n5.ctypes.data,
                                                c5.ctypes.data, o4.ctypes.data)
    for k in (0, 4097, -5):
        assert raw(61, k) == -1 and "n_draws" in err()                                   # K out of range
    for Q in (60, 1, 1027):
        assert raw(Q, K) == -1 and "odd" in err()                                        # an even Q, Q out of range
    assert raw(0, K) == 0 and list(o4[:3]) == [5, 3, 61] and np.all(np.isfinite(p5))      # and the device runs on

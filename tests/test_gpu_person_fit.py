"""Person fit on the device (erm_get_person_fit / erm_farm_get_person_fit / erm_person_fit / erm_person_fit_masked).
  1. fit_kernel against personFitHost, the numpy twin (itself pinned to scipy's quad in tests/test_fit_host.py), under both weightings, on every case of
     fit_util.CASES: five models over N in {1, 33}, J in {1, 9, 65}, rows in {1, 3}, Q in {3, 61, 127}; a_j = 8 with all-correct and all-wrong respondents, logT 22
     off, v = 0; the masked wave with n_i = 0, 1, J - 8, about J / 2 and J side by side.  The four statistics and row_ess within fit_util.KERNEL_TOL =
     max(1e-10, 10 x the twin's own conditioning against numpy.longdouble, 1.5e-13) relative to max(|ref|, 1); COARSE, row_ess under equal weights, out4, n_obs
     and the NaN pattern exactly (tests/test_fit_host.py keeps every twin S at least 0.1 from 2).
  2. bit for bit: obs = NULL against all ones; a pattern subject against its reduced data set; poisoned unobserved cells; a subject alone, at another position,
     among other subjects and under another subject's mask; two calls; COARSE equal to erm_score's.
  3. the engine entry against erm_person_fit on its own data and rows: fp64 and fp32 engines, both trace modes, two interleaved chains; twice; split runs; the
     engine, its scores and its marginal WAIC unchanged by the call.  The farm entry against erm_person_fit on the farm's table.  Every refusal with its code and words.
  4. end to end: GibbsRtIrt fitted on the device to fit_util.aberrant_problem -- the respondent with reversed responses has the smallest pResp, the one with
     shifted times the smallest pTime, neither is flagged on the other component (seed and margins: tests/test_fit_host.py).
  5. GibbsMlIrt: the rank correlation of pResp with getPpc's subject ppp_mid of the same run is above the floor measured on the CPU at five other seeds."""
import numpy as np
import pytest

import fit_util as fu
import marginal_util as mu
import obs_util as ou
import parity_util as pu
import waic_util as wu
from item_pass_util import _bytes, _engine, _farm, _kernel_x, _pkg

pytestmark = pytest.mark.gpu

TOL = fu.KERNEL_TOL
COLUMNS = fu.COLS + ("coarse",)


def _fit(model, Y, logT, X, rows, Q=61, weighting="equal", obs=None):
    return _pkg()._lib.person_fit(mu.CODE[model], Y, logT, X, rows, nodes=Q, weighting=weighting, obs=obs)


def _same_bits(a, b, i=slice(None), j=slice(None)):
    return all(np.array_equal(np.asarray(a[c])[i], np.asarray(b[c])[j], equal_nan=True) for c in COLUMNS)


# ------------------------------------------------------------------------------------------------------------ the kernel against the twin
@pytest.mark.parametrize("model", mu.MODELS)
def test_kernel_equals_twin(model):
    worst = {}
    cases = [c for c in fu.CASES if c[1] == model]
    for case in cases:
        _, Y, logT, X, rows, Q, obs = fu.problem(case)
        for w in fu.WEIGHTINGS:
            dev = _fit(model, Y, logT, X, rows, Q, w, obs)
            host, S = fu.twin(case, w)
            err = fu.errors(dev, host, fu.COLS)                 # (asserts that NaN stands against NaN: MlIrt's two columns, the subjects with n_i = 0)
            for c, e in err.items():
                worst[c] = max(worst.get(c, 0.0), e)
            assert all(e <= TOL for e in err.values()), (case, w, err)
            assert np.array_equal(dev["coarse"], host.coarse) and dev["nCoarse"] == host.nCoarse == int(np.sum(dev["coarse"])), (case, w)
            assert (dev["nSubj"], dev["nRows"], dev["nNodes"]) == (Y.shape[0], rows.shape[0], Q)
            if w == "equal":
                assert np.all(dev["rowEss"] == rows.shape[0])
            if obs is not None:
                assert np.array_equal(dev["nObs"], obs.sum(axis=1)) and np.array_equal(np.isnan(dev["lz"]), obs.sum(axis=1) == 0)
            if model == "mlirt":
                assert np.all(np.isnan(dev["ltz"])) and np.all(np.isnan(dev["pTime"]))
    print(f"{model}: {len(cases)} cases x 2 weightings, worst " + ", ".join(f"{c} {e:.3g}" for c, e in worst.items()) + f" (tolerance {TOL:.3g})")


# ------------------------------------------------------------------------------------------------------------ bit for bit
@pytest.mark.parametrize("model", ["rtirt", "cross", "mlirt"])
def test_masks_bit_for_bit(model):
    Y, logT, X, rows, obs = ou.problem(model, 33, 9, 3, seed=29)
    for w in fu.WEIGHTINGS:
        plain = _fit(model, Y, logT, X, rows, weighting=w)
        ones = _fit(model, Y, logT, X, rows, weighting=w, obs=np.ones_like(obs))
        assert _same_bits(plain, ones) and np.all(ones["nObs"] == 9) and "nObs" not in plain                       # obs = NULL against all ones
        got = _fit(model, Y, logT, X, rows, weighting=w, obs=obs)
        assert _bytes(_fit(model, Y, logT, X, rows, weighting=w, obs=obs)) == _bytes(got)                           # two calls
        Yp, lp = ou.poison(Y, logT, obs)
        assert _bytes(_fit(model, Yp, lp, X, rows, weighting=w, obs=obs)) == _bytes(got)                            # poisoned unobserved cells
        for i in range(12):                                                                                            # a pattern subject against its reduced data set
            red = ou.reduced_subject(model, Y, logT, X, rows, obs, i)
            if red is not None:
                assert _same_bits(got, _fit(model, *red, weighting=w), slice(i, i + 1)), (i, w)
        sc = _pkg()._lib.score(mu.CODE[model], Y, logT, X, rows, weighting=w, obs=obs)
        assert np.array_equal(sc["coarse"], got["coarse"]) and sc["nCoarse"] == got["nCoarse"]                     # COARSE is erm_score's
    # independence: alone, at another position, among other subjects, under another subject's mask
    got = _fit(model, Y, logT, X, rows, obs=obs)
    sub = lambda a, k: None if a is None else np.ascontiguousarray(a[k])
    for i in (0, 4, 5, 32):
        alone = _fit(model, sub(Y, [i]), sub(logT, [i]), sub(X, [i]), rows, obs=sub(obs, [i]))
        assert _same_bits(got, alone, slice(i, i + 1)), i
    perm = np.arange(33)[::-1].copy()
    moved = _fit(model, sub(Y, perm), sub(logT, perm), sub(X, perm), rows, obs=sub(obs, perm))
    assert _same_bits(got, moved, perm)
    other = obs.copy()
    other[1:] = np.roll(obs[1:], 1, axis=0)                         # everybody but subject 0 gets another subject's mask
    assert _same_bits(got, _fit(model, Y, logT, X, rows, obs=other), slice(0, 1), slice(0, 1))


def test_obs_null_is_the_unmasked_entry_bit_for_bit():
    """erm_person_fit_masked given obs = NULL through ctypes: erm_person_fit's outputs, every bit, and n_obs = n_item.  One full tile of 32 and one subject."""
    lib = _pkg()._lib.load()
    N, J, F, R, Q = 33, 5, 3, 2, 3
    Y, logT, X, rows, _ = ou.problem("rtirt", N, J, R, seed=301)
    Yf, lf, Xf = np.asfortranarray(Y), np.asfortranarray(logT), np.asfortranarray(X)
    data = (0, 1, N, J, F, Yf.ctypes.data, lf.ctypes.data, Xf.ctypes.data)
    for w in (0, 1):
        ref, ref4, got, got4 = np.empty((6, N)), np.empty(4), np.empty((6, N)), np.empty(4)
        n_obs = np.zeros(N, dtype=np.int32)
        assert lib.erm_person_fit(*data, rows.ctypes.data, R, Q, w, ref.ctypes.data, ref4.ctypes.data) == 0
        assert lib.erm_person_fit_masked(*data, None, rows.ctypes.data, R, Q, w, got.ctypes.data, got4.ctypes.data, n_obs.ctypes.data) == 0
        assert got.tobytes() == ref.tobytes() and got4.tobytes() == ref4.tobytes() and list(ref4[:3]) == [N, R, Q] and np.all(n_obs == J)
        assert lib.erm_person_fit_masked(*data, None, rows.ctypes.data, R, Q, w, got.ctypes.data, got4.ctypes.data, None) == 0      # n_obs may be NULL
        assert got.tobytes() == ref.tobytes()


@pytest.mark.parametrize("model", ["rtirt", "latent"])
def test_a_subjects_fit_depends_on_its_own_data_only(model):
    rows = mu.make_rows(model, 9, 3, 4, seed=31)
    Y, logT, X = mu.make_data(model, 600, 9, 3, seed=31)
    for w in fu.WEIGHTINGS:
        whole = _fit(model, Y, logT, X, rows, weighting=w)
        sc = _pkg()._lib.score(mu.CODE[model], Y, logT, X, rows, weighting=w)
        assert np.array_equal(sc["coarse"], whole["coarse"]) and np.array_equal(sc["rowEss"], whole["rowEss"])
        for lo, hi in ((0, 256), (256, 600), (599, 600)):
            part = _fit(model, Y[lo:hi], logT[lo:hi], X[lo:hi], rows, weighting=w)
            assert all(np.all(np.isfinite(part[c])) for c in COLUMNS) and _same_bits(whole, part, slice(lo, hi)), (lo, hi, w)


# ------------------------------------------------------------------------------------------------------------ the engine entry
def _assert_result_equals_person_fit(got, model, data, rows, Q=61, what=""):
    """The dict of an engine or farm entry against erm_person_fit on the same data and rows, equal weights."""
    ref = _fit(model, *data, rows, Q)
    err = fu.errors(got, ref, fu.COLS)
    print(f"{what}: rows {got['nRows']}, " + ", ".join(f"{c} {e:.3g}" for c, e in err.items()) + f"; coarse {got['nCoarse']}")
    assert all(e <= TOL for e in err.values()), err
    assert np.array_equal(got["coarse"], ref["coarse"])
    for k in ("nSubj", "nRows", "nNodes", "nCoarse"):
        assert got[k] == ref[k], k


@pytest.mark.parametrize("full", [True, False], ids=["full", "summary"])
@pytest.mark.parametrize("precision", ["f64", "f32"])
@pytest.mark.parametrize("model", ["rtirt", "cross"])
def test_engine_entry_equals_person_fit_on_its_own_data_and_rows(model, precision, full):
    """600 x 9, 40 sweeps as two interleaved chains of 20 with 10 burn-in iterations: the rows are rows >= 20 of the item trace."""
    Y, logT, X, init, tp = pu.make_problem(model, 600, 9, 3, seed=41)
    eng = _engine(model, Y, logT, X, init, n_iter=20, n_chain=2, n_burnin=10, precision=precision, full=full)
    eng.run(40)
    got = eng.person_fit()
    assert got["nRows"] == eng.post_count == 20 and got["nSubj"] == 600 and np.all(got["rowEss"] == 20.0)
    _assert_result_equals_person_fit(got, model, eng.get_data(), eng.item_trace()[20:], what=f"{model} {precision} {'full' if full else 'summary'}")
    assert _bytes(eng.person_fit()) == _bytes(got)                                        # twice
    split = _engine(model, Y, logT, X, init, n_iter=20, n_chain=2, n_burnin=10, precision=precision, full=full)
    split.run(17)
    split.run(23)
    assert _bytes(split.person_fit()) == _bytes(got)
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
        return [np.ascontiguousarray(v).tobytes() for v in parts + [lppd_i, p_i]], w, _bytes(eng.scores()), eng.waic(), eng.post_count, eng.rows_done

    before = everything()
    eng.person_fit()
    eng.person_fit(nodes=127)
    assert everything() == before
    eng.close()


# ------------------------------------------------------------------------------------------------------------ the farm
def test_farm_equals_person_fit_on_the_chain_major_rows():
    Y, logT, X, init, tp = pu.make_problem("rtirt", 600, 9, 3, seed=47)
    farm = _farm("rtirt", [0, 0], Y, logT, X, init, n_iter=14, n_burnin=6)
    farm.run(14)
    rows = np.concatenate([farm.engine(l).item_trace()[6:] for l in range(2)], axis=0)
    got = farm.person_fit()
    assert got["nRows"] == farm.post_count == 16
    _assert_result_equals_person_fit(got, "rtirt", farm.engine(0).get_data(), rows, what="farm of 2")
    assert _bytes(farm.person_fit()) == _bytes(got)
    farm.close()
    one = _farm("latent", [0], *pu.make_problem("latent", 600, 9, 3, seed=49)[:4], n_iter=14, n_burnin=6)
    one.run(14)
    assert _bytes(one.person_fit()) == _bytes(one.engine(0).person_fit())            # a farm of one chain is its engine
    one.close()


def test_get_person_fit_on_samplers():
    """Through the public interface: a devices= sampler (the farm's entry) and a single-engine sampler (the engine's), each against the numpy twin on its own rows."""
    pkg = _pkg()
    Y, logT, X, init, tp = pu.make_problem("rtirt", 300, 9, 3, seed=51)
    Cond = pkg.setCond(nSubj=300, nItem=9, nFeat=3, nIter=16, nChain=2, qRt=0.85)
    for devices, nodes in (([0, 0], 61), (None, 41)):
        M = pkg.GibbsRtIrt(Cond, Data=pkg.InputData(Y=Y, T=np.exp(logT), X=X), trace="summary")
        pkg.sample_b(M, devices=devices)
        pf = pkg.getPersonFit(M, nodes=nodes)
        host = pkg.personFitHost(M._model, M.Data.Y, M.Data.logT, np.asarray(M.Data.X, dtype=np.float64), pkg.gibbs.marginalRows(M), nodes)
        err = fu.errors(pf, host, fu.COLS)
        print(f"getPersonFit devices={devices}: " + ", ".join(f"{c} {e:.3g}" for c, e in err.items()) + f"; {pf}")
        assert all(e <= TOL for e in err.values()), err
        assert pf.nRows == 16 and pf.nNodes == nodes and pf.nCoarse == host.nCoarse and pf.lz.shape == (300,) and np.all(pf.rowEss == 16.0) and pf.nObs is None
        M.close()
    rows = mu.make_rows("rtirt", 9, 3, 3, seed=1)
    obs = ou.masks(5, 9, 3)
    pm = pkg.personFit(1, Y[:5], logT[:5], X[:5], rows, weighting="likelihood", obs=obs)
    assert pm.weighting == "likelihood" and pm.lz.shape == (5,) and np.array_equal(pm.nObs, obs.sum(axis=1)) and np.isnan(pm.pResp[1]) and np.isfinite(pm.pTime[0])
    assert np.all((pm.rowEss >= 1.0) & (pm.rowEss <= 3.0))


# ------------------------------------------------------------------------------------------------------------ refusals
def test_every_refusal_returns_its_code_and_words():
    L = _pkg()._lib
    lib = L.load()
    err = lambda: lib.erm_last_error().decode()
    out, ft = np.zeros(4), np.zeros((6, 500))
    Y, logT, X, init, tp = pu.make_problem("rtirt", 500, 9, 3, seed=31)
    eng = _engine("rtirt", Y, logT, X, init, n_iter=6, n_burnin=2)
    call = lambda e, n=0: lib.erm_get_person_fit(e._h, n, ft.ctypes.data, out.ctypes.data)
    assert call(eng) == -3 and err() == "the person fit needs at least one post-burn-in row"      # ERM_ERR_STATE: nothing recorded
    eng.run(2)                                                                           # rows 0, 1: burn-in
    assert call(eng) == -3 and err() == "the person fit needs at least one post-burn-in row"
    eng.run(1)                                                                           # one post-burn-in row is enough
    assert call(eng) == 0 and list(out) == [500, 1, 61, out[3]] and np.all(ft[4] == 1.0)
    eng.run(3)
    for bad in (60, 1, 1027, -3):
        assert call(eng, bad) == -1 and "odd" in err()                                   # ERM_ERR_ARG
    assert lib.erm_get_person_fit(eng._h, 0, None, out.ctypes.data) == -1 and "NULL" in err()
    assert lib.erm_get_person_fit(None, 0, ft.ctypes.data, out.ctypes.data) == -1 and "handle" in err()
    assert lib.erm_get_person_fit(eng._h, 0, ft.ctypes.data, None) == 0                  # out4 may be NULL
    assert call(eng) == 0 and list(out[:3]) == [500, 4, 61]
    assert call(eng, 3) == 0 and out[2] == 3 and out[3] == 500 and np.all(ft[5] == 1.0)  # three nodes: every unit is coarse
    eng.close()
    for model in ("crossqr", "latentqr"):                                                # the quantile models, with the marginal WAIC's reason
        Yq, lq, Xq, iq, _ = pu.make_problem(model, 200, 7, 3, seed=33)
        q = _engine(model, Yq, lq, Xq, iq, n_iter=6, n_burnin=2)
        q.run(4)
        assert call(q) == -1 and "quantile weights" in err() and "no longer Gaussian in zeta" in err()
        q.close()
    sh = L.Engine(model=L.MODEL_RTIRT, n_item=9, n_subj=500, n_feat=3, n_iter=6, n_chain=1, n_burnin=2, cov2one=1, q_rt=0.5, seed=1, precision=L.PREC_F64, trace_mode=0)
    sh.set_shard(0, 1, 500, 0, lambda s, r, n: lib.erm_copy(r, s, n))
    sh.set_data(Y, logT, X)
    sh.set_state(**init)
    sh.run(4)
    assert call(sh) == -3 and err() == "the person fit is not available on a shard (every subject's data must be resident on one device)"
    sh.run(2)
    sh.close()
    nodata = L.Engine(model=L.MODEL_RTIRT, n_item=9, n_subj=500, n_feat=3, n_iter=6, n_chain=1, n_burnin=2, cov2one=1, q_rt=0.5, seed=1, precision=L.PREC_F64, trace_mode=0)
    assert call(nodata) == -3 and "no data set" in err()
    nodata.close()
    farm = _farm("rtirt", [0, 0], Y, logT, X, init, n_iter=6, n_burnin=2)
    fcall = lambda n=0: lib.erm_farm_get_person_fit(farm._h, n, ft.ctypes.data, out.ctypes.data)
    farm.run(2)
    assert fcall() == -3 and err() == "chain 0: the person fit needs at least one post-burn-in row"
    assert fcall(8) == -1
    farm.run(4)
    assert fcall() == 0 and out[1] == 8
    farm.close()
    # erm_person_fit and erm_person_fit_masked
    rows = mu.make_rows("rtirt", 9, 3, 3, seed=1)
    Ys, ls, Xs = mu.make_data("rtirt", 5, 9, 3, seed=1)
    obs = ou.masks(5, 9, 3)
    code = lambda f: int(str(f.value).split()[2].rstrip(":"))
    for kw in ({}, {"obs": obs}):
        with pytest.raises(L.ErmError, match="NaN in row 1") as e:
            bad = rows.copy(); bad[1, 4] = np.nan
            L.person_fit(1, Ys, ls, Xs, bad, **kw)
        assert code(e) == -4                                                             # ERM_ERR_NONFINITE
        with pytest.raises(L.ErmError, match="NaN in logT") as e:
            lb = ls.copy(); lb[0, 3] = np.nan                                            # (subject 0 sees every item)
            L.person_fit(1, Ys, lb, Xs, rows, **kw)
        assert code(e) == -4
        with pytest.raises(L.ErmError, match="NaN in X") as e:
            xb = Xs.copy(); xb[4, 0] = np.nan
            L.person_fit(1, Ys, ls, xb, rows, **kw)
        assert code(e) == -4
        with pytest.raises(L.ErmError, match="row 2: sig2t") as e:
            bad = rows.copy(); bad[2, 3 * 9 + 1] = 0.0
            L.person_fit(1, Ys, ls, Xs, bad, **kw)
        assert code(e) == -1
        with pytest.raises(L.ErmError, match="row 1: the conditional variance") as e:
            bad = rows.copy(); bad[1, -4:] = [1.0, 2.0, 2.0, 1.0]
            L.person_fit(1, Ys, ls, Xs, bad, **kw)
        assert code(e) == -1
        with pytest.raises(L.ErmError, match="n_rows") as e:
            L.person_fit(1, Ys, ls, Xs, rows[:0], **kw)
        assert code(e) == -1
        with pytest.raises(L.ErmError, match="quantile") as e:
            L.person_fit(L.MODEL_CROSSQR, Ys, ls, None, np.zeros((2, 5 * 9 + 4)), **kw)
        assert code(e) == -1
    with pytest.raises(L.ErmError, match="obs must be 0/1") as e:
        bad = obs.copy(); bad[2, 2] = 2
        L.person_fit(1, Ys, ls, Xs, rows, obs=bad)
    assert code(e) == -1
    lb = ls.copy(); lb[1, 3] = np.nan                                                    # subject 1 sees nothing: its NaN is never read
    assert np.isnan(L.person_fit(1, Ys, lb, Xs, rows, obs=obs)["lz"][1])
    f5, o4 = np.zeros((6, 5)), np.zeros(4)
    Yf, lf, Xf = np.asfortranarray(Ys), np.asfortranarray(ls), np.asfortranarray(Xs)
    raw = lambda Q, w, f=f5: lib.erm_person_fit(0, 1, 5, 9, 3, Yf.ctypes.data, lf.ctypes.data, Xf.ctypes.data, rows.ctypes.data, 3, Q, w, None if f is None else f.ctypes.data, o4.ctypes.data)
    for w in (2, -1, 7):
        assert raw(61, w) == -1 and "weighting" in err()                                 # an unknown weighting
    for Q in (60, 1, 1027):
        assert raw(Q, 0) == -1 and "odd" in err()                                        # an even Q, Q out of range
    assert raw(61, 0, None) == -1 and "NULL" in err()
    assert raw(0, 1) == 0 and list(o4[:3]) == [5, 3, 61] and np.all(np.isfinite(f5))      # and the device runs on


# ------------------------------------------------------------------------------------------------------------ it discriminates
def test_planted_respondents_have_the_smallest_p_values():
    """fit_util.aberrant_problem through the engine from make_problem's initial state, the chain the oracle ran on the CPU (tests/test_fit_host.py: pResp 3.2e-4
    against 0.095 for the next respondent, pTime 8.5e-59 against 0.114; pTime 0.61 and pResp 0.81 on the component that was not touched)."""
    Y, logT, X, who_r, who_t = fu.aberrant_problem()
    init = pu.make_problem("rtirt", fu.E2E_N, fu.E2E_J, 3, seed=fu.E2E_SEED)[3]
    eng = _engine("rtirt", Y, logT, X, init, n_iter=fu.E2E_SWEEPS, n_burnin=fu.E2E_BURNIN, full=False)
    eng.run(fu.E2E_SWEEPS)
    got = eng.person_fit()
    host = _pkg().personFitHost(mu.CODE["rtirt"], *eng.get_data(), eng.item_trace()[fu.E2E_BURNIN:], 61)
    eng.close()
    pr, pt = got["pResp"], got["pTime"]
    print(f"pResp[{who_r}] {pr[who_r]:.3g} (next {np.delete(pr, who_r).min():.3g}), pTime[{who_t}] {pt[who_t]:.3g} (next {np.delete(pt, who_t).min():.3g}); "
          f"pTime[{who_r}] {pt[who_r]:.3f}, pResp[{who_t}] {pr[who_t]:.3f}; lz {got['lz'][who_r]:.2f}, ltz {got['ltz'][who_t]:.2f}")
    assert got["nRows"] == fu.E2E_SWEEPS - fu.E2E_BURNIN and got["nCoarse"] == 0
    assert int(np.argmin(pr)) == who_r and int(np.argmin(pt)) == who_t
    assert pt[who_r] >= 0.05 and pr[who_t] >= 0.05
    assert got["lz"][who_r] < -2.0 and got["ltz"][who_t] > 5.0
    assert all(e <= TOL for e in fu.errors(got, host, fu.COLS).values())


def test_p_resp_tracks_the_predictive_check_for_mlirt():
    """GibbsMlIrt on waic_util.spread_problem (600 x 12, 200 sweeps) through the public interface with the posterior predictive check switched on: the rank
    correlation of pResp with the subject ppp_mid of the response deviance, against fit_util.PPC_FLOOR (measured on the CPU at five other seeds; 0.976 at this one)."""
    from scipy.stats import spearmanr
    pkg = _pkg()
    Y, X, init = wu.spread_problem()
    Cond = pkg.setCond(nSubj=wu.SPREAD_N, nItem=wu.SPREAD_J, nFeat=1, nIter=wu.SPREAD_ITER, nChain=1)
    M = pkg.GibbsMlIrt(Cond, Data=pkg.InputData(Y=Y, X=X), trace="summary")
    pkg.sample_b(M, ppc=True, fill=False)
    mid = pkg.getPpc(M).ppp_mid("subject", "ra")
    pf = pkg.getPersonFit(M)
    r = float(spearmanr(mid, pf.pResp).correlation)
    print(f"rank correlation of pResp with the subject ppp_mid: {r:.4f} (floor {fu.PPC_FLOOR:.4f}); {pf}")
    assert pf.nCoarse == 0 and np.all(np.isnan(pf.ltz)) and np.all(np.isnan(pf.pTime)) and pf.nRows == wu.SPREAD_ITER - Cond.nBurnin
    assert r >= fu.PPC_FLOOR
    M.close()

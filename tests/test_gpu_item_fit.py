"""Item fit on the device (erm_get_item_fit / erm_farm_get_item_fit / erm_item_fit).
  1. item_fit_kernel and its reduction against itemFitHost, the numpy twin (itself pinned to scipy's quadrature in tests/test_ifit_host.py), on every case of
     ifit_util.CASES: five models over N in {1, 33, 257}, J in {1, 9, 65}, rows in {1, 3}, Q in {3, 61, 127}; a_j = 8 with all-correct and all-wrong respondents,
     logT 22 off, v = 0; the masked wave with n_i = 0, 1, J - 8, about J / 2 and J side by side; a column nobody observed; 896 items x 33 subjects x 1 row.  The
     five statistics within ifit_util.KERNEL_TOL = max(1e-10, 10 x the twin's own conditioning against numpy.longdouble) relative to max(|ref|, 1); N_OBS, out4,
     the NaN pattern and COARSE (against erm_score's) exactly (tests/test_ifit_host.py keeps every twin S at least 0.1 from 2).
  2. bit for bit: obs = NULL against all ones; poisoned unobserved cells; two calls; ERM_IFIT_CHUNK = 256 against unset at N = 600 (the library reads it at every
     call); a permutation of the items permuting the result's rows.  The last holds bit for bit where the sums over the items keep their value under the
     permutation: the two items of J = 2 exchanged (every sum over the items is then a + b against b + a).  At J = 9 the item sums of a subject are added in
     another order, (M, S) move in their last bits, and the permuted result stands within the tolerance of section 1.
  3. additivity: removing one subject changes the items' sums by that subject's twin cells.
  4. the engine entry against erm_item_fit on its own data and rows: fp64 and fp32 engines, both trace modes; twice; split runs 17 + 23; the engine, its scores
     and its person fit unchanged by the call.  The farm entry against erm_item_fit on the farm's table.  Every refusal with its code and words.
  5. end to end: GibbsRtIrt calibrated on a clean sample; a second sample with one item's b + 1 and another's lambda + sigma / 2 carries the largest |RESP_Z| and
     |RT_Z| on exactly those items (seed and factors: tests/test_ifit_host.py)."""
import numpy as np
import pytest

import ifit_util as iu
import marginal_util as mu
import obs_util as ou
import parity_util as pu
from item_pass_util import _bytes, _engine, _farm, _pkg

pytestmark = pytest.mark.gpu

TOL = iu.KERNEL_TOL
KEYS = iu.COLS + ("nObs",)


def _fit(model, Y, logT, X, rows, Q=61, obs=None):
    return _pkg()._lib.item_fit(mu.CODE[model], Y, logT, X, rows, nodes=Q, obs=obs)


def _same_bits(a, b, perm=slice(None)):
    return all(np.array_equal(np.asarray(a[c]), np.asarray(b[c])[perm], equal_nan=True) for c in KEYS)


# ------------------------------------------------------------------------------------------------------------ the kernels against the twin
@pytest.mark.parametrize("model", mu.MODELS)
def test_kernel_equals_twin(model):
    worst = {}
    cases = [c for c in iu.CASES if c[1] == model]
    for case in cases:
        _, Y, logT, X, rows, Q, obs = iu.problem(case)
        dev = _fit(model, Y, logT, X, rows, Q, obs)
        host, _, S = iu.twin(case)
        err = iu.errors(dev, host)                              # (asserts that NaN stands against NaN: MlIrt's two columns, the items with n_j = 0)
        for c, e in err.items():
            worst[c] = max(worst.get(c, 0.0), e)
        assert all(e <= TOL for e in err.values()), (case, err)
        n_j = np.full(Y.shape[1], Y.shape[0]) if obs is None else obs.sum(axis=0)
        assert np.array_equal(dev["nObs"], n_j) and np.array_equal(dev["nObs"], host.nObs), case
        assert np.array_equal(np.isnan(dev["infit"]), n_j == 0) and np.array_equal(np.isnan(dev["respZ"]), n_j == 0) and np.array_equal(np.isnan(dev["outfit"]), n_j == 0)
        assert np.array_equal(np.isnan(dev["rtZ"]), (n_j == 0) | (model == "mlirt")) and np.array_equal(np.isnan(dev["rtMsq"]), (n_j == 0) | (model == "mlirt"))
        sc = _pkg()._lib.score(mu.CODE[model], Y, logT, X, rows, nodes=Q, obs=obs)
        assert (dev["nSubj"], dev["nRows"], dev["nNodes"], dev["nCoarse"]) == (Y.shape[0], rows.shape[0], Q, sc["nCoarse"]), case
        assert dev["nCoarse"] == host.nCoarse == int(np.sum(np.any(S < 2.0, axis=0))), case
    print(f"{model}: {len(cases)} cases, worst " + ", ".join(f"{c} {e:.3g}" for c, e in worst.items()) + f" (tolerance {TOL:.3g})")


# ------------------------------------------------------------------------------------------------------------ bit for bit
@pytest.mark.parametrize("model", ["rtirt", "cross", "mlirt"])
def test_masks_and_calls_bit_for_bit(model):
    Y, logT, X, rows, obs = ou.problem(model, 33, 9, 3, seed=29)
    plain = _fit(model, Y, logT, X, rows)
    assert _bytes(_fit(model, Y, logT, X, rows, obs=np.ones_like(obs))) == _bytes(plain)                   # obs = NULL against all ones
    got = _fit(model, Y, logT, X, rows, obs=obs)
    assert _bytes(_fit(model, Y, logT, X, rows, obs=obs)) == _bytes(got) and _bytes(_fit(model, Y, logT, X, rows)) == _bytes(plain)      # two calls
    Yp, lp = ou.poison(Y, logT, obs)
    assert _bytes(_fit(model, Yp, lp, X, rows, obs=obs)) == _bytes(got)                                    # poisoned unobserved cells
    assert np.array_equal(got["nObs"], obs.sum(axis=0)) and not _same_bits(got, plain)


@pytest.mark.parametrize("model", ["rtirt", "latent"])
def test_result_does_not_depend_on_the_chunk(model, monkeypatch):
    """600 subjects: one chunk of three blocks (256 + 256 + 88) against three chunks of one block; and a cap of 1, which is rounded up to one block."""
    rows = mu.make_rows(model, 9, 3, 4, seed=31)
    Y, logT, X = mu.make_data(model, 600, 9, 3, seed=31)
    obs = ou.masks(600, 9, 5)
    monkeypatch.delenv("ERM_IFIT_CHUNK", raising=False)
    whole, wm = _fit(model, Y, logT, X, rows), _fit(model, Y, logT, X, rows, obs=obs)
    for cap in ("256", "1", "300"):
        monkeypatch.setenv("ERM_IFIT_CHUNK", cap)
        assert _bytes(_fit(model, Y, logT, X, rows)) == _bytes(whole) and _bytes(_fit(model, Y, logT, X, rows, obs=obs)) == _bytes(wm), cap
    monkeypatch.delenv("ERM_IFIT_CHUNK")
    assert all(np.all(np.isfinite(whole[c])) for c in iu.COLS) and np.all(whole["nObs"] == 600)


def _permute_items(model, Y, logT, rows, perm):
    J = Y.shape[1]
    r = rows.copy()
    for k in range(5 if model == "cross" else 4):
        r[:, k * J:(k + 1) * J] = rows[:, k * J:(k + 1) * J][:, perm]
    return np.ascontiguousarray(Y[:, perm]), None if logT is None else np.ascontiguousarray(logT[:, perm]), r


@pytest.mark.parametrize("model", ["rtirt", "cross", "mlirt"])
def test_a_permutation_of_the_items_permutes_the_rows(model):
    rows = mu.make_rows(model, 2, 3, 3, seed=37)
    Y, logT, X = mu.make_data(model, 300, 2, 3, seed=37)
    Xk = ou.kernel_x(model, X)
    perm = np.array([1, 0])
    assert _same_bits(_fit(model, *_permute_items(model, Y, logT, rows, perm)[:2], Xk, _permute_items(model, Y, logT, rows, perm)[2]), _fit(model, Y, logT, Xk, rows), perm)
    rows = mu.make_rows(model, 9, 3, 3, seed=37)                       # nine items: the item sums change their order, the result stands within the tolerance
    Y, logT, X = mu.make_data(model, 300, 9, 3, seed=37)
    Xk = ou.kernel_x(model, X)
    perm = np.random.default_rng(1).permutation(9)
    Yp, lp, rp = _permute_items(model, Y, logT, rows, perm)
    a, b = _fit(model, Yp, lp, Xk, rp), _fit(model, Y, logT, Xk, rows)
    err = {c: ou.rel(a[c], b[c][perm]) for c in iu.COLS}
    print(f"{model}: nine items permuted, " + ", ".join(f"{c} {e:.3g}" for c, e in err.items()))
    assert all(e <= TOL for e in err.values()) and np.array_equal(a["nObs"], b["nObs"][perm])


# ------------------------------------------------------------------------------------------------------------ additivity
@pytest.mark.parametrize("model", ["rtirt", "cross"])
def test_removing_a_subject_removes_its_cells(model):
    """The sums behind three columns can be read off the result: sum E[z^2] = OUTFIT n_j, sum E[d^2] = RT_MSQ n_j, sum E[d] = RT_Z sqrt(n_j).  With subject 100 of
    300 removed they fall by that subject's twin cells, within the tolerance relative to the sums."""
    rows = mu.make_rows(model, 9, 3, 3, seed=39)
    Y, logT, X = mu.make_data(model, 300, 9, 3, seed=39)
    Xk = ou.kernel_x(model, X)
    keep = np.arange(300) != 100
    sub = lambda a: None if a is None else np.ascontiguousarray(a[keep])
    full, less = _fit(model, Y, logT, Xk, rows), _fit(model, sub(Y), sub(logT), sub(Xk), rows)
    _, cells = _pkg().itemFitHost(mu.CODE[model], Y[100:101], logT[100:101], None if Xk is None else Xk[100:101], rows, 61, with_cells=True)
    sums = lambda r: (r["outfit"] * r["nObs"], r["rtMsq"] * r["nObs"], r["rtZ"] * np.sqrt(r["nObs"]))
    for (a, b), col in zip(zip(sums(full), sums(less)), (3, 5, 4)):
        scale = np.maximum(np.abs(a), 1.0)
        assert np.all(np.abs((a - b) - cells[0, :, col]) <= 4 * TOL * scale), (col, a - b, cells[0, :, col])
    assert np.all(full["nObs"] == 300) and np.all(less["nObs"] == 299)


# ------------------------------------------------------------------------------------------------------------ the engine entry
def _assert_result_equals_item_fit(got, model, data, rows, Q=61, what=""):
    ref = _fit(model, *data, rows, Q)
    err = iu.errors(got, ref)
    print(f"{what}: rows {got['nRows']}, " + ", ".join(f"{c} {e:.3g}" for c, e in err.items()) + f"; coarse {got['nCoarse']}")
    assert _same_bits(got, ref), err                                                       # identical
    for k in ("nSubj", "nRows", "nNodes", "nCoarse"):
        assert got[k] == ref[k], k


@pytest.mark.parametrize("full", [True, False], ids=["full", "summary"])
@pytest.mark.parametrize("precision", ["f64", "f32"])
@pytest.mark.parametrize("model", ["rtirt", "cross"])
def test_engine_entry_equals_item_fit_on_its_own_data_and_rows(model, precision, full):
    """600 x 9, 40 sweeps as two interleaved chains of 20 with 10 burn-in iterations: the rows are rows >= 20 of the item trace.  The engine holds logT centred by
    its column means and adds them back in the kernel, erm_get_data adds them back on the host, by the same addition: the entry is erm_item_fit on its own data
    and rows by the bit, and so are two calls and split runs."""
    Y, logT, X, init, tp = pu.make_problem(model, 600, 9, 3, seed=41)
    eng = _engine(model, Y, logT, X, init, n_iter=20, n_chain=2, n_burnin=10, precision=precision, full=full)
    eng.run(40)
    got = eng.item_fit()
    assert got["nRows"] == eng.post_count == 20 and got["nSubj"] == 600 and np.all(got["nObs"] == 600)
    _assert_result_equals_item_fit(got, model, eng.get_data(), eng.item_trace()[20:], what=f"{model} {precision} {'full' if full else 'summary'}")
    assert _bytes(eng.item_fit()) == _bytes(got)                                          # twice
    split = _engine(model, Y, logT, X, init, n_iter=20, n_chain=2, n_burnin=10, precision=precision, full=full)
    split.run(17)
    split.run(23)
    assert _bytes(split.item_fit()) == _bytes(got)
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
        return [np.ascontiguousarray(v).tobytes() for v in parts], _bytes(eng.scores()), _bytes(eng.person_fit()), eng.waic(), eng.post_count, eng.rows_done

    before = everything()
    eng.item_fit()
    eng.item_fit(nodes=127)
    assert everything() == before
    eng.close()


def test_farm_equals_item_fit_on_the_chain_major_rows():
    Y, logT, X, init, tp = pu.make_problem("rtirt", 600, 9, 3, seed=47)
    farm = _farm("rtirt", [0, 0], Y, logT, X, init, n_iter=14, n_burnin=6)
    farm.run(14)
    rows = np.concatenate([farm.engine(l).item_trace()[6:] for l in range(2)], axis=0)
    got = farm.item_fit()
    assert got["nRows"] == farm.post_count == 16
    _assert_result_equals_item_fit(got, "rtirt", farm.engine(0).get_data(), rows, what="farm of 2")
    assert _bytes(farm.item_fit()) == _bytes(got)
    farm.close()


def test_get_item_fit_on_samplers():
    """Through the public interface: a devices= sampler (the farm's entry) and a single-engine sampler (the engine's), each against the numpy twin on its own rows."""
    pkg = _pkg()
    Y, logT, X, init, tp = pu.make_problem("rtirt", 300, 9, 3, seed=51)
    Cond = pkg.setCond(nSubj=300, nItem=9, nFeat=3, nIter=16, nChain=2, qRt=0.85)
    for devices, nodes in (([0, 0], 61), (None, 41)):
        M = pkg.GibbsRtIrt(Cond, Data=pkg.InputData(Y=Y, T=np.exp(logT), X=X), trace="summary")
        pkg.sample_b(M, devices=devices)
        f = pkg.getItemFit(M, nodes=nodes)
        host = pkg.itemFitHost(M._model, M.Data.Y, M.Data.logT, np.asarray(M.Data.X, dtype=np.float64), pkg.gibbs.marginalRows(M), nodes)
        err = iu.errors(f, host)
        print(f"getItemFit devices={devices}: " + ", ".join(f"{c} {e:.3g}" for c, e in err.items()) + f"; {f}")
        assert all(e <= TOL for e in err.values()), err
        assert f.nRows == 16 and f.nNodes == nodes and f.nCoarse == host.nCoarse and f.infit.shape == (9,) and np.all(f.nObs == 300) and f.nSubj == 300
        M.close()
    rows = mu.make_rows("rtirt", 9, 3, 3, seed=1)
    obs = ou.masks(5, 9, 3)
    fm = pkg.itemFit(1, Y[:5], logT[:5], X[:5], rows, obs=obs)
    assert fm.infit.shape == (9,) and np.array_equal(fm.nObs, obs.sum(axis=0)) and fm.nSubj == 5 and fm.nRows == 3


# ------------------------------------------------------------------------------------------------------------ refusals
def test_every_refusal_returns_its_code_and_words():
    L = _pkg()._lib
    lib = L.load()
    err = lambda: lib.erm_last_error().decode()
    out, ft = np.zeros(4), np.zeros((6, 9))
    Y, logT, X, init, tp = pu.make_problem("rtirt", 500, 9, 3, seed=31)
    eng = _engine("rtirt", Y, logT, X, init, n_iter=6, n_burnin=2)
    call = lambda e, n=0: lib.erm_get_item_fit(e._h, n, ft.ctypes.data, out.ctypes.data)
    assert call(eng) == -3 and err() == "the item fit needs at least one post-burn-in row"        # ERM_ERR_STATE: nothing recorded
    eng.run(2)                                                                           # rows 0, 1: burn-in
    assert call(eng) == -3 and err() == "the item fit needs at least one post-burn-in row"
    eng.run(1)                                                                           # one post-burn-in row is enough
    assert call(eng) == 0 and list(out) == [500, 1, 61, out[3]] and np.all(ft[5] == 500.0)
    eng.run(3)
    for bad in (60, 1, 1027, -3):
        assert call(eng, bad) == -1 and "odd" in err()                                   # ERM_ERR_ARG
    assert lib.erm_get_item_fit(eng._h, 0, None, out.ctypes.data) == -1 and "NULL" in err()
    assert lib.erm_get_item_fit(None, 0, ft.ctypes.data, out.ctypes.data) == -1 and "handle" in err()
    assert lib.erm_get_item_fit(eng._h, 0, ft.ctypes.data, None) == 0                    # out4 may be NULL
    assert call(eng) == 0 and list(out[:3]) == [500, 4, 61]
    assert call(eng, 3) == 0 and out[2] == 3 and out[3] == 500                           # three nodes: every unit is coarse
    eng.close()
    for model in ("crossqr", "latentqr"):                                                # the quantile models, with the marginal WAIC's reason
        Yq, lq, Xq, iq, _ = pu.make_problem(model, 200, 9, 3, seed=33)
        q = _engine(model, Yq, lq, Xq, iq, n_iter=6, n_burnin=2)
        q.run(4)
        assert call(q) == -1 and "quantile weights" in err() and "no longer Gaussian in zeta" in err()
        q.close()
    sh = L.Engine(model=L.MODEL_RTIRT, n_item=9, n_subj=500, n_feat=3, n_iter=6, n_chain=1, n_burnin=2, cov2one=1, q_rt=0.5, seed=1, precision=L.PREC_F64, trace_mode=0)
    sh.set_shard(0, 1, 500, 0, lambda s, r, n: lib.erm_copy(r, s, n))
    sh.set_data(Y, logT, X)
    sh.set_state(**init)
    sh.run(4)
    assert call(sh) == -3 and err() == "the item fit is not available on a shard (every subject's data must be resident on one device)"
    sh.run(2)
    sh.close()
    nodata = L.Engine(model=L.MODEL_RTIRT, n_item=9, n_subj=500, n_feat=3, n_iter=6, n_chain=1, n_burnin=2, cov2one=1, q_rt=0.5, seed=1, precision=L.PREC_F64, trace_mode=0)
    assert call(nodata) == -3 and "no data set" in err()
    nodata.close()
    farm = _farm("rtirt", [0, 0], Y, logT, X, init, n_iter=6, n_burnin=2)
    fcall = lambda n=0: lib.erm_farm_get_item_fit(farm._h, n, ft.ctypes.data, out.ctypes.data)
    farm.run(2)
    assert fcall() == -3 and err() == "chain 0: the item fit needs at least one post-burn-in row"
    assert fcall(8) == -1
    farm.run(4)
    assert fcall() == 0 and out[1] == 8
    farm.close()
    # erm_item_fit, complete and masked
    rows = mu.make_rows("rtirt", 9, 3, 3, seed=1)
    Ys, ls, Xs = mu.make_data("rtirt", 5, 9, 3, seed=1)
    obs = ou.masks(5, 9, 3)
    code = lambda f: int(str(f.value).split()[2].rstrip(":"))
    for kw in ({}, {"obs": obs}):
        with pytest.raises(L.ErmError, match="NaN in row 1") as e:
            bad = rows.copy(); bad[1, 4] = np.nan
            L.item_fit(1, Ys, ls, Xs, bad, **kw)
        assert code(e) == -4                                                             # ERM_ERR_NONFINITE
        with pytest.raises(L.ErmError, match="NaN in logT") as e:
            lb = ls.copy(); lb[0, 3] = np.nan                                            # (subject 0 sees every item)
            L.item_fit(1, Ys, lb, Xs, rows, **kw)
        assert code(e) == -4
        with pytest.raises(L.ErmError, match="NaN in X") as e:
            xb = Xs.copy(); xb[4, 0] = np.nan
            L.item_fit(1, Ys, ls, xb, rows, **kw)
        assert code(e) == -4
        with pytest.raises(L.ErmError, match="row 2: sig2t") as e:
            bad = rows.copy(); bad[2, 3 * 9 + 1] = 0.0
            L.item_fit(1, Ys, ls, Xs, bad, **kw)
        assert code(e) == -1
        with pytest.raises(L.ErmError, match="row 1: the conditional variance") as e:
            bad = rows.copy(); bad[1, -4:] = [1.0, 2.0, 2.0, 1.0]
            L.item_fit(1, Ys, ls, Xs, bad, **kw)
        assert code(e) == -1
        with pytest.raises(L.ErmError, match="n_rows") as e:
            L.item_fit(1, Ys, ls, Xs, rows[:0], **kw)
        assert code(e) == -1
        with pytest.raises(L.ErmError, match="quantile") as e:
            L.item_fit(L.MODEL_CROSSQR, Ys, ls, None, np.zeros((2, 5 * 9 + 4)), **kw)
        assert code(e) == -1
    with pytest.raises(L.ErmError, match="obs must be 0/1") as e:
        bad = obs.copy(); bad[2, 2] = 2
        L.item_fit(1, Ys, ls, Xs, rows, obs=bad)
    assert code(e) == -1
    lb = ls.copy(); lb[1, 3] = np.nan                                                    # subject 1 sees nothing: its NaN is never read
    assert np.all(np.isfinite(L.item_fit(1, Ys, lb, Xs, rows, obs=obs)["nObs"]))
    f9, o4 = np.zeros((6, 9)), np.zeros(4)
    Yf, lf, Xf = np.asfortranarray(Ys), np.asfortranarray(ls), np.asfortranarray(Xs)
    raw = lambda Q, f=f9: lib.erm_item_fit(0, 1, 5, 9, 3, Yf.ctypes.data, lf.ctypes.data, Xf.ctypes.data, None, rows.ctypes.data, 3, Q, None if f is None else f.ctypes.data, o4.ctypes.data)
    for Q in (60, 1, 1027):
        assert raw(Q) == -1 and "odd" in err()                                           # an even Q, Q out of range
    assert raw(61, None) == -1 and "NULL" in err()
    assert raw(0) == 0 and list(o4[:3]) == [5, 3, 61] and np.all(np.isfinite(f9)) and np.all(f9[5] == 5.0)      # and the device runs on


# ------------------------------------------------------------------------------------------------------------ it finds drift
def test_planted_items_carry_the_largest_signed_residuals():
    """ifit_util.e2e_problem: the calibration through the engine from make_problem's initial state (the chain the oracle ran on the CPU), the second sample through
    erm_item_fit against the engine's post-burn-in rows.  tests/test_ifit_host.py measured on the oracle's chain the planted items' |z| against the largest other
    (ifit_util.E2E_RESP_FACTOR, E2E_RT_FACTOR); here they must hold less the stated margin, and the device's columns must match the twin's on the oracle's rows."""
    (Y, logT, X, init), (Y2, logT2, X2) = iu.e2e_problem()
    eng = _engine("rtirt", Y, logT, X, init, n_iter=iu.E2E_SWEEPS, n_burnin=iu.E2E_BURNIN, full=False)
    eng.run(iu.E2E_SWEEPS)
    rows = eng.item_trace()[iu.E2E_BURNIN:]
    eng.close()
    got = _fit("rtirt", Y2, logT2, X2, rows)
    cpu = _pkg().itemFitHost(mu.CODE["rtirt"], Y2, logT2, X2, iu.e2e_oracle_rows(), 61)
    rz, tz = np.abs(got["respZ"]), np.abs(got["rtZ"])
    fr, ft = rz[iu.E2E_ITEM_B] / np.delete(rz, iu.E2E_ITEM_B).max(), tz[iu.E2E_ITEM_LAM] / np.delete(tz, iu.E2E_ITEM_LAM).max()
    gap = iu.errors(got, cpu)
    print(f"RESP_Z[{iu.E2E_ITEM_B}] {got['respZ'][iu.E2E_ITEM_B]:.2f} (factor {fr:.2f}), RT_Z[{iu.E2E_ITEM_LAM}] {got['rtZ'][iu.E2E_ITEM_LAM]:.2f} (factor {ft:.2f}); "
          "device against the CPU: " + ", ".join(f"{c} {e:.3g}" for c, e in gap.items()))
    assert got["nRows"] == iu.E2E_SWEEPS - iu.E2E_BURNIN and got["nCoarse"] == 0
    assert int(np.argmax(rz)) == iu.E2E_ITEM_B and int(np.argmax(tz)) == iu.E2E_ITEM_LAM
    assert got["respZ"][iu.E2E_ITEM_B] < 0.0 and got["rtZ"][iu.E2E_ITEM_LAM] > 0.0
    assert fr >= iu.E2E_RESP_FACTOR - iu.E2E_MARGIN and ft >= iu.E2E_RT_FACTOR - iu.E2E_MARGIN
    assert all(e <= iu.E2E_GAP_BOUND for e in gap.values()), gap

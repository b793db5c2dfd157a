"""Marginal PSIS-LOO on the device (erm_get_marginal_loo / erm_farm_get_marginal_loo / erm_psis_loo).
  1. erm_psis_loo against psisLooHost, the numpy twin written from the papers (tests/test_psis_host.py pins it): pw, lw and out12 for N = 67 units and
     S in {25, 26, 127, 225, 1000, 4097, 8192} -- Gaussian columns, one row 700 below the rest, ties across the cutoff, a constant column, a heavy tail with
     k^ > 0.7, a constant tail, exceedances over 300 orders of magnitude (psis_util).  Integers and the Inf pattern exactly; the rest within PSIS_BOUND.
  2. packing: a unit's pw and lw rows are bit-identical alone, first, in the middle and last of 67 and in batches of one; twice in a row.
  3. the engine entry equals erm_psis_loo on erm_marginal_loglik's l for the engine's data and rows bit for bit, and the twin within PSIS_BOUND + the marginal
     kernel's 1e-10 (tests/test_gpu_marginal_waic.py); fp32 engine included.
  4. chunks: 13 chunks of 23 subjects and a tail of one equal the one-chunk result bit for bit.
  5. the farm: one chain equals its engine bit for bit; two chains equal erm_psis_loo on the chain-major table.
  6. the call only reads the engine.
  7. every refusal returns its code and a word of its own.
  8. an aberrant respondent has the largest k^, and no untouched respondent is flagged."""
import functools

import numpy as np
import pytest

import marginal_util as mu
import parity_util as pu
import psis_util as ps
import item_pass_util as ipu
from item_pass_util import _bytes, _farm, _kernel_x, _pkg

pytestmark = pytest.mark.gpu

# The floating tolerance between the kernel and the twin: 64 x the largest difference between psisLooHost in fp64 and the same code in np.longdouble over the
# tables of test 1 (rel(): |a - b| / max(|b|, 1)), floor 1e-13.  MEASURED: 2.31e-12 (S = 8192, the column with one row 700 below the rest: its other ratios are
# about 1e-304 and k^ about 4.7; S = 25 .. 226: 0.4 .. 1.1e-13; S = 1000: 5.6e-13; S = 4097: 1.7e-12), so the bound is 1.48e-10.  Computed again at run time from
# the same tables (ps.bound), so the constant documents and the assertion uses the measurement of the machine the test runs on.
PSIS_BOUND_MEASURED = 64 * 2.31e-12
MARGINAL_TOL = 1e-10                          # tests/test_gpu_marginal_waic.py: marginal_kernel against its twin
TOTALS = ("elpd", "pLoo", "LOOIC", "se", "lppd")
COUNTS = ("nUnits", "nRows", "nBadK", "nHighK", "tailLen", "nNodes", "nCoarse")
COLS = (("elpd_u", "elpd_u"), ("p_u", "p_u"), ("khat", "khat"), ("nEff", "nEff"))
_engine = functools.partial(ipu._engine, full=False)          # these tests run in summary mode


def _bound():
    b = ps.bound(ps.S_GPU)
    assert ps.FLOOR <= b <= 4.0 * PSIS_BOUND_MEASURED, b          # the documented measurement still describes the tables
    return b


def _assert_equals_host(dev, host, tol, what, lw=None, lw_host=None):
    errs = {d: ps.rel(dev[d], getattr(host, h)) for d, h in COLS}
    if lw is not None:
        errs["lw"] = ps.rel(lw, lw_host)
    for k in TOTALS:
        errs[k] = ps.rel([dev[k]], [getattr(host, k)])
    print(f"{what}: " + ", ".join(f"{k} {v:.3g}" for k, v in errs.items()) + f"; bound {tol:.3g}; nBadK {dev['nBadK']}, nHighK {dev['nHighK']}, M {dev['tailLen']}")
    assert np.array_equal(np.isposinf(dev["khat"]), np.isposinf(host.khat)) and not np.any(np.isnan(dev["khat"]))
    for k in ("nUnits", "nRows", "nBadK", "nHighK", "tailLen"):
        assert dev[k] == getattr(host, k), k
    for k, v in errs.items():
        assert v <= tol, (k, v, tol)


# ------------------------------------------------------------------------------------------------------------ the kernel against the twin
@pytest.mark.parametrize("S", ps.S_GPU)
def test_kernel_equals_twin(S):
    pkg = _pkg()
    L = ps.table(S)
    dev = pkg._lib.psis_loo(L.T, want_lw=True)
    host, lw_host = pkg.psisLooHost(L, with_lw=True)
    _assert_equals_host(dev, host, _bound(), f"S={S}", dev["lw"].T, lw_host)
    assert dev["nNodes"] == 0 and dev["nCoarse"] == 0 and dev["tailLen"] == ps.tail_len(S)
    by_kind = {ps.kind_of(u): dev["khat"][u] for u in range(7)}
    assert np.isposinf(by_kind["constant"]) and np.isposinf(by_kind["consttail"]) and np.isfinite(by_kind["gauss"])
    if S >= 1000:
        assert by_kind["heavy"] > 0.7
    assert np.all(np.abs(np.log(np.sum(np.exp(dev["lw"]), axis=1))) <= 1e-12)                 # normalised: LSE = 0


# ------------------------------------------------------------------------------------------------------------ packing
@pytest.mark.parametrize("S", [127, 1000, 4097, 8192])
def test_packing_does_not_change_a_bit(S, monkeypatch):
    """One wave per unit (S = 127, 1000), two (4097), the whole workgroup (8192)."""
    L = _pkg()._lib
    T = ps.table(S)

    def row(r, u):
        return b"".join(np.ascontiguousarray(r[k][u]).tobytes() for k in ("elpd_u", "p_u", "khat", "nEff", "lw"))

    for u in (0, 4, 6):                                                                      # gauss, heavy, span300
        col = T[:, u]
        alone = L.psis_loo(col[None, :], want_lw=True)
        want = row(alone, 0)
        assert np.isfinite(alone["elpd_u"][0])
        for at in (0, 33, 66):
            tab = np.array(T.T)
            tab[at] = col
            assert row(L.psis_loo(tab, want_lw=True), at) == want, (u, at)
        assert row(L.psis_loo(col[None, :], want_lw=True), 0) == want                        # twice
        tab = np.array(T.T)
        tab[65] = col
        monkeypatch.setenv("ERM_PSIS_CHUNK", "1")                                            # 67 batches of one
        assert row(L.psis_loo(tab, want_lw=True), 65) == want
        monkeypatch.delenv("ERM_PSIS_CHUNK")


# ------------------------------------------------------------------------------------------------------------ the engine entry
def _via_loglik(model, data, rows, Q=61):
    """erm_psis_loo on the l erm_marginal_loglik returns for the data and the rows, with the node count and the coarse count of the marginal kernel's totals."""
    L = _pkg()._lib
    Y, logT, X = data
    m = L.marginal_loglik(mu.CODE[model], Y, logT, X, rows, nodes=Q)
    r = L.psis_loo(m["l"])
    r["nNodes"], r["nCoarse"] = m["totals"]["nNodes"], m["totals"]["nCoarse"]
    return r


@pytest.mark.parametrize("model,precision", [("rtirt", "f64"), ("rtirt", "f32"), ("mlirt", "f64"), ("cross", "f64")])
def test_engine_entry_equals_psis_loo_on_its_own_loglik(model, precision):
    """300 x 9, F = 3, 60 sweeps, 30 post-burn-in rows."""
    pkg = _pkg()
    Y, logT, X, init, tp = pu.make_problem(model, 300, 9, 3, seed=71)
    eng = _engine(model, Y, logT, X, init, n_iter=60, n_burnin=30, precision=precision)
    eng.run(60)
    got = eng.marginal_loo(pointwise=True)
    assert got["nRows"] == eng.post_count == 30 and got["nUnits"] == 300 and got["nNodes"] == 61 and got["tailLen"] == 6
    data, rows = eng.get_data(), eng.item_trace()[30:]
    assert _bytes(got) == _bytes(_via_loglik(model, data, rows))                              # bit for bit
    assert _bytes(eng.marginal_loo(pointwise=True)) == _bytes(got)                            # twice
    tot = eng.marginal_loo()
    assert all(tot[k] == got[k] for k in TOTALS + COUNTS) and "khat" not in tot
    Lh, Sh = pkg.marginalLogLikHost(mu.CODE[model], data[0], data[1], _kernel_x(model, data[2]), rows, 61, with_S=True)
    host = pkg.psisLooHost(Lh)
    _assert_equals_host(got, host, _bound() + MARGINAL_TOL, f"{model} {precision}")
    assert got["nCoarse"] == int(np.sum(np.any(Sh < 2.0, axis=0)))
    assert abs(got["lppd"] - eng.marginal_waic()["lppd"]) <= 1e-12 * abs(got["lppd"])       # lppd_i is the marginal WAIC's
    eng.close()


def test_chunks_equal_one_chunk_bit_for_bit(monkeypatch):
    Y, logT, X, init, tp = pu.make_problem("rtirt", 300, 9, 3, seed=73)
    eng = _engine("rtirt", Y, logT, X, init, n_iter=60, n_burnin=30)
    eng.run(60)
    whole = eng.marginal_loo(pointwise=True)
    monkeypatch.setenv("ERM_PSIS_CHUNK", "23")                                               # 13 chunks of 23 and a tail of one subject
    assert _bytes(eng.marginal_loo(pointwise=True)) == _bytes(whole)
    monkeypatch.setenv("ERM_PSIS_CHUNK", "128")                                              # 128, 128, 44: tile tails inside the chunks
    assert _bytes(eng.marginal_loo(pointwise=True)) == _bytes(whole)
    monkeypatch.delenv("ERM_PSIS_CHUNK")
    eng.close()


# ------------------------------------------------------------------------------------------------------------ the farm
def test_farm_of_one_chain_equals_its_engine_and_two_chains_the_chain_major_table():
    Y, logT, X, init, tp = pu.make_problem("rtirt", 300, 9, 3, seed=75)
    one = _farm("rtirt", [0], Y, logT, X, init, n_iter=60, n_burnin=30)
    one.run(60)
    assert _bytes(one.marginal_loo(pointwise=True)) == _bytes(one.engine(0).marginal_loo(pointwise=True))
    one.close()
    two = _farm("rtirt", [0, 0], Y, logT, X, init, n_iter=60, n_burnin=30)
    two.run(60)
    rows = np.concatenate([two.engine(l).item_trace()[30:] for l in range(2)], axis=0)
    got = two.marginal_loo(pointwise=True)
    assert got["nRows"] == two.post_count == 60 and got["tailLen"] == 12
    assert _bytes(got) == _bytes(_via_loglik("rtirt", two.engine(0).get_data(), rows))
    two.close()


# ------------------------------------------------------------------------------------------------------------ read-only
def test_the_call_only_reads_the_engine():
    L = _pkg()._lib
    Y, logT, X, init, tp = pu.make_problem("rtirt", 300, 9, 3, seed=77)
    eng = _engine("rtirt", Y, logT, X, init, n_iter=60, n_burnin=30, full=True)
    eng.run(60)

    def everything():
        parts = [eng.item_trace(), eng.trace(L.TRACE_LOGLIKE), eng.trace(L.TRACE_RA), eng.trace(L.TRACE_RT), eng.trace(L.TRACE_QR)]
        for d in (eng.get_mean(), eng.get_state()):
            parts += [v for _, v in sorted(d.items()) if v is not None]
        return [np.ascontiguousarray(p).tobytes() for p in parts], _mw(eng.marginal_waic(pointwise=True)), eng.post_count, eng.rows_done

    def _mw(r):
        return repr(sorted(r[0].items())).encode() + r[1].tobytes() + r[2].tobytes()

    before = everything()
    eng.marginal_loo(pointwise=True)
    eng.marginal_loo(nodes=127)
    assert everything() == before
    eng.close()


# ------------------------------------------------------------------------------------------------------------ refusals
def test_every_refusal_returns_its_code_and_a_word_of_its_own():
    L = _pkg()._lib
    lib = L.load()
    err = lambda: lib.erm_last_error().decode()
    out = np.zeros(12)
    Y, logT, X, init, tp = pu.make_problem("rtirt", 100, 9, 3, seed=31)
    eng = _engine("rtirt", Y, logT, X, init, n_iter=60, n_burnin=30)
    call = lambda e, n=0: lib.erm_get_marginal_loo(e._h, n, out.ctypes.data, None)
    eng.run(54)                                                                          # 24 post-burn-in rows
    assert call(eng) == -1 and "at least 25" in err()                                    # ERM_ERR_ARG
    eng.run(1)
    for bad in (60, 1, 1027, -3):
        assert call(eng, bad) == -1 and "odd" in err()
    assert lib.erm_get_marginal_loo(eng._h, 0, None, None) == -1 and "NULL" in err()
    assert call(eng) == 0 and out[5] == 100 and out[6] == 25 and out[9] == 5 and out[10] == 61
    eng.close()
    # 8193 rows
    Ys, ls, Xs, inits, _ = pu.make_problem("rtirt", 40, 5, 3, seed=35)
    long = _engine("rtirt", Ys, ls, Xs, inits, n_iter=8193, n_burnin=0)
    long.run(8193)
    assert call(long) == -1 and "at most 8192" in err()
    long.close()
    # the quantile models
    for model in ("crossqr", "latentqr"):
        Yq, lq, Xq, iq, _ = pu.make_problem(model, 100, 7, 3, seed=33)
        q = _engine(model, Yq, lq, Xq, iq, n_iter=60, n_burnin=30)
        q.run(60)
        assert call(q) == -1 and "quantile" in err()
        q.close()
    # a subject-sharded engine
    sh = L.Engine(model=L.MODEL_RTIRT, n_item=9, n_subj=100, n_feat=3, n_iter=60, n_chain=1, n_burnin=30, cov2one=1, q_rt=0.5, seed=1, precision=L.PREC_F64, trace_mode=0)
    sh.set_shard(0, 1, 100, 0, lambda s, r, n: lib.erm_copy(r, s, n))
    sh.set_data(Y, logT, X)
    sh.set_state(**init)
    sh.run(60)
    assert call(sh) == -3 and "shard" in err()                                           # ERM_ERR_STATE
    sh.close()
    # the farm: a chain with no post-burn-in row is named; too few rows over the chains; and it runs on
    farm = _farm("rtirt", [0, 0], Y, logT, X, init, n_iter=60, n_burnin=30)
    fcall = lambda n=0: lib.erm_farm_get_marginal_loo(farm._h, n, out.ctypes.data, None)
    farm.run(30)
    assert fcall() == -3 and "chain 0" in err() and "post-burn-in" in err()
    farm.run(12)
    assert fcall() == -1 and "at least 25" in err()                                      # 2 x 12 rows
    assert fcall(8) == -1 and "odd" in err()
    assert lib.erm_farm_get_marginal_loo(farm._h, 0, None, None) == -1
    farm.run(1)
    assert fcall() == 0 and out[6] == 26
    farm.close()
    # erm_psis_loo
    code = lambda f: int(str(f.value).split()[2].rstrip(":"))
    good = np.array(ps.table(25)[:, :3].T)
    for S, word in ((24, "at least 25"), (8193, "at most 8192")):
        with pytest.raises(L.ErmError, match=word) as e:
            L.psis_loo(np.zeros((2, S)))
        assert code(e) == -1
    with pytest.raises(L.ErmError, match="unit 1, row 7") as e:
        bad = good.copy(); bad[1, 7] = np.nan
        L.psis_loo(bad)
    assert code(e) == -4                                                                 # ERM_ERR_NONFINITE
    assert lib.erm_psis_loo(0, good.ctypes.data, 3, 25, None, None, None) == -1 and "NULL" in err()
    assert L.psis_loo(good)["nRows"] == 25


# ------------------------------------------------------------------------------------------------------------ it discriminates
def aberrant_problem(seed=62, who=17, shift=3.5):
    """make_problem("rtirt", 300, 12) with respondent `who` overwritten: the six hardest items correct and answered 3.5 log-seconds faster than the item's mean
    time, the six easiest wrong and 3.5 slower."""
    Y, logT, X, init, tp = pu.make_problem("rtirt", 300, 12, 3, seed=seed)
    Y, logT = Y.copy(), logT.copy()
    order = np.argsort(np.asarray(tp.b).ravel())
    easy, hard = order[:6], order[6:]
    Y[who, hard], Y[who, easy] = 1, 0
    cm = logT.mean(axis=0)
    logT[who, hard], logT[who, easy] = cm[hard] - shift, cm[easy] + shift
    return Y, logT, X, who


def test_an_aberrant_respondent_has_the_largest_khat():
    """Through the public interface: GibbsRtIrt, 1000 sweeps, 500 post-burn-in rows (M = 68).  On the CPU, with the oracle chain of make_problem's initial state and
    psisLooHost on marginalLogLikHost's table, the twin gave k^ = 2.455 for the respondent and at most 0.387 for the 299 untouched ones (seed 62; seeds 61, 63, 64
    and a shift of 2.5: the respondent 1.27 .. 2.60, the others at most 0.54).  With 100 rows (M = 20) the same data gave untouched respondents up to 0.83: k^ of
    twenty values is too noisy for a flag, hence the chain length.  The device, through sample_b, gave the same: 2.455 against 0.387, elpd_loo - elpd_waic +8.60 for
    the respondent and within [-0.007, +0.002] for the others, n_eff 1.2 of 500 rows."""
    pkg = _pkg()
    Y, logT, X, who = aberrant_problem()
    Cond = pkg.setCond(nSubj=300, nItem=12, nFeat=3, nIter=1000, nChain=1, qRt=0.85)
    M = pkg.GibbsRtIrt(Cond, Data=pkg.InputData(Y=Y, T=np.exp(logT), X=X), trace="summary")
    pkg.sample_b(M)
    loo = pkg.getLooMarginal(M, pointwise=True)
    waic = pkg.getWaicMarginal(M, pointwise=True)
    host = pkg.getLooMarginalHost(M)
    others = np.delete(loo.khat, who)
    d = loo.elpd_u - waic.elpd_u
    print(f"{loo}; khat[{who}] {loo.khat[who]:.3f} (twin {host.khat[who]:.3f}), largest untouched {others.max():.3f}; elpd_loo - elpd_waic: respondent {d[who]:.3f}, "
          f"others in [{np.delete(d, who).min():.3f}, {np.delete(d, who).max():.3f}]; nEff[{who}] {loo.nEff[who]:.1f}")
    assert loo.unit == host.unit == "subject-marginal" and loo.nRows == 500 and loo.tailLen == 68 and loo.nCoarse == host.nCoarse == 0
    assert int(np.argmax(loo.khat)) == who and loo.khat[who] > 0.7
    assert np.all(others < 0.7) and loo.nBadK == 1
    assert ps.rel(loo.khat, host.khat) <= _bound() + MARGINAL_TOL and ps.rel(loo.elpd_u, host.elpd_u) <= _bound() + MARGINAL_TOL
    c = pkg.compareLoo(loo, loo)
    assert c["elpd_diff"] == 0.0 and c["nUnits"] == 300
    M.close()

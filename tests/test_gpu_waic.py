"""WAIC accumulated on the device (erm_set_pointwise / erm_get_waic / erm_get_pointwise): the chain does not move when it is enabled, on any
schedule; per-unit values and totals equal getWaicHost, the numpy twin, evaluated on erm_get_data's data set and the engine's own traces (1e-10 relative, the
bound tests/test_gpu_dic.py uses for device = host: the comparison holds no storage rounding) for every model, both precisions and both units; the bookkeeping
(split runs, summary-trace engines, erm_reset_trace, every refusal); the full size; and the 2pl-against-1pl comparison."""
import numpy as np
import pytest

import parity_util as pu
import waic_util as wu

pytestmark = pytest.mark.gpu

MODELS = ["mlirt", "rtirt", "crossqr", "latentqr", "null", "cross", "latent"]
LPPD_FLOOR = 1e-3
TOTALS = ("elpd", "pWaic", "WAIC", "se", "lppd", "nUnits", "nRows", "nHighVar")


def _engine(model, Y, logT, X, init, *, n_iter, n_chain=1, n_burnin, precision="f64", full=True, unit=None, flags=0, onepl=False, seed=1234):
    L = pu.ge.load_package()._lib
    N, J = Y.shape
    eng = L.Engine(model=pu.MODELS[model], n_item=J, n_subj=N, n_feat=0 if X is None else X.shape[1], n_iter=n_iter, n_chain=n_chain, n_burnin=n_burnin,
                   one_pl=int(onepl), cov2one=int(model not in ("latentqr", "latent")), q_rt=0.85, seed=seed, precision={"f32": 0, "f64": 1}[precision],
                   trace_mode=1 if full else 0, flags=flags)
    eng.set_data(Y, logT, X)
    if unit is not None:
        eng.set_pointwise(unit)
    eng.set_state(**{("lambda_" if k == "lam" else k): v for k, v in init.items()})
    return eng


def _everything(eng, model):
    """What a chain leaves behind, as bytes: item trace, logLike, the subject-level traces, Post.mean, the final state."""
    L = pu.ge.load_package()._lib
    parts = [eng.item_trace(), eng.trace(L.TRACE_LOGLIKE), eng.trace(L.TRACE_RA), eng.trace(L.TRACE_QR)]
    if model != "mlirt":
        parts.append(eng.trace(L.TRACE_RT))
    for d in (eng.get_mean(), eng.get_state()):
        parts += [v for _, v in sorted(d.items()) if v is not None]
    return [np.ascontiguousarray(p).tobytes() for p in parts], eng.post_count


def _twin(eng, model, *, n_iter, n_chain, n_burnin, unit, data=None):
    pkg = pu.ge.load_package()
    L = pkg._lib
    Y, logT, _ = eng.get_data() if data is None else data
    M = wu.as_sampler(model, Y, logT, eng.trace(L.TRACE_RA), None if model == "mlirt" else eng.trace(L.TRACE_RT), eng.trace(L.TRACE_QR), nIter=n_iter, nChain=n_chain,
                      nBurnin=n_burnin)
    return pkg.getWaicHost(M, unit)


def _assert_equals_twin(eng, host, tol=1e-10, what=""):
    w = eng.waic()
    lppd_u, p_u = eng.pointwise()
    assert lppd_u.shape == host.lppd_u.shape
    # lppd_u of a response-time cell is a negative response term plus a normal log-density that may be positive, each O(1): it passes through zero (508 000 cells
    # of the Cross family: a few within 1e-6 of it), where no fp64 evaluation -- the twin's included, which rounds terms of that size to 1e-16 -- has a relative
    # error to speak of.  Below |lppd_u| = LPPD_FLOOR the bound is therefore the absolute 1e-10 * LPPD_FLOOR = 1e-13; p_u, a variance, stays purely relative.
    el, ep = np.max(np.abs(lppd_u - host.lppd_u) / np.maximum(np.abs(host.lppd_u), LPPD_FLOOR)), np.max(np.abs(p_u - host.p_u) / np.abs(host.p_u))
    print(f"{what}: units {w['nUnits']}, rows {w['nRows']}, max rel err lppd_u {el:.3g}, p_u {ep:.3g}; " +
          ", ".join(f"{k} {w[k]!r} / {getattr(host, k)!r}" for k in TOTALS))
    assert el <= tol and ep <= tol
    for k in TOTALS[:5]:
        assert abs(w[k] - getattr(host, k)) <= tol * abs(getattr(host, k)), k
    for k in TOTALS[5:]:
        assert w[k] == getattr(host, k), k


# ------------------------------------------------------------------------------------------------------------ nothing else moves
@pytest.mark.parametrize("precision", ["f64", "f32"])
@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("shape,flags", [((1000, 15), 0), ((20000, 24), 0), ((20000, 24), 1), ((20000, 24), 2)], ids=["persist-size", "graphs", "no-fuse", "no-graph"])
def test_chain_is_bit_identical_with_waic_off_subject_and_cell(model, precision, shape, flags):
    """1 000 x 15 is eligible for the persistent schedule: with WAIC enabled the engine plans per-sweep launches at the same geometry (erm_timing.persistent == 0) and
    the chain equals the persistent chain bit for bit.  20 000 x 24 runs from captured graphs (two calls: block graphs, then the whole-call graph), under
    ERM_FLAG_NO_FUSE as two kernels per sweep and under ERM_FLAG_NO_GRAPH sweep by sweep."""
    N, J = shape
    Y, logT, X, init, tp = pu.make_problem(model, N, J, 3, seed=13)
    got = {}
    for unit in (None, "subject", "cell"):
        eng = _engine(model, Y, logT, X, init, n_iter=12, n_burnin=5, precision=precision, unit=unit, flags=flags)
        tm = eng.timing()
        if unit is not None:
            assert tm["persistent"] == 0
        elif shape == (20000, 24) or model in ("crossqr", "cross"):
            assert tm["persistent"] == 0
        else:
            assert tm["persistent"] == 1
        eng.run(5)
        eng.run(7)
        tm = eng.timing()
        if unit is None and shape == (1000, 15) and model not in ("crossqr", "cross"):
            assert tm["persistent"] == 1 or tm["persist_fallbacks"] > 0
        got[unit] = _everything(eng, model)
        if unit is not None:
            assert eng.pointwise_units == (N if unit == "subject" else N * J) and eng.waic()["nRows"] == 7
        eng.close()
    assert got["subject"] == got[None] and got["cell"] == got[None]


# ------------------------------------------------------------------------------------------------------------ values
@pytest.mark.parametrize("unit", ["subject", "cell"])
@pytest.mark.parametrize("precision", ["f64", "f32"])
@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("shape", [(1001, 17), (4000, 127)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_device_waic_equals_the_host_twin(model, precision, unit, shape):
    """nChain = 3 interleaved pseudo-chains, 6 iterations, burn-in 3: S = the 9 rows m >= 3 of all chains.  The fp32 engine's totals on the log-likelihood scale
    (lppd, elpd, WAIC) are also compared with the twin on the ORIGINAL fp64 data, at the 2e-6 tests/test_gpu_dic.py grants the rounded data set."""
    N, J = shape
    Y, logT, X, init, tp = pu.make_problem(model, N, J, 3, seed=17)
    eng = _engine(model, Y, logT, X, init, n_iter=6, n_chain=3, n_burnin=3, precision=precision, unit=unit)
    eng.run(18)
    assert eng.post_count == 9
    _assert_equals_twin(eng, _twin(eng, model, n_iter=6, n_chain=3, n_burnin=3, unit=unit), what=f"{model} {precision} {unit} {N}x{J}")
    if precision == "f32":
        orig, w = _twin(eng, model, n_iter=6, n_chain=3, n_burnin=3, unit=unit, data=(Y, logT, X)), eng.waic()
        for k in ("lppd", "elpd", "WAIC"):
            print(f"  against the original data: {k} {w[k]!r} / {getattr(orig, k)!r}")
            assert abs(w[k] - getattr(orig, k)) <= 2e-6 * abs(getattr(orig, k)), k
    eng.close()


@pytest.mark.parametrize("unit", ["subject", "cell"])
def test_device_waic_at_896_items(unit):
    Y, logT, X, init, tp = pu.make_problem("rtirt", 300, 896, 3, seed=19)
    eng = _engine("rtirt", Y, logT, X, init, n_iter=6, n_burnin=2, unit=unit)
    eng.run(6)
    _assert_equals_twin(eng, _twin(eng, "rtirt", n_iter=6, n_chain=1, n_burnin=2, unit=unit), what=f"rtirt f64 {unit} 300x896")
    eng.close()


# ------------------------------------------------------------------------------------------------------------ bookkeeping
@pytest.mark.parametrize("model,precision,unit", [("rtirt", "f64", "subject"), ("crossqr", "f64", "cell"), ("latentqr", "f32", "cell"), ("mlirt", "f32", "subject")])
def test_split_runs_and_summary_engines_keep_the_same_accumulators(model, precision, unit):
    """run(3) + run(1) + run(3) leaves bit-identical accumulators to run(7), and a summary-trace engine to a full-trace one."""
    Y, logT, X, init, tp = pu.make_problem(model, 3000, 21, 3, seed=23)
    out = []
    for full, calls in ((True, (7,)), (True, (3, 1, 3)), (False, (7,)), (False, (3, 1, 3))):
        eng = _engine(model, Y, logT, X, init, n_iter=7, n_burnin=2, precision=precision, full=full, unit=unit)
        for n in calls:
            eng.run(n)
        lppd_u, p_u = eng.pointwise()
        out.append((lppd_u.tobytes(), p_u.tobytes(), tuple(sorted(eng.waic().items()))))
        eng.close()
    assert out[1] == out[0] and out[2] == out[0] and out[3] == out[0]


def test_reset_trace_clears_the_accumulators():
    L = pu.ge.load_package()._lib
    Y, logT, X, init, tp = pu.make_problem("rtirt", 800, 11, 3, seed=29)
    eng = _engine("rtirt", Y, logT, X, init, n_iter=6, n_burnin=2, unit="cell")
    eng.run(6)
    first = eng.waic()
    eng.reset_trace()
    with pytest.raises(L.ErmError, match="two post-burn-in rows"):
        eng.waic()
    eng.run(6)                                               # the chain goes on from where it was: other draws, a new S
    again = eng.waic()
    assert again["nRows"] == 4 and again["elpd"] != first["elpd"]
    _assert_equals_twin(eng, _twin(eng, "rtirt", n_iter=6, n_chain=1, n_burnin=2, unit="cell"), what="after erm_reset_trace")
    eng.close()


def test_every_refusal_returns_its_code_and_leaves_the_engine_usable():
    import ctypes as C
    L = pu.ge.load_package()._lib
    lib = L.load()
    Y, logT, X, init, tp = pu.make_problem("rtirt", 500, 9, 3, seed=31)
    eng = _engine("rtirt", Y, logT, X, init, n_iter=6, n_burnin=2)
    out = np.zeros(8)
    err = lambda: lib.erm_last_error().decode()
    assert lib.erm_set_pointwise(eng._h, 3) == -1 and lib.erm_set_pointwise(eng._h, -1) == -1 and "unit" in err()        # ERM_ERR_ARG
    assert lib.erm_get_waic(eng._h, out.ctypes.data) == -3 and "not enabled" in err()                                    # ERM_ERR_STATE
    assert lib.erm_pointwise_units(eng._h) == 0
    assert lib.erm_set_pointwise(eng._h, L.POINTWISE_SUBJECT) == 0 and lib.erm_pointwise_units(eng._h) == 500
    eng.run(3)                                               # rows 0, 1 burn-in, one post-burn-in row
    assert lib.erm_get_waic(eng._h, out.ctypes.data) == -3 and "two post-burn-in rows" in err()
    assert lib.erm_get_pointwise(eng._h, None, None) == -3
    assert lib.erm_set_pointwise(eng._h, L.POINTWISE_CELL) == -3 and "no trace row" in err()                             # rows are recorded
    assert lib.erm_set_pointwise(eng._h, L.POINTWISE_OFF) == -3
    eng.run(3)
    assert lib.erm_get_waic(eng._h, out.ctypes.data) == 0 and out[5] == 500 and out[6] == 4
    lp = np.zeros(500)
    assert lib.erm_get_pointwise(eng._h, lp.ctypes.data, None) == 0 and lib.erm_get_pointwise(eng._h, None, None) == 0 and np.all(lp < 0)
    eng.reset_trace()
    eng.set_pointwise("cell")                                # allowed again; switching the unit re-allocates
    assert eng.pointwise_units == 500 * 9
    eng.run(6)
    _assert_equals_twin(eng, _twin(eng, "rtirt", n_iter=6, n_chain=1, n_burnin=2, unit="cell"), what="after the refusals")
    eng.close()
    # a subject-sharded engine
    sh = L.Engine(model=L.MODEL_RTIRT, n_item=9, n_subj=500, n_feat=3, n_iter=4, n_chain=1, n_burnin=2, cov2one=1, q_rt=0.5, seed=1, precision=L.PREC_F64, trace_mode=0)
    sh.set_shard(0, 1, 500, 0, lambda s, r, n: lib.erm_copy(r, s, n))
    assert lib.erm_set_pointwise(sh._h, L.POINTWISE_SUBJECT) == -3 and "sharding" in err()
    sh.set_data(Y, logT, X)
    sh.set_state(**init)
    sh.run(4)                                                # still usable
    sh.close()
    # accumulators that cannot be allocated: 12 000 000 x 896 cells need 344 GB (the engine itself, fp32 GibbsMlIrt without subject traces: 54 GB)
    big = L.Engine(model=L.MODEL_MLIRT, n_item=896, n_subj=12_000_000, n_feat=0, n_iter=2, n_chain=1, n_burnin=0, q_rt=0.5, seed=1, precision=L.PREC_F32, trace_mode=0)
    assert lib.erm_set_pointwise(big._h, L.POINTWISE_CELL) == -6 and "memory" in err()                                   # ERM_ERR_NOMEM
    assert lib.erm_pointwise_units(big._h) == 0
    assert lib.erm_set_pointwise(big._h, L.POINTWISE_SUBJECT) == 0 and lib.erm_pointwise_units(big._h) == 12_000_000
    big.close()


# ------------------------------------------------------------------------------------------------------------ full size
def test_full_size_rtirt_subject_unit():
    """GibbsRtIrt 100 000 x 50, fp64, default geometry, subject unit, four post-burn-in sweeps, against the twin."""
    Y, logT, X, init, tp = pu.make_problem("rtirt", 100_000, 50, 3, seed=21)
    eng = _engine("rtirt", Y, logT, X, init, n_iter=8, n_burnin=4, unit="subject")
    eng.run(8)
    _assert_equals_twin(eng, _twin(eng, "rtirt", n_iter=8, n_chain=1, n_burnin=4, unit="subject"), what="rtirt f64 subject 100000x50")
    eng.close()


def test_crossqr_nu_snapshot_inside_the_whole_call_graph():
    """GibbsRtIrtCrossQr 20 000 x 30, cell unit: the second erm_run replays ONE graph that holds run-begin, its four sweeps -- each with the copy of nu_t ahead of pass B
    and the pointwise pass behind it -- the closing step and run-end."""
    Y, logT, X, init, tp = pu.make_problem("crossqr", 20_000, 30, 3, seed=33)
    eng = _engine("crossqr", Y, logT, X, init, n_iter=8, n_burnin=3, unit="cell")
    eng.run(4)
    eng.run(4)
    _assert_equals_twin(eng, _twin(eng, "crossqr", n_iter=8, n_chain=1, n_burnin=3, unit="cell"), what="crossqr f64 cell 20000x30")
    eng.close()


# ------------------------------------------------------------------------------------------------------------ it discriminates
def test_waic_prefers_2pl_over_1pl_on_spread_discriminations():
    """GibbsMlIrt itemtype "2pl" against "1pl" on 600 x 12 data generated with discriminations 0.25 ... 3 (waic_util.spread_problem), 200 sweeps, subject unit, through
    the public interface: compareWaic must prefer 2pl by more than 2 se_diff.  Size and chain length were fixed on the CPU with the oracle chain and getWaicHost
    (tests/test_waic_host.py): its margin is 13.2 se_diff (elpd_diff 276.1, se_diff 20.85)."""
    pkg = pu.ge.load_package()
    Y, X, init = wu.spread_problem()
    Cond = pkg.setCond(nSubj=wu.SPREAD_N, nItem=wu.SPREAD_J, nFeat=1, nIter=wu.SPREAD_ITER, nChain=1)
    fits = {}
    for itemtype in ("2pl", "1pl"):
        M = pkg.GibbsMlIrt(Cond, Data=pkg.InputData(Y=Y, X=X), trace="summary")
        pkg.sample_b(M, itemtype=itemtype, waic="subject", fill=False)
        fits[itemtype] = (M, pkg.getWaic(M, pointwise=True))
    c = pkg.compareWaic(fits["2pl"][1], fits["1pl"][1])
    print(f"2pl {fits['2pl'][1]}\n1pl {fits['1pl'][1]}\n2pl - 1pl: elpd_diff {c['elpd_diff']:.4f}, se_diff {c['se_diff']:.4f}, margin {c['elpd_diff'] / c['se_diff']:.2f} se_diff")
    assert c["elpd_diff"] > 2.0 * c["se_diff"] > 0.0
    assert pkg.compareWaic(fits["2pl"][0], fits["1pl"][0]) == c          # samplers are accepted too
    for M, _ in fits.values():
        M.close()

"""Posterior predictive checks drawn and accumulated on the device (erm_set_predictive / erm_predictive_reps / erm_get_predictive): the chain does
not move when the pass is enabled, alone or next to WAIC, on any schedule; the accumulators equal getPpcHost, the numpy twin, evaluated on erm_get_data's data set and
the engine's own traces (means to 1e-10 relative, the device = host bound of tests/test_gpu_dic.py and tests/test_gpu_waic.py: no storage rounding enters; counts
exactly, but for units decided within 1e-9 of the compared magnitudes, at most 0.1 % of a case's units -- on the oracle chain there is none:
tests/test_predictive_host.py); bit-reproducibility; every refusal; the full size; and the 2pl-against-1pl misfit case through the public interface."""
import numpy as np
import pytest

import parity_util as pu
import ppc_util as ppu
import waic_util as wu

pytestmark = pytest.mark.gpu

MODELS = ppu.MODELS


def _engine(model, Y, logT, X, init, *, n_iter, n_chain=1, n_burnin, precision="f64", full=True, ppc=None, waic=None, flags=0, onepl=False, seed=1234, **opts):
    L = pu.ge.load_package()._lib
    N, J = Y.shape
    eng = L.Engine(model=pu.MODELS[model], n_item=J, n_subj=N, n_feat=0 if X is None else X.shape[1], n_iter=n_iter, n_chain=n_chain, n_burnin=n_burnin,
                   one_pl=int(onepl), cov2one=int(model not in ("latentqr", "latent")), q_rt=0.85, seed=seed, precision={"f32": 0, "f64": 1}[precision],
                   trace_mode=1 if full else 0, flags=flags, **opts)
    eng.set_data(Y, logT, X)
    if waic is not None:
        eng.set_pointwise(waic)
    if ppc is not None:
        eng.set_predictive(True, ppc)
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


def _device(eng, thin):
    pkg = pu.ge.load_package()
    item, subj, total = eng.predictive()
    return pkg.OutputPpc(R=eng.predictive_reps, thin=thin, item=item, subj=subj, total=total)


def _twin(eng, model, *, n_iter, n_chain, n_burnin, thin, sweep0=1, seed=1234):
    pkg = pu.ge.load_package()
    L = pkg._lib
    Y, logT, _ = eng.get_data()
    M = wu.as_sampler(model, Y, logT, eng.trace(L.TRACE_RA), None if model == "mlirt" else eng.trace(L.TRACE_RT), eng.trace(L.TRACE_QR), nIter=n_iter, nChain=n_chain,
                      nBurnin=n_burnin)
    return pkg.getPpcHost(M, thin=thin, sweep0=sweep0, seed=seed), M


def _bytes(eng):
    return tuple(np.ascontiguousarray(a).tobytes() for a in eng.predictive()) + (eng.predictive_reps,)


# ------------------------------------------------------------------------------------------------------------ nothing else moves
@pytest.mark.parametrize("precision", ["f64", "f32"])
@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("shape,flags", [((1000, 15), 0), ((20000, 24), 0), ((20000, 24), 1), ((20000, 24), 2)], ids=["persist-size", "graphs", "no-fuse", "no-graph"])
def test_chain_is_bit_identical_with_predictive_off_on_and_on_with_waic(model, precision, shape, flags):
    """1 000 x 15 is eligible for the persistent schedule: with the pass enabled the engine plans per-sweep launches at the same geometry (erm_timing.persistent == 0)
    and the chain equals the persistent chain bit for bit.  20 000 x 24 runs from captured graphs (two calls: block graphs, then the whole-call graph), under
    ERM_FLAG_NO_FUSE as two kernels per sweep and under ERM_FLAG_NO_GRAPH sweep by sweep.  The pass with WAIC next to it leaves the same accumulators as alone."""
    N, J = shape
    Y, logT, X, init, tp = pu.make_problem(model, N, J, 3, seed=13)
    got, acc = {}, {}
    for key, ppc, waic in (("off", None, None), ("on", 2, None), ("both", 2, "subject")):
        eng = _engine(model, Y, logT, X, init, n_iter=12, n_burnin=5, precision=precision, ppc=ppc, waic=waic, flags=flags)
        tm = eng.timing()
        if ppc is not None:
            assert tm["persistent"] == 0
        elif shape == (20000, 24) or model in ("crossqr", "cross"):
            assert tm["persistent"] == 0
        else:
            assert tm["persistent"] == 1
        eng.run(5)
        eng.run(7)
        tm = eng.timing()
        if ppc is None and shape == (1000, 15) and model not in ("crossqr", "cross"):
            assert tm["persistent"] == 1 or tm["persist_fallbacks"] > 0
        got[key] = _everything(eng, model)
        if ppc is not None:
            assert eng.predictive_reps == 4                 # post-burn-in rows 1, 3, 5, 7 of seven
            acc[key] = _bytes(eng)
        if waic is not None:
            assert eng.waic()["nRows"] == 7
        eng.close()
    assert got["on"] == got["off"] and got["both"] == got["off"]
    assert acc["both"] == acc["on"]


# ------------------------------------------------------------------------------------------------------------ values
@pytest.mark.parametrize("thin", [1, 2])
@pytest.mark.parametrize("precision", ["f64", "f32"])
@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("shape", [(1001, 17), (4000, 127)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_device_accumulators_equal_the_host_twin(model, precision, thin, shape):
    """nChain = 3 interleaved pseudo-chains, 6 iterations, burn-in 3: nine post-burn-in rows, every thin-th of them replicated."""
    N, J = shape
    Y, logT, X, init, tp = pu.make_problem(model, N, J, 3, seed=17)
    eng = _engine(model, Y, logT, X, init, n_iter=6, n_chain=3, n_burnin=3, precision=precision, ppc=thin)
    eng.run(18)
    assert eng.post_count == 9 and eng.predictive_reps == (9 if thin == 1 else 5)
    host, _ = _twin(eng, model, n_iter=6, n_chain=3, n_burnin=3, thin=thin)
    dev = _device(eng, thin)
    ppu.assert_equals_twin(dev, host, what=f"{model} {precision} thin {thin} {N}x{J}")
    ppu.check_counts(dev)
    eng.close()


def test_device_accumulators_at_896_items():
    """The longest test: 128 threads per workgroup, two subject slots of item sums in 115 KB of LDS."""
    Y, logT, X, init, tp = pu.make_problem("rtirt", 300, 896, 3, seed=19)
    eng = _engine("rtirt", Y, logT, X, init, n_iter=6, n_burnin=2, ppc=1)
    eng.run(6)
    host, _ = _twin(eng, "rtirt", n_iter=6, n_chain=1, n_burnin=2, thin=1)
    ppu.assert_equals_twin(_device(eng, 1), host, what="rtirt f64 300x896")
    eng.close()


def test_crossqr_nu_snapshot_inside_the_whole_call_graph():
    """GibbsRtIrtCrossQr 20 000 x 30 without WAIC: the copy of nu_t ahead of pass B is taken for the predictive pass alone, inside the replayed graph."""
    Y, logT, X, init, tp = pu.make_problem("crossqr", 20_000, 30, 3, seed=33)
    eng = _engine("crossqr", Y, logT, X, init, n_iter=8, n_burnin=3, ppc=1)
    eng.run(4)
    eng.run(4)
    host, _ = _twin(eng, "crossqr", n_iter=8, n_chain=1, n_burnin=3, thin=1)
    ppu.assert_equals_twin(_device(eng, 1), host, what="crossqr f64 20000x30")
    eng.close()


# ------------------------------------------------------------------------------------------------------------ reproducibility
@pytest.mark.parametrize("model,precision", [("rtirt", "f64"), ("crossqr", "f64"), ("latentqr", "f32"), ("mlirt", "f32")])
def test_two_engines_and_split_runs_leave_the_same_bits(model, precision):
    """Two engines agree bit for bit; run(3) + run(1) + run(3) leaves the accumulators of run(7); a summary-trace engine those of a full-trace one."""
    Y, logT, X, init, tp = pu.make_problem(model, 3000, 21, 3, seed=23)
    out = []
    for full, calls in ((True, (7,)), (True, (7,)), (True, (3, 1, 3)), (False, (7,)), (False, (3, 1, 3))):
        eng = _engine(model, Y, logT, X, init, n_iter=7, n_burnin=2, precision=precision, full=full, ppc=2)
        for n in calls:
            eng.run(n)
        assert eng.predictive_reps == 3
        out.append(_bytes(eng))
        eng.close()
    assert all(o == out[0] for o in out[1:])


def test_geometry_overrides_of_the_sweep_do_not_enter_the_pass():
    """The pass has a geometry of its own, a function of (nSubj, nItem) alone: lanes_per_row / block_threads / grid_blocks shape the sweep kernels only.  They do move the
    CHAIN in its last bits (its statistics are added in another order), so the comparison is made where the chains still agree to rounding: one sweep from the same
    state, no burn-in.  Counts are equal exactly; the means agree to 1e-10 relative -- they are sums of smooth functions of parameters that differ by a few ulp, not
    bit for bit, and the bound is the device = host bound of the twin comparison."""
    pkg = pu.ge.load_package()
    Y, logT, X, init, tp = pu.make_problem("rtirt", 5000, 20, 3, seed=37)
    res = []
    for opts in ({}, dict(block_threads=256, grid_blocks=100), dict(block_threads=512, grid_blocks=40, lanes_per_row=4)):
        eng = _engine("rtirt", Y, logT, X, init, n_iter=1, n_burnin=0, ppc=1, **opts)
        eng.run(1)
        res.append(_device(eng, 1))
        eng.close()
    for other in res[1:]:
        for a, b in ((res[0].item, other.item), (res[0].subj, other.subj), (res[0].total, other.total)):
            assert np.array_equal(a[:, :2], b[:, :2])
            assert np.all(np.abs(a[:, 2:] - b[:, 2:]) <= 1e-10 * np.abs(a[:, 2:]))


def test_reset_trace_and_set_seed_clear_the_accumulators():
    L = pu.ge.load_package()._lib
    Y, logT, X, init, tp = pu.make_problem("rtirt", 800, 11, 3, seed=29)
    eng = _engine("rtirt", Y, logT, X, init, n_iter=6, n_burnin=2, ppc=1)
    eng.run(6)
    first = _bytes(eng)
    assert eng.predictive_reps == 4
    eng.reset_trace()
    assert eng.predictive_reps == 0
    with pytest.raises(L.ErmError, match="at least one replicate row"):
        eng.predictive()
    eng.run(6)                                               # the chain goes on from where it was: sweeps 7 ... 12
    assert eng.predictive_reps == 4 and _bytes(eng) != first
    host, _ = _twin(eng, "rtirt", n_iter=6, n_chain=1, n_burnin=2, thin=1, sweep0=7)
    ppu.assert_equals_twin(_device(eng, 1), host, what="after erm_reset_trace")
    eng.reset_trace()
    eng.set_seed(99)                                         # a new chain: sweeps from 1 again, other streams
    eng.set_state(**{("lambda_" if k == "lam" else k): v for k, v in init.items()})
    eng.run(6)
    host, _ = _twin(eng, "rtirt", n_iter=6, n_chain=1, n_burnin=2, thin=1, sweep0=1, seed=99)
    ppu.assert_equals_twin(_device(eng, 1), host, what="after erm_set_seed")
    eng.close()


# ------------------------------------------------------------------------------------------------------------ refusals
def test_every_refusal_returns_its_code_and_leaves_the_engine_usable():
    pkg = pu.ge.load_package()
    L = pkg._lib
    lib = L.load()
    Y, logT, X, init, tp = pu.make_problem("rtirt", 500, 9, 3, seed=31)
    eng = _engine("rtirt", Y, logT, X, init, n_iter=6, n_burnin=2)
    err = lambda: lib.erm_last_error().decode()
    tot = np.zeros(8)
    persistent0 = eng.timing()["persistent"]
    assert lib.erm_set_predictive(eng._h, 1, 0) == -1 and "thin" in err() and lib.erm_set_predictive(eng._h, 1, -3) == -1          # ERM_ERR_ARG
    assert lib.erm_get_predictive(eng._h, None, None, tot.ctypes.data) == -3 and "not enabled" in err()                              # ERM_ERR_STATE
    assert lib.erm_predictive_reps(eng._h) == 0
    assert lib.erm_set_predictive(eng._h, 1, 2) == 0 and eng.timing()["persistent"] == 0
    assert lib.erm_get_predictive(eng._h, None, None, tot.ctypes.data) == -3 and "at least one replicate row" in err()               # R = 0
    eng.run(2)                                               # burn-in only
    assert lib.erm_predictive_reps(eng._h) == 0 and lib.erm_get_predictive(eng._h, None, None, None) == -3
    assert lib.erm_set_predictive(eng._h, 1, 1) == -3 and "no trace row" in err()                                                    # rows are recorded
    assert lib.erm_set_predictive(eng._h, 0, 1) == -3
    eng.run(4)
    assert lib.erm_predictive_reps(eng._h) == 2
    assert lib.erm_get_predictive(eng._h, None, None, tot.ctypes.data) == 0 and lib.erm_get_predictive(eng._h, None, None, None) == 0
    assert 0 <= tot[1] <= tot[0] <= 2 and tot[2] > 0
    host, _ = _twin(eng, "rtirt", n_iter=6, n_chain=1, n_burnin=2, thin=2)
    ppu.assert_equals_twin(_device(eng, 2), host, what="after the refusals")
    eng.reset_trace()
    eng.set_predictive(False)                                # off again: the persistent schedule returns
    assert eng.timing()["persistent"] == persistent0 and eng.predictive_reps == 0
    eng.close()
    # a subject-sharded engine
    sh = L.Engine(model=L.MODEL_RTIRT, n_item=9, n_subj=500, n_feat=3, n_iter=4, n_chain=1, n_burnin=2, cov2one=1, q_rt=0.5, seed=1, precision=L.PREC_F64, trace_mode=0)
    sh.set_shard(0, 1, 500, 0, lambda s, r, n: lib.erm_copy(r, s, n))
    assert lib.erm_set_predictive(sh._h, 1, 1) == -3 and "sharding" in err()
    sh.set_data(Y, logT, X)
    sh.set_state(**init)
    sh.run(4)                                                # still usable
    sh.close()
    # an engine with the pass enabled cannot become a shard
    en = L.Engine(model=L.MODEL_RTIRT, n_item=9, n_subj=500, n_feat=3, n_iter=4, n_chain=1, n_burnin=2, cov2one=1, q_rt=0.5, seed=1, precision=L.PREC_F64, trace_mode=0)
    en.set_predictive(True, 1)
    with pytest.raises(L.ErmError, match="sharding"):
        en.set_shard(0, 1, 500, 0, lambda s, r, n: lib.erm_copy(r, s, n))
    en.close()
    # the public interface
    Cond = pkg.setCond(nSubj=500, nItem=9, nFeat=3, nIter=4, nChain=1)
    M = pkg.GibbsRtIrt(Cond, Data=pkg.InputData(Y=Y, T=np.exp(logT), X=X))
    with pytest.raises(ValueError, match="chain farm"):
        pkg.sample_b(M, ppc=True, devices=[0])
    M.close()


# ------------------------------------------------------------------------------------------------------------ two switches, one path
@pytest.mark.parametrize("model,precision", [("crossqr", "f64"), ("cross", "f32")])
def test_one_pass_turned_off_leaves_the_other_as_if_alone(model, precision):
    """600 x 9 (two workgroups and the tail subject; the Cross family never runs persistent).  Both passes enabled, then one of them turned off again, in both orders:
    the pass that stays -- and for GibbsRtIrtCrossQr the copy of nu_t it reads -- leaves the accumulators of an engine that only ever had that pass, and the chain
    does not move."""
    Y, logT, X, init, tp = pu.make_problem(model, 600, 9, 3, seed=41)
    kw = dict(n_iter=6, n_burnin=2, precision=precision)
    a = _engine(model, Y, logT, X, init, waic="subject", ppc=1, **kw)
    a.set_pointwise(None)
    b = _engine(model, Y, logT, X, init, ppc=1, **kw)
    c = _engine(model, Y, logT, X, init, waic="subject", ppc=1, **kw)
    c.set_predictive(False)
    d = _engine(model, Y, logT, X, init, waic="subject", **kw)
    for eng in (a, b, c, d):
        eng.run(6)
    assert _bytes(a) == _bytes(b)
    assert c.waic() == d.waic() and [x.tobytes() for x in c.pointwise()] == [x.tobytes() for x in d.pointwise()]
    ref = _everything(a, model)
    assert all(_everything(eng, model) == ref for eng in (b, c, d))
    host, _ = _twin(a, model, n_iter=6, n_chain=1, n_burnin=2, thin=1)
    ppu.assert_equals_twin(_device(a, 1), host, what=f"{model} {precision} after WAIC was turned off")
    for eng in (a, b, c, d):
        eng.close()


def test_persistent_schedule_returns_only_when_the_last_pass_goes():
    """1 000 x 15 is eligible for the persistent schedule (erm_timing.persistent is 1 unless the occupancy check declined: compared with a fresh engine's)."""
    Y, logT, X, init, tp = pu.make_problem("rtirt", 1000, 15, 3, seed=13)
    ref = _engine("rtirt", Y, logT, X, init, n_iter=12, n_burnin=5)
    eng = _engine("rtirt", Y, logT, X, init, n_iter=12, n_burnin=5)
    p0 = eng.timing()["persistent"]
    assert p0 == ref.timing()["persistent"]
    eng.set_pointwise("subject")
    assert eng.timing()["persistent"] == 0
    eng.set_predictive(True, 1)
    assert eng.timing()["persistent"] == 0
    eng.set_pointwise(None)
    assert eng.timing()["persistent"] == 0
    eng.set_predictive(False)
    assert eng.timing()["persistent"] == p0
    for e in (eng, ref):
        e.run(5)
        e.run(7)
    assert _everything(eng, "rtirt") == _everything(ref, "rtirt")
    eng.close()
    ref.close()


def test_a_refused_switch_changes_nothing():
    """erm_set_pointwise on an engine with two rows recorded is refused; the replicate pass that was running goes on as on an engine that never received the call."""
    lib = pu.ge.load_package()._lib.load()
    Y, logT, X, init, tp = pu.make_problem("rtirt", 500, 9, 3, seed=31)
    out = []
    for refused in (True, False):
        eng = _engine("rtirt", Y, logT, X, init, n_iter=6, n_burnin=2, ppc=1)
        eng.run(2)
        if refused:
            assert lib.erm_set_pointwise(eng._h, 1) == -3 and "no trace row" in lib.erm_last_error().decode()
        eng.run(4)
        out.append((_bytes(eng), _everything(eng, "rtirt")))
        eng.close()
    assert out[0] == out[1]


# ------------------------------------------------------------------------------------------------------------ full size
def test_full_size_rtirt_summary_trace():
    """GibbsRtIrt 100 000 x 50, fp64, default geometry, summary-trace mode (no per-sweep theta / zeta is kept anywhere): 160 sweeps, the last 60 replicated.
    A posterior predictive p-value says something about the fit only once the chain has reached the posterior, and at this size the chain takes about a hundred
    sweeps from the test's initial values: on the oracle chain (CPU, same data and initial values) the total response discrepancy D_rep - D_obs falls from +2e4 in
    the first sweeps (every replicate above the data: ppp = 1, which is what eight sweeps give on the device too) to a fluctuation around zero; the share of rows
    with D_rep >= D_obs is 0.83 over sweeps 60-99, then 0.48 (100-149), 0.54 (150-199), 0.51 (100-199); response times 0.28, 0.62, 0.42, 0.52.  Hence burn-in 100.
    The laws of the replicates: D^T_rep is chi^2 with 50 degrees of freedom per subject; the item scores follow the Bernoulli means p_ij averaged over the replicate
    rows.  A summary-trace engine has no rows to average over, so a full-trace engine runs the same chain next to it: its accumulators must be the summary engine's
    bit for bit, and its theta / a / b rows are then the rows the summary engine replicated."""
    N, J, n_iter, burn = 100_000, 50, 160, 100
    Y, logT, X, init, tp = pu.make_problem("rtirt", N, J, 3, seed=21)
    eng = _engine("rtirt", Y, logT, X, init, n_iter=n_iter, n_burnin=burn, full=False, ppc=1)
    eng.run(n_iter)
    assert eng.predictive_reps == n_iter - burn
    P = _device(eng, 1)
    ppu.check_counts(P)
    ppu.check_rt_law(P, N, J)
    assert np.array_equal(P.item[2, 2], Y.sum(axis=0))
    print("  total ppp RA", P.ppp("total", "ra"), "RT", P.ppp("total", "rt"), "mid", P.ppp_mid("total", "ra"), P.ppp_mid("total", "rt"))
    assert 0.0 < P.ppp("total", "ra") < 1.0 and 0.0 < P.ppp("total", "rt") < 1.0
    acc = _bytes(eng)
    eng.close()
    L = pu.ge.load_package()._lib
    full = _engine("rtirt", Y, logT, X, init, n_iter=n_iter, n_burnin=burn, full=True, ppc=1)
    full.run(n_iter)
    assert _bytes(full) == acc
    ra = full.trace(L.TRACE_RA)
    full.close()
    ppu.check_score_law(P, ppu.mean_p(ra, N, J, ppu.replicate_rows(n_iter, 1, burn, 1)), N)


# ------------------------------------------------------------------------------------------------------------ it discriminates
def test_ppc_flags_the_1pl_fit_on_spread_discriminations():
    """GibbsMlIrt itemtype "2pl" against "1pl" on waic_util.spread_problem through the public interface, thresholds fixed on the CPU (ppc_util)."""
    pkg = pu.ge.load_package()
    Y, X, init = wu.spread_problem()
    Cond = pkg.setCond(nSubj=wu.SPREAD_N, nItem=wu.SPREAD_J, nFeat=1, nIter=wu.SPREAD_ITER, nChain=1)
    mid = {}
    for itemtype in ("2pl", "1pl"):
        M = pkg.GibbsMlIrt(Cond, Data=pkg.InputData(Y=Y, X=X), trace="summary")
        pkg.sample_b(M, itemtype=itemtype, ppc=True, fill=False)
        P = pkg.getPpc(M)
        assert P.R == wu.SPREAD_ITER - Cond.nBurnin and np.all(np.isnan(P.item[1]))
        mid[itemtype] = P.ppp_mid("item", "ra")
        print(itemtype, P, "item RA ppp_mid", np.round(mid[itemtype], 3))
        M.close()
    assert np.all(mid["2pl"] > ppu.BAND_2PL[0]) and np.all(mid["2pl"] < ppu.BAND_2PL[1])
    assert mid["1pl"][0] <= ppu.LOW_A_1PL_MAX and mid["1pl"][-1] >= ppu.HIGH_A_1PL_MIN

"""erm_get_rank_diagnostics / erm_get_rank_convergence / erm_debug_rank_diagnostics (rank_stage_kernel, rank_diag_kernel) against the independent reference of
tests/rank_diag_util.py: scipy's ranks and normal quantile, then diag_util's long-double estimator on the four transformed series.

Through the debug entry: the smallest shapes at which each mechanism can go wrong -- S = 8 (k = 1), an odd length, S = 78 (no power of two), M = 32 sequences,
several draws per lane; 1, 63, 65 and 193 columns (tiles and chunks with tails); both precisions (fp32 rounds the draws to float first, and so does the
reference's input); the edge columns of the definition; the refusals; bit-reproducibility, independence of the other columns and of the chunking, and
invariance under x -> 2 x.  Through the engine: every column of every trace of four models in both precisions against the reference on erm_get_trace's output,
the counters, the refusals, and that the call reads the engine only.

Tolerances are diag_util's: ESS within 1e-6 relative, R-hat within 1e-9 absolute, the NaN pattern exact; a column whose stop rule was decided by less than 1e-9
in any of its four series may be left out, at most one column in 1000 of a trace -- and none of the synthetic sets, which is asserted on the host first.
Every comparison prints one "RANK <case>: ..." line (run with -s).  Figures on record (MI355X, all 86 comparisons of this module): worst bulk-ESS error 7.2e-12
relative (GibbsRtIrtCrossQr qr, fp64), tail-ESS 7.9e-14, R-hat 6.7e-16; no column skipped anywhere; the module runs in under five seconds."""
import os
import re

import numpy as np
import pytest

import parity_util as pu
import rank_diag_util as ru

pytestmark = pytest.mark.gpu
pkg = pu.ge.load_package()
L = pkg._lib

SEED = 1
CAP = 8192
PREC = {"f32": 0, "f64": 1}
ERR = {"ARG": -1, "STATE": -3, "NONFINITE": -4, "NOTRACE": -5}


def _as(x, prec):
    return x if prec == "f64" else x.astype(np.float32).astype(np.float64)


_SETS = {}


def _set(nd, nc, prec):
    """193 synthetic columns and their reference, made once per (shape, precision) and left unchanged"""
    if (nd, nc, prec) not in _SETS:
        x = _as(ru.synthetic(nd, nc, max(ru.NCOLS), SEED), prec)
        _SETS[nd, nc, prec] = (x, ru.reference(x))
    return _SETS[nd, nc, prec]


def _cut(ref, k):
    return {key: (v[:k] if isinstance(v, np.ndarray) else v) for key, v in ref.items()}


def _compare(label, got, ref, cap=0.0):
    c = ru.compare(*got, ref)
    print(f"RANK {label}: columns {ref['constant'].size} compared {c['compared']} constant {int(ref['constant'].sum())} skipped {c['skipped']} "
          f"bulk_err {c['bulk_err']:.3e} tail_err {c['tail_err']:.3e} rhat_err {c['rhat_err']:.3e} min_margin {float(ref['margin'].min()):.3e}")
    bad = c["bad"][:8]
    assert c["bad"].size == 0, (label, bad, [np.asarray(g)[bad] for g in got], [np.asarray(ref[k][bad], dtype=float) for k in ("ess_bulk", "ess_tail", "rhat_rank")])
    assert c["skipped"] <= cap * ref["constant"].size, (label, c["skipped"])
    return c


@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("ncol", ru.NCOLS)
@pytest.mark.parametrize("nd,nc", ru.PAIRS)
def test_debug_entry_against_the_reference(nd, nc, ncol, prec):
    x, ref = _set(nd, nc, prec)
    assert float(ref["margin"].min()) >= ru.MARGIN_MIN, "the reference alone must skip no column of the synthetic sets"
    assert ref["fold_wins"].any() and not ref["fold_wins"].all(), "both branches of the max must occur"
    got = L.rank_diagnostics_device(x[:, :ncol, :], precision=PREC[prec])
    _compare(f"debug-{nd}x{nc}-{ncol}-{prec}", got, _cut(ref, ncol))


@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_edge_columns(prec):
    """constant -> three NaN; two-valued and evenly split -> R(z') undefined, rhat_rank = R(z); all ties but one (k = 2: U constant, no tail ESS; S = 8, k = 1: defined);
    the two zeros tie; infinities rank at the ends; a ramp."""
    x = _as(ru.edge_columns(20, 2), prec)
    ref = ru.reference(x)
    assert ref["constant"][0] and np.isnan(ref["rf"][1]) and ref["rhat_rank"][1] == ref["rz"][1] and np.isnan(ref["ess_tail"][2]) and not np.isnan(ref["ess_bulk"][2])
    got = L.rank_diagnostics_device(x, precision=PREC[prec])
    assert all(np.isnan(g[0]) for g in got)
    _compare(f"edge-20x2-{prec}", got, ref, cap=1.0)          # (no seed to choose here: a column may sit on its stop rule, the NaN pattern is still exact)
    x8 = np.full((8, 2, 1), 3.0)
    x8[2, 0, 0] = 7.0
    x8[:, 1, 0] = [0.0, -0.0, 1.0, -1.0, -0.0, 0.0, 1.0, -1.0]
    ref8 = ru.reference(x8)
    assert ref8["k"] == 1 and not np.isnan(ref8["ess_tail"][0])
    _compare(f"edge-8x1-{prec}", L.rank_diagnostics_device(x8, precision=PREC[prec]), ref8, cap=1.0)
    swapped = x8.copy()
    swapped[:, 1, 0] = [-0.0, 0.0, 1.0, -1.0, 0.0, -0.0, 1.0, -1.0]
    a, b = L.rank_diagnostics_device(x8, precision=PREC[prec]), L.rank_diagnostics_device(swapped, precision=PREC[prec])
    assert all(np.array_equal(u, v, equal_nan=True) for u, v in zip(a, b)), "-0.0 and +0.0 must tie"


def test_outputs_are_optional():
    x, ref = _set(64, 2, "f64")
    lib = L.load()
    xf = np.asfortranarray(x[:, :5, :])
    full = L.rank_diagnostics_device(xf)
    for q in range(3):
        out = np.empty(5)
        ptr = [None, None, None]
        ptr[q] = out.ctypes.data
        L.check(lib.erm_debug_rank_diagnostics(0, 1, xf.ctypes.data, 64, 5, 2, *ptr))
        assert np.array_equal(out, full[q], equal_nan=True)


def _code(exc):
    return int(re.match(r"libertirt error (-?\d+):", str(exc.value)).group(1))


def test_debug_entry_refusals_and_the_cap():
    g = np.random.default_rng(2)
    for shape in ((7, 3, 1), (8, 3, 17)):                       # fewer than 8 draws; 34 sequences
        with pytest.raises(L.ErmError) as e:
            L.rank_diagnostics_device(g.standard_normal(shape))
        assert _code(e) == ERR["ARG"], str(e.value)
    x = g.standard_normal((16, 4, 2))
    x[5, 2, 1] = np.nan
    for prec in (0, 1):
        with pytest.raises(L.ErmError) as e:
            L.rank_diagnostics_device(x, precision=prec)
        assert _code(e) == ERR["NONFINITE"], str(e.value)
    with pytest.raises(L.ErmError) as e:
        L.rank_diagnostics_device(g.standard_normal((CAP + 2, 1, 1)))
    assert _code(e) == ERR["ARG"] and str(CAP) in str(e.value), str(e.value)
    with pytest.raises(L.ErmError) as e:
        L.rank_diagnostics_device(g.standard_normal((2 * (CAP // 16) + 2, 1, 8)))
    assert _code(e) == ERR["ARG"] and str(CAP) in str(e.value), str(e.value)
    # S at the cap, in one chain and in sixteen
    for nd, nc in ((CAP, 1), (2 * (CAP // 32) + 1, 16)):
        xc = ru.synthetic(nd, nc, 6 if nc > 1 else 3, SEED)
        ref = ru.reference(xc)
        assert ref["S"] == CAP
        assert float(ref["margin"].min()) >= ru.MARGIN_MIN
        _compare(f"debug-cap-{nd}x{nc}", L.rank_diagnostics_device(xc), ref)


def test_determinism_and_invariance():
    x, _ = _set(200, 4, "f64")
    a, b = L.rank_diagnostics_device(x), L.rank_diagnostics_device(x)
    assert all(np.array_equal(u, v, equal_nan=True) for u, v in zip(a, b)), "two calls, identical bits"
    for k in (0, 64, 100, 192):                                 # a column alone against the same column among 193
        one = L.rank_diagnostics_device(x[:, k:k + 1, :])
        assert all(u[0] == v[k] for u, v in zip(one, a)), k
    y = L.rank_diagnostics_device(2.0 * x)
    assert np.array_equal(y[0], a[0]) and np.array_equal(y[1], a[1], equal_nan=True), "bulk and tail depend on the order only"
    assert np.array_equal(y[2], a[2]), "doubling is exact, so the folded series keeps its order too"
    os.environ["ERM_RANK_DIAG_CHUNK"] = "50"                    # 193 columns in chunks of 50, 50, 50, 43
    try:
        c = L.rank_diagnostics_device(x)
    finally:
        del os.environ["ERM_RANK_DIAG_CHUNK"]
    assert all(np.array_equal(u, v, equal_nan=True) for u, v in zip(a, c)), "the chunking must not show"


# ---------------------------------------------------------------------------------------------------------------- through the engine
SHAPES = {"rtirt": (300, 7), "latentqr": (300, 7), "crossqr": (120, 5), "mlirt": (300, 7)}
N_ITER, N_CHAIN, N_BURN = 40, 2, 20
_PROBLEMS = {}


def _problem(model, N, J):
    if (model, N, J) not in _PROBLEMS:
        _PROBLEMS[model, N, J] = pu.make_problem(model, N, J, 3)[:4]
    return _PROBLEMS[model, N, J]


def _traces(model):
    return [("ra", L.TRACE_RA)] + ([] if model == "mlirt" else [("rt", L.TRACE_RT)]) + [("qr", L.TRACE_QR)]


def _run(model, precision, **kw):
    N, J = SHAPES[model]
    Y, logT, X, init = _problem(model, N, J)
    return pu.run_device(model, Y, logT, X, init, N_ITER * N_CHAIN, precision=precision, n_chain=N_CHAIN, n_burnin=N_BURN, **kw)


@pytest.mark.parametrize("precision", ["f64", "f32"])
@pytest.mark.parametrize("model", list(SHAPES))
def test_every_column_of_every_trace(model, precision):
    d = _run(model, precision)
    eng = d["engine"]
    N, J = SHAPES[model]
    for name, which in _traces(model):
        before = eng.diagnostics(which)
        got = eng.rank_diagnostics(which)
        after = eng.diagnostics(which)
        assert all(np.array_equal(u, v, equal_nan=True) for u, v in zip(before, after)), "erm_get_diagnostics must not change"
        tr = d[name]
        assert all(g.shape == (tr.shape[1],) for g in got)
        ref = ru.reference(tr[N_BURN:])
        _compare(f"{model}-{precision}-{name}", got, ref, cap=ru.SKIP_CAP)
        assert eng.rank_convergence(which) == ru.counts6(*got), name
        if precision == "f64":                                   # the engine path and the debug entry run the same kernels on the same draws
            dbg = L.rank_diagnostics_device(tr[N_BURN:])
            assert all(np.array_equal(u, v, equal_nan=True) for u, v in zip(got, dbg)), name
    if model == "crossqr":                                       # [rho; vec(Sigp); vec(nu)]: the nu block is in device order on the device, in Julia's here
        assert d["qr"].shape[1] == J + 4 + N * J and not ref["constant"][J + 4:].any()
    if model == "mlirt":
        with pytest.raises(L.ErmError) as e:
            eng.rank_diagnostics(L.TRACE_RT)
        assert _code(e) == ERR["ARG"]


def _small_engine(model="rtirt", n_iter=16, n_chain=1, n_burnin=8, run=None, **kw):
    N, J = 64, 5
    Y, logT, X, init = _problem(model, N, J)
    eng = L.Engine(model=pu.MODELS[model], n_item=J, n_subj=N, n_feat=0 if X is None else X.shape[1], n_iter=n_iter, n_chain=n_chain, n_burnin=n_burnin,
                   cov2one=1, q_rt=0.85, seed=1234, precision=1, **{"trace_mode": 1, **kw})
    eng.set_data(Y, logT, X)
    eng.set_state(**{("lambda_" if k == "lam" else k): v for k, v in init.items()})
    eng.run(n_iter * n_chain if run is None else run)
    return eng


def _refused(eng, which, code, text=None):
    for query in (eng.rank_diagnostics, eng.rank_convergence):
        with pytest.raises(L.ErmError) as e:
            query(which)
        assert _code(e) == ERR[code], (query.__name__, str(e.value))
        assert text is None or text in str(e.value), str(e.value)


def test_engine_refusals_leave_the_engine_usable():
    e = _small_engine(n_iter=14, n_burnin=7)                     # fewer than 8 post-burn-in iterations
    _refused(e, L.TRACE_RA, "ARG")
    e = _small_engine(n_iter=8, n_burnin=0, n_chain=17)          # 34 sequences
    _refused(e, L.TRACE_RA, "ARG")
    e = _small_engine()
    _refused(e, L.TRACE_LOGLIKE, "ARG")
    e = _small_engine(run=10)                                    # rows still to run
    _refused(e, L.TRACE_RA, "STATE")
    e.run(6)
    _compare("after-incomplete-refusal-rt", e.rank_diagnostics(L.TRACE_RT), ru.reference(e.trace(L.TRACE_RT)[8:]), cap=1.0)
    e = _small_engine(trace_mode=0)                              # a SUMMARY engine keeps no subject-level trace
    for which in (L.TRACE_RA, L.TRACE_RT, L.TRACE_QR):
        _refused(e, which, "NOTRACE")
    e = _small_engine("crossqr", nu_trace_max_gb=1e-7)           # no resident nu trace: qr is refused, ra is not
    _refused(e, L.TRACE_QR, "NOTRACE")
    assert not np.isnan(e.rank_diagnostics(L.TRACE_RA)[0]).any()


def test_engine_at_the_cap_and_above():
    e = _small_engine(n_iter=CAP, n_burnin=0)                    # S = 8192
    cols = [0, 1, 63] + list(range(64, 74))                      # three subjects and the ten item columns: the reference at this length is slow
    got = e.rank_diagnostics(L.TRACE_RA)
    assert not any(np.isnan(g).any() for g in got)
    _compare("engine-cap-ra", [g[cols] for g in got], ru.reference(e.trace(L.TRACE_RA)[:, cols, :]), cap=1.0 / len(cols))
    e = _small_engine(n_iter=CAP + 2, n_burnin=0)
    _refused(e, L.TRACE_RA, "ARG", text=str(CAP))
    assert e.diagnostics(L.TRACE_RA)[0].shape == (64 + 10,)      # the basic estimator has no such cap


def test_the_chain_continues_unchanged_after_a_rank_call():
    def chain(ask):
        e = _small_engine(n_iter=16, n_chain=2, n_burnin=0)
        if ask:
            for which in (L.TRACE_RA, L.TRACE_RT, L.TRACE_QR):
                e.rank_diagnostics(which)
                e.rank_convergence(which)
        mean = e.get_mean()
        e.reset_trace()
        e.run(32)
        return mean, e.get_state(), e.trace(L.TRACE_RA)
    a, b = chain(False), chain(True)
    for u, v in zip(a[:2], b[:2]):
        assert set(u) == set(v) and all((u[k] is None and v[k] is None) or np.array_equal(u[k], v[k]) for k in u)
    assert np.array_equal(a[2], b[2])


@pytest.mark.parametrize("name,model", [("GibbsRtIrt", "rtirt"), ("GibbsRtIrtCrossQr", "crossqr"), ("GibbsMlIrt", "mlirt")])
def test_check_convergence_rank_counts_on_the_device_what_it_counts_on_the_host(name, model):
    N, J = SHAPES[model]
    Y, logT, X, init = _problem(model, N, J)
    Cond = pkg.setCond(nSubj=N, nItem=J, nFeat=0 if model == "crossqr" else 3, nIter=40, nChain=2, qRt=0.85)
    D = pkg.InputData(Y=Y, T=np.exp(logT) if logT is not None else np.ones_like(Y, dtype=float), X=X if X is not None else np.zeros((N, 0)))
    M = getattr(pkg, name)(Cond, Data=D, precision="f64")
    pkg.sample_b(M)
    full, short = pkg.checkConvergence(M, detail=True, kind="rank"), pkg.checkConvergence(M, detail=False, kind="rank")
    keys = ["ess", "essTail", "rhat", "essN", "essTailN", "rhatN"]
    assert list(short) == keys and list(full) == keys + ["detail"] and set(full["detail"]) == {n for n, _ in _traces(model)}
    for k in keys:
        assert full[k] == short[k], (k, full[k], short[k])
    tot = np.sum([ru.counts6(*v) for v in full["detail"].values()], axis=0)
    assert full["essN"] == f"{tot[1]} / {tot[0]}" and full["essTailN"] == f"{tot[3]} / {tot[2]}" and full["rhatN"] == f"{tot[5]} / {tot[4]}" and tot[0] > N
    basic = pkg.checkConvergence(M, detail=False)
    assert list(basic) == ["ess", "rhat", "essN", "rhatN"]
    for tr_name, which in _traces(model):
        _compare(f"mirror-{model}-{tr_name}", full["detail"][tr_name], ru.reference(getattr(M.Post, tr_name)[Cond.nBurnin:]), cap=ru.SKIP_CAP)

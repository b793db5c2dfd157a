"""erm_get_diagnostics / erm_get_convergence (diag_kernel, diag_count_kernel) against the independent longdouble reference of tests/diag_util.py: every column of
every trace of every model in both precisions, the split edges (n = 4, odd lengths, three and sixteen chains, a burn-in that is not half), the refusals, the
counters and the chain farm.  The reference is computed on the trace erm_get_trace returns -- for an fp32 engine the fp32 values -- so both sides see the same
numbers.  Tolerances: ESS within 1e-6 relative, R-hat within 1e-9 absolute; a column is NaN exactly where the reference's `constant` mask is set; a column whose
stop rule P_k > 0 was decided by less than 1e-9 may be left out, at most one column in 1000 of a trace.

Every test prints one "DIAG <case>: ..." line per trace (run with -s): the columns compared, constant and skipped, the worst |ess - e| / |e| and |rhat - r|, the
smallest ESS and the smallest stop margin.  Figures on record: the host twin `ess_rhat`, which carries the kernel's arithmetic, misses the reference by at most
2.9e-13 (ESS, relative) and 1.3e-14 (R-hat) over all columns of CPU-oracle chains of every shape used here, with 0 columns skipped per trace and a smallest stop
margin of 5e-6 (tests/test_diag_reference.py).  Device figures have not been recorded yet: this module had not run on an MI355X when it was written.
"""
import re

import numpy as np
import pytest

import diag_util as du
import parity_util as pu

pytestmark = pytest.mark.gpu
L = pu.ge.load_package()._lib

ALL_MODELS = ["mlirt", "rtirt", "latentqr", "crossqr", "null", "cross", "latent"]
ERR = {"ARG": -1, "STATE": -3, "NOTRACE": -5}          # include/ertirt.h: ERM_ERR_*


def _shape(model):
    return (120, 5) if model == "crossqr" else (300, 8)


def _traces(model):
    return [("ra", L.TRACE_RA)] + ([] if model == "mlirt" else [("rt", L.TRACE_RT)]) + [("qr", L.TRACE_QR)]


_PROBLEMS = {}


def _problem(model, N, J):
    """make_problem's data set and initial state, made once per (model, shape) and left unchanged."""
    key = (model, N, J)
    if key not in _PROBLEMS:
        _PROBLEMS[key] = pu.make_problem(model, N, J, 3)[:4]
    return _PROBLEMS[key]


def _run(model, precision, n_iter, n_chain, n_burnin, **kw):
    N, J = _shape(model)
    Y, logT, X, init = _problem(model, N, J)
    return pu.run_device(model, Y, logT, X, init, n_iter * n_chain, precision=precision, n_chain=n_chain, n_burnin=n_burnin, **kw)


def _check(eng, which, trace, n_burnin, label):
    """Every column of one trace: values, NaN pattern, skip cap; erm_get_convergence equal to the counts of the vectors the engine itself returned."""
    assert trace.shape[0] == eng.cfg.n_iter and trace.shape[2] == eng.cfg.n_chain
    ref = du.reference(trace[n_burnin:])
    ess, rhat = eng.diagnostics(which)
    assert ess.shape == rhat.shape == (trace.shape[1],)
    c = du.compare(ess, rhat, ref)
    print(f"DIAG {label}: columns {trace.shape[1]} compared {c['compared']} constant {int(ref['constant'].sum())} skipped {c['skipped']} "
          f"ess_err {c['ess_err']:.3e} rhat_err {c['rhat_err']:.3e} min_ess {np.nanmin(ess) if c['compared'] else float('nan'):.4g} "
          f"min_margin {float(ref['margin'].min()):.3e}")
    assert c["bad"].size == 0, (label, c["bad"][:10], ess[c["bad"]][:10], np.asarray(ref["ess"][c["bad"]][:10], dtype=float), rhat[c["bad"]][:10],
                                np.asarray(ref["rhat"][c["bad"]][:10], dtype=float))
    assert c["skipped"] <= du.SKIP_CAP * trace.shape[1], (label, c["skipped"])
    assert eng.convergence(which) == du.counts(ess, rhat), label
    return ref, ess, rhat


@pytest.mark.parametrize("precision", ["f64", "f32"])
@pytest.mark.parametrize("model", ALL_MODELS)
def test_every_column_of_every_trace(model, precision):
    N, J = _shape(model)
    d = _run(model, precision, 240, 2, 120)
    for name, which in _traces(model):
        ref, ess, rhat = _check(d["engine"], which, d[name], 120, f"{model}-{precision}-{name}")
        if name != "qr":
            assert not ref["constant"].any()
    if model == "crossqr":              # [rho; vec(Sigp); vec(nu)]: the 600 nu columns move and are compared in Julia's column-major order
        assert d["qr"].shape[1] == J + 4 + N * J and not ref["constant"][J + 4:].any()


@pytest.mark.parametrize("precision", ["f64", "f32"])
@pytest.mark.parametrize("cov2one", [True, False])
def test_null_reports_the_zero_betas_as_nan_and_the_right_sigma_columns(cov2one, precision):
    """GibbsRtIrtNull's qr is [vec(beta) = 0 (2 (F + 1) columns); vec(Sigma_p)]: the NaN block is written by the host, the Sigma_p columns are read from the item-level
    trace behind the two beta entries the kernels keep.  cov2one fixes the diagonal at 1 (NaN); without it all four entries move."""
    d = _run("null", precision, 240, 2, 120, cov2one=cov2one)
    ref, ess, rhat = _check(d["engine"], L.TRACE_QR, d["qr"], 120, f"null-{precision}-cov2one={cov2one}-qr")
    nb = 2 * (3 + 1)
    assert d["qr"].shape[1] == nb + 4 and np.all(d["qr"][:, :nb, :] == 0)
    assert np.all(np.isnan(ess[:nb])) and np.all(np.isnan(rhat[:nb]))
    want = [True, False, False, True] if cov2one else [False] * 4
    assert list(ref["constant"][nb:]) == want and list(np.isnan(ess[nb:])) == want
    _check(d["engine"], L.TRACE_RA, d["ra"], 120, f"null-{precision}-cov2one={cov2one}-ra")


@pytest.mark.parametrize("precision", ["f64", "f32"])
def test_one_pl_reports_the_discriminations_as_nan(precision):
    N, J = _shape("rtirt")
    d = _run("rtirt", precision, 240, 2, 120, onepl=True)
    ref, ess, rhat = _check(d["engine"], L.TRACE_RA, d["ra"], 120, f"rtirt-1pl-{precision}-ra")
    assert np.all(d["ra"][:, N:N + J, :] == 1)
    assert np.all(ref["constant"][N:N + J]) and int(ref["constant"].sum()) == J and np.all(np.isnan(ess[N:N + J])) and np.all(np.isnan(rhat[N:N + J]))


@pytest.mark.parametrize("n_iter,n_burnin,n_chain", [(8, 0, 1), (9, 0, 1), (30, 13, 3), (20, 4, 16), (64, 0, 1)])
@pytest.mark.parametrize("model,precision", [("rtirt", "f64"), ("latentqr", "f32")])
def test_split_edges(model, precision, n_iter, n_burnin, n_chain):
    """n = 4 (the minimum), an odd length (the second half starts at Tn - n, the middle draw is dropped), odd Tn = 17 with three interleaved chains after a burn-in
    that is not half, M = 32 sequences (the cap), and a plain even length."""
    d = _run(model, precision, n_iter, n_chain, n_burnin)
    for name, which in _traces(model):
        ref, _, _ = _check(d["engine"], which, d[name], n_burnin, f"{model}-{precision}-{n_iter}/{n_burnin}/{n_chain}-{name}")
        assert ref["n"] == (n_iter - n_burnin) // 2 and ref["M"] == 2 * n_chain


def _code(exc):
    return int(re.match(r"libertirt error (-?\d+):", str(exc.value)).group(1))


def _refused(eng, which, code):
    for query in (eng.diagnostics, eng.convergence):
        with pytest.raises(L.ErmError) as e:
            query(which)
        assert _code(e) == ERR[code], (query.__name__, str(e.value))


def _small_engine(model="rtirt", n_iter=16, n_chain=1, n_burnin=8, run=None, **kw):
    N, J = 64, 5
    Y, logT, X, init = _problem(model, N, J)
    eng = L.Engine(model=pu.MODELS[model], n_item=J, n_subj=N, n_feat=0 if X is None else X.shape[1], n_iter=n_iter, n_chain=n_chain, n_burnin=n_burnin,
                   cov2one=1, q_rt=0.85, seed=1234, precision=1, **{"trace_mode": 1, **kw})
    eng.set_data(Y, logT, X)
    eng.set_state(**{("lambda_" if k == "lam" else k): v for k, v in init.items()})
    eng.run(n_iter * n_chain if run is None else run)
    return eng


def test_refusals_return_their_code_and_leave_the_engine_usable():
    # fewer than 8 post-burn-in iterations
    e = _small_engine(n_iter=14, n_burnin=7)
    for which in (L.TRACE_RA, L.TRACE_RT, L.TRACE_QR):
        _refused(e, which, "ARG")
    assert e.trace(L.TRACE_RA).shape == (14, 64 + 10, 1) and e.post_count == 7
    # 2 * 17 sequences are more than the kernel holds
    e = _small_engine(n_iter=8, n_burnin=0, n_chain=17)
    _refused(e, L.TRACE_RA, "ARG")
    assert e.trace(L.TRACE_RA).shape == (8, 64 + 10, 17)
    # the logLike trace has no diagnostics; the engine answers the next valid query
    e = _small_engine()
    _refused(e, L.TRACE_LOGLIKE, "ARG")
    _check(e, L.TRACE_RA, e.trace(L.TRACE_RA), 8, "after-loglike-refusal-ra")
    # GibbsMlIrt has no rt trace
    e = _small_engine("mlirt")
    _refused(e, L.TRACE_RT, "ARG")
    _check(e, L.TRACE_QR, e.trace(L.TRACE_QR), 8, "after-mlirt-rt-refusal-qr")
    # rows still to run
    e = _small_engine(run=10)
    for which in (L.TRACE_RA, L.TRACE_QR):
        _refused(e, which, "STATE")
    e.run(6)
    _check(e, L.TRACE_RT, e.trace(L.TRACE_RT), 8, "after-incomplete-refusal-rt")
    # a SUMMARY engine keeps no subject-level trace
    e = _small_engine(trace_mode=0)
    for which in (L.TRACE_RA, L.TRACE_RT, L.TRACE_QR):
        _refused(e, which, "NOTRACE")
    assert e.item_trace().shape[0] == 16 and np.all(np.isfinite(e.get_mean()["theta"]))
    # GibbsRtIrtCrossQr whose budget does not hold the nu block: qr is refused, ra and rt are not
    e = _small_engine("crossqr", nu_trace_max_gb=1e-7)
    _refused(e, L.TRACE_QR, "NOTRACE")
    _check(e, L.TRACE_RA, e.trace(L.TRACE_RA), 8, "crossqr-no-nu-ra")
    _check(e, L.TRACE_RT, e.trace(L.TRACE_RT), 8, "crossqr-no-nu-rt")
    _refused(e, L.TRACE_QR, "NOTRACE")


LONG_ITER = 600          # M n = 2 * 2 * 150 = 600: the threshold ESS > 400 falls among the columns (tests/test_diag_reference.py checks that on an oracle chain)


@pytest.mark.parametrize("model", ["rtirt", "crossqr"])
def test_counters_equal_the_reference_counts_with_the_threshold_among_the_columns(model):
    d = _run(model, "f64", LONG_ITER, 2, LONG_ITER // 2)
    for name, which in _traces(model):
        ref, ess, rhat = _check(d["engine"], which, d[name], LONG_ITER // 2, f"{model}-long-{name}")
        got = d["engine"].convergence(which)
        e, r = np.asarray(ref["ess"], dtype=np.float64), np.asarray(ref["rhat"], dtype=np.float64)
        with np.errstate(invalid="ignore"):
            near = ~ref["constant"] & ((ref["margin"] < du.MARGIN_MIN) | (np.abs(e - 400.0) <= du.ESS_RTOL * 400.0) | (np.abs(r - 1.1) <= du.RHAT_ATOL))
        n_near = int(near.sum())
        assert n_near <= du.SKIP_CAP * e.size, (name, n_near)
        lo = du.counts(np.where(near, np.nan, e), np.where(near, np.nan, r))
        print(f"DIAG {model}-long-{name}: device counts {got} reference counts {lo} columns near a threshold {n_near}")
        assert all(a <= b <= a + n_near for a, b in zip(lo, got)), (name, got, lo, n_near)
        if name == "ra":
            assert np.sum(e > 400.0 * (1 + du.ESS_RTOL)) > 0 and np.sum(e < 400.0 * (1 - du.ESS_RTOL)) > 0, (np.nanmin(e), np.nanmax(e))
            assert 0 < got[1] < got[0]


def test_the_counters_on_their_thresholds():
    """diag_count_kernel on vectors that sit ON its thresholds (erm_debug_convergence runs the code erm_get_convergence runs): ESS > 400 and R-hat < 1.1 are strict,
    NaN enters no count, a negative or infinite value is defined.  300 001 values: more than the 1024 x 256 threads of the launch, so the grid-stride loop turns."""
    nan, up, dn = float("nan"), np.nextafter(400.0, np.inf), np.nextafter(400.0, -np.inf)
    ess = np.array([400.0, up, dn, nan, -120.0, np.inf, -np.inf, 0.0, 401.0, 399.0])
    rhat = np.array([1.1, np.nextafter(1.1, 2.0), np.nextafter(1.1, 0.0), nan, 1.0, np.inf, 0.0, nan, 1.1, 1.1])
    assert L.debug_convergence(ess, rhat) == du.counts(ess, rhat) == (9, 3, 8, 3)
    assert L.debug_convergence(np.full(7, 400.0), np.full(7, 1.1)) == (7, 0, 7, 0)
    g = np.random.default_rng(3)
    n = 300_001
    big_e, big_r = g.choice(ess, n), g.choice(rhat, n)
    assert L.debug_convergence(big_e, big_r) == du.counts(big_e, big_r)
    assert L.debug_convergence(ess[:1], rhat[:1]) == (1, 0, 1, 0)


@pytest.mark.parametrize("name,model", [("GibbsRtIrt", "rtirt"), ("GibbsRtIrtCrossQr", "crossqr"), ("GibbsRtIrtNull", "null"), ("GibbsMlIrt", "mlirt")])
def test_check_convergence_counts_on_the_device_what_it_counts_on_the_host(name, model):
    """checkConvergence(M, detail=False) (erm_get_convergence) against detail=True (the vectors, counted with numpy) through the Julia-surface mirror."""
    pkg = pu.ge.load_package()
    N, J = _shape(model)
    Y, logT, X, init = _problem(model, N, J)
    Cond = pkg.setCond(nSubj=N, nItem=J, nFeat=0 if model == "crossqr" else 3, nIter=60, nChain=2, qRt=0.85)
    D = pkg.InputData(Y=Y, T=np.exp(logT) if logT is not None else np.ones_like(Y, dtype=float), X=X if X is not None else np.zeros((N, 3 if model == "null" else 0)))
    M = getattr(pkg, name)(Cond, Data=D, precision="f64")
    pkg.sample_b(M)
    full, short = pkg.checkConvergence(M, detail=True), pkg.checkConvergence(M, detail=False)
    assert "detail" not in short and set(full["detail"]) == {n for n, _ in _traces(model)}
    for k in ("ess", "rhat", "essN", "rhatN"):
        assert full[k] == short[k], (k, full[k], short[k])
    ess_n = sum(int(np.sum(~np.isnan(e))) for e, _ in full["detail"].values())
    assert full["essN"].endswith(f" / {ess_n}") and ess_n > N
    for tr_name, which in _traces(model):
        _check(M._engine, which, getattr(M.Post, tr_name), Cond.nBurnin, f"mirror-{model}-{tr_name}")


def test_chain_farm_diagnoses_each_chain_on_its_own_slab():
    """Two chains on one device: Farm.engine(l).diagnostics(which) is the diagnostic of ONE chain (M = 2), equal to the reference on slab l of erm_farm_get_trace."""
    N, J, T = 300, 8, 40
    Y, logT, X, init = _problem("rtirt", N, J)
    farm = L.Farm([0, 0], model=pu.MODELS["rtirt"], n_item=J, n_subj=N, n_feat=3, n_iter=T, n_chain=1, n_burnin=T // 2, cov2one=1, q_rt=0.85, seed=1234,
                  precision=1, trace_mode=1)
    farm.set_data(Y, logT, X)
    for l in range(2):
        farm.set_state(l, **{("lambda_" if k == "lam" else k): v for k, v in init.items()})
    farm.run(T)
    seen = []
    for name, which in _traces("rtirt"):
        tr = farm.trace(which)
        assert tr.shape[2] == 2
        for l in range(2):
            ref, ess, _ = _check(farm.engine(l), which, tr[:, :, l:l + 1], T // 2, f"farm-chain{l}-{name}")
            assert ref["M"] == 2
            seen.append(ess)
    assert not np.array_equal(seen[0], seen[1], equal_nan=True)          # the chains differ: so do their diagnostics

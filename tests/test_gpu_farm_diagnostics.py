"""The chain farm's JOINT convergence diagnostics (erm_farm_get_diagnostics / _convergence / _rank_diagnostics / _rank_convergence): the estimators
of erm_get_diagnostics and erm_get_rank_diagnostics over the farm's L chains, chain l in the place of interleaved chain l, computed on chain 0's device from a
gathered view of the chains' resident traces (farm_gather_kernel) by the kernels the engine entries run.

Shapes: rtirt (f64) and latentqr (f32) at 300 x 8, crossqr (f64) at 120 x 5 -- its nu block is the device-order case --, n_iter = 40, n_burnin = 20, L in
{2, 3, 16} chains on device 0 that share one initial state and differ by their random streams.
  1. bit for bit the debug entries (erm_debug_diagnostics, erm_debug_rank_diagnostics: the same kernels on caller-supplied draws) on erm_farm_get_trace's
     post-burn-in rows, every column of every trace.  Subject-level columns are uploaded in the engine's precision; the item-level columns of an fp32 engine are
     fp64 on the device and are uploaded as such.
  2. the independent references (tests/diag_util.py, tests/rank_diag_util.py) on the same rows, with their tolerances and their skip cap.
  3. the result is cross-chain: it differs from one chain's own diagnostics, and a farm of ONE chain equals its engine's diagnostics bit for bit.
  4. the counts equal the counts of the vectors the farm returned.
  5. ERM_FARM_DIAG_CHUNK = 100, = 1, and ERM_FARM_DIAG_REMOTE = 1 (every chain but chain 0 through the slab path) change no bit.  Chunks are planned per trace
     BLOCK: under a cap of 100 the 300 subject columns go as 100 / 100 / 100 and the 16 item columns as one chunk; crossqr's 120 subject columns leave a tail of 20
     (fp64).  latentqr (f32) at 302 x 8 adds the widths that are no multiple of four: unset, each
     302-column block is ONE chunk that the gather copies one element a lane; under the cap a tail of 2 float columns follows three 16-byte chunks.
  6. the refusals return their codes and leave the farm usable.
  7. checkConvergence after sample_b(devices=[0]).
  8. chains on two devices (skipped on a box with one GPU).

The skip cap.  A column whose stop rule P_k > 0 was decided by less than 1e-9 may be left out of a value comparison (at most one column in 1000).  CPU-oracle
chains with chain ids 0 .. L - 1 at exactly these shapes, seeds and lengths, through diag_util.reference and rank_diag_util.reference: no column of any trace of
any of the nine (model, L) cases is below the threshold; the smallest margin is 9.4e-6 for the basic estimator (latentqr, L = 16, rt) and 2.6e-6 over the four
series of the rank estimator (latentqr, L = 3, rt).  On the MI355X (the device chains; fp32 for latentqr): no column skipped in any of the 54 comparisons, smallest
margin 6.2e-6; worst errors against the references 1.7e-12 (ESS, relative; bulk 8.7e-14, tail 4.2e-15) and 1.2e-14 (R-hat).

Every case prints "FARMDIAG <case>: ..." lines (run with -s): columns compared, constant and skipped, and the worst errors against the references."""
import re

import numpy as np
import pytest

import diag_util as du
import parity_util as pu
import rank_diag_util as ru

pytestmark = pytest.mark.gpu
L = pu.ge.load_package()._lib

N_ITER, N_BURN = 40, 20
MODELS = {"rtirt": "f64", "latentqr": "f32", "crossqr": "f64"}          # model -> the precision it is run in
CHAINS = (2, 3, 16)
CASES = [(m, n) for m in MODELS for n in CHAINS]
PREC = {"f32": L.PREC_F32, "f64": L.PREC_F64}
ERR = {"ARG": -1, "STATE": -3, "NOTRACE": -5}          # include/ertirt.h: ERM_ERR_*


def _shape(model):
    return (120, 5) if model == "crossqr" else (300, 8)


def _traces(model):
    return [("ra", L.TRACE_RA), ("rt", L.TRACE_RT), ("qr", L.TRACE_QR)]


_PROBLEMS, _FARMS = {}, {}


def _problem(model, N, J):
    key = (model, N, J)
    if key not in _PROBLEMS:
        _PROBLEMS[key] = pu.make_problem(model, N, J, 3)[:4]
    return _PROBLEMS[key]


def _make_farm(model, devices, *, shape=None, n_iter=N_ITER, n_burnin=N_BURN, run=None, **kw):
    N, J = shape or _shape(model)
    Y, logT, X, init = _problem(model, N, J)
    farm = L.Farm(devices, model=pu.MODELS[model], n_item=J, n_subj=N, n_feat=0 if X is None else X.shape[1], n_iter=n_iter, n_chain=1, n_burnin=n_burnin,
                  cov2one=int(model != "latentqr"), q_rt=0.85, seed=1234, precision=PREC[MODELS[model]], **{"trace_mode": 1, **kw})
    farm.set_data(Y, logT, X)
    for l in range(len(devices)):
        farm.set_state(l, **{("lambda_" if k == "lam" else k): v for k, v in init.items()})
    farm.run(n_iter if run is None else run)
    return farm


def _farm(model, n_chains):
    """One farm per (model, chains), run once; its post-burn-in traces and the diagnostics of the unset environment, fetched once and left unchanged."""
    key = (model, n_chains)
    if key not in _FARMS:
        farm = _make_farm(model, [0] * n_chains)
        out = dict(farm=farm, tr={}, basic={}, rank={})
        for name, which in _traces(model):
            out["tr"][which] = farm.trace(which)[N_BURN:]
            out["basic"][which] = farm.diagnostics(which)
            out["rank"][which] = farm.rank_diagnostics(which)
        _FARMS[key] = out
    return _FARMS[key]


def _subject_columns(model, which, width, shape=None):
    """The columns of a trace that come from a subject-level block (the engine's trace type); the others are item-level (fp64 whatever the precision)."""
    N, J = shape or _shape(model)
    m = np.zeros(width, dtype=bool)
    if which in (L.TRACE_RA, L.TRACE_RT):
        m[:N] = True
    else:
        nu = L.nu_len(pu.MODELS[model], N, J)
        m[width - nu:] = nu > 0
    return m


def _debug(model, which, tr, shape=None):
    """(ess, rhat), (bulk, tail, rhat_rank) of the debug entries on tr[draw, column, chain]: every column, each in the type its block has on the device."""
    subj = _subject_columns(model, which, tr.shape[1], shape)
    basic, rank = [np.empty(tr.shape[1]) for _ in range(2)], [np.empty(tr.shape[1]) for _ in range(3)]
    done = np.zeros(tr.shape[1], dtype=bool)
    for mask, prec in ((subj, PREC[MODELS[model]]), (~subj, L.PREC_F64)):
        if not mask.any():
            continue
        for dst, got in ((basic, L.debug_diagnostics(tr[:, mask, :], precision=prec)), (rank, L.rank_diagnostics_device(tr[:, mask, :], precision=prec))):
            for d, g in zip(dst, got):
                d[mask] = g
        done |= mask
    assert done.all()                                                  # no column left out
    return tuple(basic), tuple(rank)


def _same(a, b):
    return len(a) == len(b) and all(x.shape == y.shape and np.array_equal(x, y, equal_nan=True) for x, y in zip(a, b))


def _check_bit_exact(model, which, tr, got_basic, got_rank, label, shape=None):
    """The farm's vectors of one trace against the debug entries on its post-burn-in rows tr[draw, column, chain]: equal bit for bit, NaNs matched, every column."""
    basic, rank = _debug(model, which, tr, shape)
    assert got_basic[0].shape == (tr.shape[1],)
    assert _same(got_basic, basic), (label, "basic", np.flatnonzero(~((got_basic[0] == basic[0]) | np.isnan(basic[0])))[:10])
    assert _same(got_rank, rank), (label, "rank", np.flatnonzero(~((got_rank[0] == rank[0]) | np.isnan(rank[0])))[:10])
    assert np.isnan(got_basic[0]).sum() < tr.shape[1]                # something was computed


@pytest.mark.parametrize("model,n_chains", CASES)
def test_bit_exact_against_the_debug_entries(model, n_chains):
    f = _farm(model, n_chains)
    for name, which in _traces(model):
        tr = f["tr"][which]
        assert tr.shape[0] == N_ITER - N_BURN and tr.shape[2] == n_chains
        _check_bit_exact(model, which, tr, f["basic"][which], f["rank"][which], (model, n_chains, name))
    if model == "crossqr":              # [rho; vec(Sigp); vec(nu)]: the N * J nu columns come back in the caller's column-major order and all of them move
        N, J = _shape(model)
        assert f["tr"][L.TRACE_QR].shape[1] == J + 4 + N * J and not np.isnan(f["basic"][L.TRACE_QR][0][J + 4:]).any()


@pytest.mark.parametrize("model,n_chains", CASES)
def test_against_the_independent_references(model, n_chains):
    f = _farm(model, n_chains)
    for name, which in _traces(model):
        tr = f["tr"][which]
        ref = du.reference(tr)
        assert ref["M"] == 2 * n_chains and ref["n"] == (N_ITER - N_BURN) // 2
        ess, rhat = f["basic"][which]
        c = du.compare(ess, rhat, ref)
        print(f"FARMDIAG {model}-L{n_chains}-{name}: basic columns {tr.shape[1]} compared {c['compared']} constant {int(ref['constant'].sum())} skipped {c['skipped']} "
              f"ess_err {c['ess_err']:.3e} rhat_err {c['rhat_err']:.3e} min_margin {float(ref['margin'].min()):.3e}")
        assert c["bad"].size == 0, (model, n_chains, name, c["bad"][:10], ess[c["bad"]][:10], np.asarray(ref["ess"][c["bad"]][:10], dtype=float))
        assert c["skipped"] <= du.SKIP_CAP * tr.shape[1], (name, c["skipped"])
        rref = ru.reference(tr)
        bulk, tail, rr = f["rank"][which]
        rc = ru.compare(bulk, tail, rr, rref)
        print(f"FARMDIAG {model}-L{n_chains}-{name}: rank compared {rc['compared']} skipped {rc['skipped']} bulk_err {rc['bulk_err']:.3e} tail_err {rc['tail_err']:.3e} "
              f"rhat_err {rc['rhat_err']:.3e} min_margin {float(rref['margin'].min()):.3e}")
        assert rc["bad"].size == 0, (model, n_chains, name, rc["bad"][:10])
        assert rc["skipped"] <= ru.SKIP_CAP * tr.shape[1], (name, rc["skipped"])
        assert rref["S"] == 2 * n_chains * ((N_ITER - N_BURN) // 2)


def test_the_result_is_cross_chain():
    f = _farm("rtirt", 3)
    one = f["farm"].engine(0)
    for name, which in _traces("rtirt"):
        ess, rhat = f["basic"][which]
        e0, r0 = one.diagnostics(which)
        moving = ~np.isnan(rhat)
        assert np.array_equal(np.isnan(r0), ~moving) and moving.sum() >= 8
        assert np.all(rhat[moving] != r0[moving]) and np.all(ess[moving] != e0[moving]), name
        b0 = one.rank_diagnostics(which)
        assert np.all(f["rank"][which][2][moving] != b0[2][moving]), name


@pytest.mark.parametrize("model", list(MODELS))
def test_a_farm_of_one_chain_equals_its_engine(model):
    farm = _make_farm(model, [0])
    one = farm.engine(0)
    for name, which in _traces(model):
        assert _same(farm.diagnostics(which), one.diagnostics(which)), (model, name)
        assert _same(farm.rank_diagnostics(which), one.rank_diagnostics(which)), (model, name)
        assert farm.convergence(which) == one.convergence(which) and farm.rank_convergence(which) == one.rank_convergence(which)


@pytest.mark.parametrize("model,n_chains", CASES)
def test_counts_equal_the_counts_of_the_returned_vectors(model, n_chains):
    f = _farm(model, n_chains)
    for name, which in _traces(model):
        assert f["farm"].convergence(which) == du.counts(*f["basic"][which]), (model, n_chains, name)
        assert f["farm"].rank_convergence(which) == ru.counts6(*f["rank"][which]), (model, n_chains, name)


@pytest.mark.parametrize("model,n_chains", CASES)
def test_chunks_and_the_slab_path_change_no_bit(model, n_chains, monkeypatch):
    f = _farm(model, n_chains)
    for var, value in (("ERM_FARM_DIAG_CHUNK", "100"), ("ERM_FARM_DIAG_CHUNK", "1"), ("ERM_FARM_DIAG_REMOTE", "1")):
        monkeypatch.delenv("ERM_FARM_DIAG_CHUNK", raising=False)
        monkeypatch.delenv("ERM_FARM_DIAG_REMOTE", raising=False)
        monkeypatch.setenv(var, value)
        for name, which in _traces(model):
            assert _same(f["farm"].diagnostics(which), f["basic"][which]), (model, n_chains, name, var, value, "basic")
            assert _same(f["farm"].rank_diagnostics(which), f["rank"][which]), (model, n_chains, name, var, value, "rank")
            assert f["farm"].convergence(which) == du.counts(*f["basic"][which])
    monkeypatch.undo()
    which = L.TRACE_RA
    assert _same(f["farm"].diagnostics(which), f["basic"][which])


def test_block_widths_that_are_no_multiple_of_four(monkeypatch):
    """latentqr in fp32 with 302 subjects: theta, zeta and nu are 302-column float blocks.  Unset, each is one chunk of 302 columns (no 16-byte path: 302 floats are
    no whole number of 16 bytes); a cap of 100 leaves a tail of 2 float columns behind three wide chunks; a cap of 1; the slab path.  All equal the debug entries."""
    shape = (302, 8)
    farm = _make_farm("latentqr", [0] * 3, shape=shape)
    first = {}
    for var, value in ((None, None), ("ERM_FARM_DIAG_CHUNK", "100"), ("ERM_FARM_DIAG_CHUNK", "1"), ("ERM_FARM_DIAG_REMOTE", "1")):
        monkeypatch.delenv("ERM_FARM_DIAG_CHUNK", raising=False)
        monkeypatch.delenv("ERM_FARM_DIAG_REMOTE", raising=False)
        if var:
            monkeypatch.setenv(var, value)
        for name, which in _traces("latentqr"):
            got = farm.diagnostics(which), farm.rank_diagnostics(which)
            if var is None:
                tr = farm.trace(which)[N_BURN:]
                assert tr.shape[1] in (302 + 16, 9 + 302)                  # ra, rt: [subjects; 2 J items]; qr: [beta (5); vec(Sigp); nu]
                _check_bit_exact("latentqr", which, tr, got[0], got[1], ("302", name), shape)
                first[which] = got
            else:
                assert _same(got[0], first[which][0]) and _same(got[1], first[which][1]), (name, var, value)


def _code(exc):
    return int(re.match(r"libertirt error (-?\d+):", str(exc.value)).group(1))


def _refused(farm, which, code, match=None, queries=("diagnostics", "convergence", "rank_diagnostics", "rank_convergence")):
    for q in queries:
        with pytest.raises(L.ErmError) as e:
            getattr(farm, q)(which)
        assert _code(e) == ERR[code], (q, str(e.value))
        if match:
            assert re.search(match, str(e.value)), (q, str(e.value))


def test_refusals_return_their_code_and_leave_the_farm_usable():
    small = (64, 5)
    # 17 chains are 34 sequences: more than the kernels hold
    f = _make_farm("rtirt", [0] * 17, shape=small)
    _refused(f, L.TRACE_RA, "ARG", "too many chains")
    assert f.trace(L.TRACE_RA).shape == (N_ITER, 64 + 10, 17) and np.all(np.isfinite(f.engine(16).diagnostics(L.TRACE_RA)[0]))
    # six post-burn-in iterations
    f = _make_farm("rtirt", [0, 0], shape=small, n_iter=26, n_burnin=20)
    for which in (L.TRACE_RA, L.TRACE_RT, L.TRACE_QR):
        _refused(f, which, "ARG", "too few post-burn-in")
    assert f.post_count == 12 and np.all(np.isfinite(f.get_mean()["theta"]))
    # a SUMMARY farm keeps no subject-level trace
    f = _make_farm("rtirt", [0, 0], shape=small, trace_mode=0)
    for which in (L.TRACE_RA, L.TRACE_RT, L.TRACE_QR):
        _refused(f, which, "NOTRACE")
    assert np.all(np.isfinite(f.get_mean()["theta"]))
    # rows still to run: the message names the first chain that is short; the same farm answers once they have run
    f = _make_farm("rtirt", [0, 0], shape=small, run=30)
    for which in (L.TRACE_RA, L.TRACE_QR):
        _refused(f, which, "STATE", r"chain 0\b")
    f.run(N_ITER - 30)
    tr = f.trace(L.TRACE_RT)[N_BURN:]
    assert du.compare(*f.diagnostics(L.TRACE_RT), du.reference(tr))["bad"].size == 0
    # the logLike trace has no diagnostics; the next valid query is answered
    _refused(f, L.TRACE_LOGLIKE, "ARG")
    assert ru.compare(*f.rank_diagnostics(L.TRACE_RT), ru.reference(tr))["bad"].size == 0
    assert f.convergence(L.TRACE_RT) == du.counts(*f.diagnostics(L.TRACE_RT))
    # GibbsRtIrtCrossQr whose budget does not hold the nu block: qr is refused, ra is not
    f = _make_farm("crossqr", [0, 0], shape=small, nu_trace_max_gb=1e-7)
    _refused(f, L.TRACE_QR, "NOTRACE", "nu trace")
    assert du.compare(*f.diagnostics(L.TRACE_RA), du.reference(f.trace(L.TRACE_RA)[N_BURN:]))["bad"].size == 0
    # S = 2 * 16 * 257 = 8224 pooled draws are more than the rank kernel sorts: the rank entries refuse and name the cap, the basic ones answer
    f = _make_farm("rtirt", [0] * 16, shape=small, n_iter=514, n_burnin=0)
    _refused(f, L.TRACE_RA, "ARG", r"\b8192\b", queries=("rank_diagnostics", "rank_convergence"))
    ess, rhat = f.diagnostics(L.TRACE_RA)
    assert du.compare(ess, rhat, du.reference(f.trace(L.TRACE_RA)))["bad"].size == 0 and f.convergence(L.TRACE_RA) == du.counts(ess, rhat)


def test_check_convergence_after_a_farmed_sample():
    pkg = pu.ge.load_package()
    N, J = _shape("rtirt")
    Y, logT, X, init = _problem("rtirt", N, J)
    Cond = pkg.setCond(nSubj=N, nItem=J, nFeat=3, nIter=N_ITER, nChain=2, qRt=0.85)
    M = pkg.GibbsRtIrt(Cond, Data=pkg.InputData(Y=Y, T=np.exp(logT), X=X), precision="f64")
    pkg.sample_b(M, devices=[0])
    assert M.farm is not None and M._engine is None
    full, short = pkg.checkConvergence(M), pkg.checkConvergence(M, detail=False)
    assert "detail" not in short and set(full["detail"]) == {"ra", "rt", "qr"}
    for k in ("ess", "rhat", "essN", "rhatN"):
        assert full[k] == short[k], (k, full[k], short[k])
    tot = np.sum([du.counts(*full["detail"][n]) for n in ("ra", "rt", "qr")], axis=0)
    assert full["essN"] == f"{tot[1]} / {tot[0]}" and full["rhatN"] == f"{tot[3]} / {tot[2]}" and tot[0] > 2 * N
    rfull, rshort = pkg.checkConvergence(M, kind="rank"), pkg.checkConvergence(M, kind="rank", detail=False)
    for k in ("ess", "essTail", "rhat", "essN", "essTailN", "rhatN"):
        assert rfull[k] == rshort[k], (k, rfull[k], rshort[k])
    rtot = np.sum([ru.counts6(*rfull["detail"][n]) for n in ("ra", "rt", "qr")], axis=0)
    assert rshort["essN"] == f"{rtot[1]} / {rtot[0]}" and rshort["essTailN"] == f"{rtot[3]} / {rtot[2]}" and rshort["rhatN"] == f"{rtot[5]} / {rtot[4]}"
    # the vectors are the joint diagnostics of both chains: the reference on Post.ra over two chains
    ref = du.reference(M.Post.ra[Cond.nBurnin:])
    assert ref["M"] == 4 and du.compare(*full["detail"]["ra"], ref)["bad"].size == 0


def test_chains_on_two_devices():
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("the box shows fewer than two GPUs: chains on two devices cannot be placed")
    farm = _make_farm("rtirt", [0, 1])
    for name, which in _traces("rtirt"):
        tr = farm.trace(which)[N_BURN:]
        assert tr.shape[2] == 2
        _check_bit_exact("rtirt", which, tr, farm.diagnostics(which), farm.rank_diagnostics(which), ("two-devices", name))

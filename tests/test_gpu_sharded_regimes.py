"""Subject-sharded chains (include/ertirt.h erm_set_shard / erm_set_shard_rccl) where test_gpu_sharded.py does not go: every launch-geometry
regime of 128 to 896 items, more shards than the tiny step's GROUP = 16 rows per block, shards of one subject, data that differs between the shards, fp32
shards of every model, the in-stream RCCL exchange against the callback exchange bit for bit, and the engine's bookkeeping (split runs, interleaved chains,
trace modes, reseeding, state round trips, Post.mean, diagnostics, the DIC refusal) on shards.

A shard's statistics row is packed (shard_pack_kernel), gathered over the shards and read by the tiny step in place of the device's own group rows, with
N = the whole data set; WAIC, the predictive checks, DIC and erm_simulate_data are refused on a shard, so parity of the chain is the whole question.  The
reference for chain values is the fp64 CPU oracle on the UNSHARDED data; every bound is one the project already applies to the same comparison unsharded
(test_gpu_wide_items.py, test_gpu_data_extremes.py, test_gpu_post_mean.py, test_gpu_diagnostics.py).  All shards are engines of this one process on the one
card, driven by host threads (parallel.run_sharded_threads).  Every case prints its largest error by trace part (pytest -s)."""
import functools
import re

import numpy as np
import pytest

import diag_util as du
import parity_util as pu
import shard_util as su
import test_gpu_wide_items as wi
from parity_util import exe  # noqa: F401  (the compiled planner checker, a fixture)
from test_gpu_wide_items import cu_count  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu
L = pu.ge.load_package()._lib
F = wi.F
GROUP = 16                       # erm_kernels.hpp: rows the tiny step sums per block; the first block is prefetched into registers
ERR_STATE = -3                   # include/ertirt.h: ERM_ERR_STATE


def _check_oracle(label, res, tol=1e-8, floor=1e-6):
    parts = pu.rel_err_by_part(res, floor)
    print(f"\n[{label}] largest error by trace part (error, sweep, column): {parts}; bound {tol:g}")
    assert pu.max_rel_err(res, floor) < tol, (label, parts)


def _assert_shard_runs_plan(eng, p):
    tm = eng.timing()
    got = (tm["lanes_per_row"], tm["block_threads"], tm["grid_blocks"], tm["lds_bytes"], tm["persistent"])
    want = (p["W"], p["block_threads"], p["grid_blocks"], max(p["lds0"], p["lds1"]), 0)
    assert got == want, f"shard runs (W, threads, grid, lds, persistent) = {got}, the planner says {want}"


# ---------------------------------------------------------------------------------------------------------------
# 1. every geometry regime, two uneven shards, fp64
REGIME_J = (128, 129, 300, 400, 513, 641, 896)
REGIME_CASES = [(r, N + 1, J) for r, N, J in wi.F64_CASES if J in REGIME_J]          # odd totals: shards of (N + 2) / 2 and N / 2 subjects
ALL_MODELS_J = (129, 300, 896)
FEW_MODELS = ("rtirt", "latentqr", "crossqr")            # the fused sweep, 768-thread workgroups, two gathers per sweep


REGIME_PARAMS = [pytest.param(r, N, J, m, id=f"{r}-{N}-{J}-{m}") for r, N, J in REGIME_CASES for m in wi.MODELS if J in ALL_MODELS_J or m in FEW_MODELS]


@pytest.mark.parametrize("regime,N,J,model", REGIME_PARAMS)
def test_two_shards_in_every_regime(exe, cu_count, regime, N, J, model):
    """A shard's geometry is the PLAIN plan of its local N (pu.engine_plan without flags) with the `persist` field ignored: Engine::init plans before
    erm_set_shard is called, and erm_set_shard only turns the persistent schedule off (set_persist_avail(false)) -- it does not plan again, so a shard whose
    size the planner would run persistently keeps that plan's workgroups and launches them once per sweep.  (No shape of this test is of that size; parts 2
    and 4 hold such shards.)"""
    assert N % 2 == 1
    Y, logT, X, init, _ = pu.make_problem(model, N, J, F)
    T = wi.crossqr_sweeps(J) if model == "crossqr" else 4
    res = su.sharded_result(model, Y, logT, X, init, T, 2, oracle_threads=16 if N * J > wi.OMP_CELLS else 1)
    assert [n for _, n in res["rows"]] == [N // 2 + 1, N // 2]
    for eng, (_, n) in zip(res["engines"], res["rows"]):
        p = wi.planned(exe, cu_count, regime, model, "f64", n, J)
        assert eng.timing()["cu_count"] == cu_count
        _assert_shard_runs_plan(eng, p)
    tol, floor = wi.bound(J)
    _check_oracle(f"{model} f64 {N} x {J}, 2 shards, {regime}", res, tol, floor)


# ---------------------------------------------------------------------------------------------------------------
# 2. more shards than GROUP, and very small shards
def uneven_rows(N, count, big):
    """`count` ranges tiling [0, N): 3 subjects, `big` subjects, ONE subject, then the rest split near-equally."""
    rest, k = N - 4 - big, count - 3
    sizes = [3, big, 1] + [rest // k + (1 if r < rest % k else 0) for r in range(k)]
    assert len(sizes) == count and sum(sizes) == N and min(sizes) >= 1
    lo = np.concatenate([[0], np.cumsum(sizes)[:-1]])
    return [(int(a), int(n)) for a, n in zip(lo, sizes)]


@functools.lru_cache(maxsize=None)
def _many_problem(model, N, J):
    Y, logT, X, init, _ = pu.make_problem(model, N, J, F)
    T = 2 if model == "crossqr" else 4
    return Y, logT, X, init, T, su.oracle_chain(model, Y, logT, X, init, T)


def _many_shards(model, N, J, count, big):
    Y, logT, X, init, T, orc = _many_problem(model, N, J)          # the oracle chain is computed once per shape and left unchanged
    rows = uneven_rows(N, count, big)
    res = su.sharded_result(model, Y, logT, X, init, T, count, rows=rows, orc=orc)
    tm = [e.timing() for e in res["engines"]]
    assert rows[0][1] < 64 // tm[0]["lanes_per_row"], "shard 0 is to be smaller than the subjects one wave takes at a time"
    assert rows[2][1] == 1
    assert tm[1]["grid_blocks"] > 1 and all(t["persistent"] == 0 for t in tm)
    _check_oracle(f"{model} f64 {N} x {J}, {count} shards {[n for _, n in rows]}", res)


@pytest.mark.parametrize("count", [GROUP, GROUP + 1, 2 * GROUP + 1])
@pytest.mark.parametrize("model", ["rtirt", "crossqr"])
def test_more_shards_than_one_block_of_rows(model, count):
    """16, 17 and 33 shards: the gathered rows fill the register-prefetched block exactly, spill one row into the tiny step's second loop, and fill two
    blocks plus a tail.  The shards hold 3 subjects (fewer than a wave takes at a time), 500 (several workgroups), 1 (the engine accepts n_subj = 1) and
    near-equal parts of the rest."""
    _many_shards(model, 1001, 12, count, 500)


def test_seventeen_shards_at_a_wide_statistics_row():
    _many_shards("rtirt", 1001, 300, GROUP + 1, 500)


# ---------------------------------------------------------------------------------------------------------------
# 3. data that differs between the shards
SKEW_MODELS = ("rtirt", "latentqr", "crossqr", "mlirt")
SKEW_N, SKEW_J = 601, 12


@functools.lru_cache(maxsize=None)
def _skewed(model, key):
    """A data set whose shard 0 is unlike the whole: sorted (fastest / highest-scoring subjects first) or one of parity_util's offset kinds."""
    if key in pu.EXTREME_KINDS:
        Y, logT, X, init, _ = pu.make_extreme_problem(key, model, SKEW_N, SKEW_J, F)
        T = 2                                   # test_gpu_data_extremes.py compares runs of two sweeps from the oracle's state
    else:
        Y, logT, X, init, _ = pu.make_problem(model, SKEW_N, SKEW_J, F)
        order = np.argsort(logT.mean(axis=1), kind="stable") if key == "by_logT" else np.argsort(-Y.sum(axis=1, dtype=np.int64), kind="stable")
        Y, logT, X = Y[order], None if logT is None else logT[order], None if X is None else X[order]
        T = 2 if model == "crossqr" else 4
    Y, logT, X = np.asfortranarray(Y), None if logT is None else np.asfortranarray(logT), None if X is None else np.asfortranarray(X)
    return Y, logT, X, init, T, su.oracle_chain(model, Y, logT, X, init, T)


def _skew_cases():
    out = []
    for model in SKEW_MODELS:
        keys = (["by_logT"] if model != "mlirt" else []) + ["by_score"]
        keys += [k for k in ("rt_offset", "x_offset") if model in pu.extreme_models(k)]
        out += [pytest.param(model, k, c, id=f"{model}-{k}-{c}") for k in keys for c in (2, 3)]
    return out


@pytest.mark.parametrize("model,key,count", _skew_cases())
def test_shards_whose_data_differ(model, key, count):
    """Every shard's local column means, x'x and score sums are far from the whole data set's, so a local quantity where erm_set_data needs the all-summed
    one (the means logT is centred by, N, csq_j + N (m_j - mu)^2) moves the chain by far more than the bound.  1e-8 (floor 1e-6) on every trace column: the
    fp64 bound of test_gpu_data_extremes.py for the offset kinds, the sharded suite's for the sorted data."""
    Y, logT, X, init, T, orc = _skewed(model, key)
    if key == "by_logT":
        m = logT.mean(axis=1)
        assert m[:SKEW_N // count].mean() < m.mean() - 0.1 * m.std()
    res = su.sharded_result(model, Y, logT, X, init, T, count, orc=orc)
    _check_oracle(f"{model} f64 {SKEW_N} x {SKEW_J} {key}, {count} shards", res)


# ---------------------------------------------------------------------------------------------------------------
# 4. fp32 shards, every model
@pytest.mark.parametrize("model", wi.MODELS)
@pytest.mark.parametrize("N,J", [(3000, 20), (2000, 640)])
def test_f32_shards_one_sweep(exe, cu_count, N, J, model):
    """Two shards, one sweep from the oracle's state, judged by the rule of test_f32_wide_one_sweep (its constants are imported).  The share cap bounds how
    many subject draws may differ from the reference; the reference against itself has share 0, so no subject is left out on its side."""
    Y, logT, X, init, _ = pu.make_problem(model, N, J, F)
    res = su.sharded_result(model, Y, logT, X, init, 1, 2, precision="f32")
    for eng, (_, n) in zip(res["engines"], res["rows"]):
        p = wi.planned(exe, cu_count, None, model, "f32", n, J)
        _assert_shard_runs_plan(eng, p)
        if J == 640:
            assert p["rows_per_block"] == 1 and p["block_threads"] == 64 and p["grid_blocks"] == n == 1000, p
    dev = pu.decode_rows(model, N, J, F, res["dev_ra"], res.get("dev_rt"), res["dev_qr"])
    orc = pu.decode_rows(model, N, J, F, res["orc"]["ra"], res["orc"]["rt"] if model != "mlirt" else None, res["orc"]["qr"])
    items = {k: float(wi._abs_err(dev[k][0], orc[k][0]).max()) for k in ("a", "b", "lambda_", "sig2t") if k in dev}
    struct = {k: float(wi._abs_err(dev[k][0], orc[k][0]).max()) for k in ("beta", "rho", "sigp") if k in dev and dev[k].shape[1]}
    subj_err = {k: wi._abs_err(dev[k][0], orc[k][0]) for k in ("theta", "zeta", "nu") if k in dev}
    shares = {k: float(np.mean(e > wi.SUBJ_TOL)) for k, e in subj_err.items()}
    ll = abs(res["dev_ll"][0] - res["orc"]["ll"][0]) / abs(res["orc"]["ll"][0])
    cap = wi.share_cap(J)
    print(f"\n[{model} f32 {N} x {J}, 2 shards] share of subject draws beyond {wi.SUBJ_TOL:g}: {shares} (cap {cap:.3g}; largest "
          f"{({k: float(e.max()) for k, e in subj_err.items()})}); item draws {items}; structural {struct}; logLike {ll:.3g}")
    assert max(items.values()) < wi.ITEM_TOL, items
    assert not struct or max(struct.values()) < wi.ITEM_TOL, struct
    assert ll < wi.LL_TOL, ll
    assert max(shares.values()) < cap, shares


# ---------------------------------------------------------------------------------------------------------------
# 5. the RCCL path against the callback path
@pytest.mark.parametrize("N,J", [(301, 9), (151, 300)])
@pytest.mark.parametrize("model", ["rtirt", "latentqr", "crossqr", "cross"])
def test_rccl_exchange_equals_callback_exchange_bit_for_bit(model, N, J):
    """One shard through erm_set_shard_rccl (a one-rank communicator is all one card allows; 40 sweeps replay more than one 32-sweep graph, with the
    all-gathers captured -- two per sweep for the Cross family) against one shard through the callback (nothing captured, a host synchronisation per pass).
    The kernels, the pack and the summation order are the same and the exchange only copies: no tolerance."""
    T = 40
    Y, logT, X, init, _ = pu.make_problem(model, N, J, F)
    (cb,), _ = su.run_shards(model, Y, logT, X, init, T, 1)
    eng = L.Engine(model=pu.MODELS[model], n_item=J, n_subj=N, n_feat=0 if X is None else X.shape[1], n_iter=T, n_chain=1, n_burnin=T // 2,
                   cov2one=int(su.cov2one_of(model)), q_rt=0.85, seed=1234, precision=1, trace_mode=1)
    eng.set_shard_rccl(0, 1, N, 0, L.rccl_unique_id())
    eng.set_data(Y, logT, X)
    eng.set_state(**su.engine_state(init))
    eng.run(T)
    assert eng.timing()["persistent"] == 0 and cb.timing()["persistent"] == 0
    a, b = su.snapshot(eng, model), su.snapshot(cb, model)
    assert a["ra"].shape[0] == T and np.all(np.isfinite(a["ra"])) and np.all(np.isfinite(a["ll"]))
    su.assert_same_bits(a, b, f"{model} {N} x {J} rccl vs callback")


# ---------------------------------------------------------------------------------------------------------------
# 6. bookkeeping on shards
BK_N, BK_J = 601, 11
BK_CASES = [("rtirt", "f64"), ("crossqr", "f64"), ("latentqr", "f32")]


@functools.lru_cache(maxsize=None)
def _bk_problem(model):
    return pu.make_problem(model, BK_N, BK_J, F)[:4]


def _bk(model, precision, nsweeps, script=None, init=None, **kw):
    Y, logT, X, init0 = _bk_problem(model)
    return su.run_shards(model, Y, logT, X, init0 if init is None else init, nsweeps, 2, precision=precision, script=script, **kw)


def _snaps(engines, model, full=True):
    return [su.snapshot(e, model, full) for e in engines]


@pytest.mark.parametrize("model,precision", BK_CASES)
def test_split_runs_and_repeated_runs_leave_the_same_bits(model, precision):
    one, _ = _bk(model, precision, 7)
    again, _ = _bk(model, precision, 7)
    split, _ = _bk(model, precision, 7, script=lambda r, e: (e.run(3), e.run(1), e.run(3)))
    for r, (a, b, c) in enumerate(zip(_snaps(one, model), _snaps(again, model), _snaps(split, model))):
        assert a["ra"].shape[0] == 7 and np.all(np.isfinite(a["ra"]))
        su.assert_same_bits(a, b, f"{model} {precision} shard {r}: run(7) twice")
        su.assert_same_bits(a, c, f"{model} {precision} shard {r}: run(3) run(1) run(3) against run(7)")


def _f32_rule(label, model, N, J, dev_res, ref_res):
    """test_f32_wide_one_sweep's rule, sweep by sweep (`ref_res` holds the reference under the dev_* keys)."""
    dev = pu.decode_rows(model, N, J, F, dev_res["dev_ra"], dev_res.get("dev_rt"), dev_res["dev_qr"])
    ref = pu.decode_rows(model, N, J, F, ref_res["dev_ra"], ref_res.get("dev_rt"), ref_res["dev_qr"])
    worst = {}
    for k in dev:
        e = wi._abs_err(dev[k], ref[k])
        if not e.size:
            continue
        worst[k] = float(np.mean(e > wi.SUBJ_TOL, axis=1).max()) if k in ("theta", "zeta", "nu") else float(e.max())
    ll = float((np.abs(dev_res["dev_ll"] - ref_res["dev_ll"]) / np.abs(ref_res["dev_ll"])).max())
    print(f"\n[{label}] subject shares beyond {wi.SUBJ_TOL:g} / largest item and structural errors: {worst}; logLike {ll:.3g}")
    for k, v in worst.items():
        assert v < (wi.share_cap(J) if k in ("theta", "zeta", "nu") else wi.ITEM_TOL), (label, k, v)
    assert ll < wi.LL_TOL, (label, ll)


@pytest.mark.parametrize("model,precision", BK_CASES)
def test_interleaved_chains_fill_the_slabs_like_the_unsharded_engine(model, precision):
    """n_chain = 3: sweep m * 3 + l is row m of slab l.  GibbsRtIrt (6 sweeps) against the oracle under 1e-8; every case against an UNSHARDED device engine
    of the same configuration -- fp64 under the same 1e-8 (GibbsRtIrtCrossQr: 3 sweeps, as test_gpu_sharded.py free-runs it), fp32 under the rule of
    test_f32_wide_one_sweep (two fp32 chains differ by the summation order of their statistics, which can flip a rare Polya-Gamma decision)."""
    T = 6 if model == "rtirt" else 3
    Y, logT, X, init = _bk_problem(model)
    engines, rows = _bk(model, precision, T, n_chain=3)
    assert engines[0].trace(L.TRACE_RA).shape == (T // 3, rows[0][1] + 2 * BK_J, 3)
    res = su.concat_traces(model, engines, rows, BK_J, 0 if X is None else X.shape[1])
    res["model"] = model
    dev = pu.run_device(model, Y, logT, X, init, T, precision=precision, n_chain=3, n_burnin=(T // 3) // 2)
    whole = dict(model=model, dev_ra=pu.trace_rows(dev["ra"]), dev_qr=pu.trace_rows(dev["qr"]), dev_ll=pu.trace_rows(dev["ll"])[:, 0])
    if model != "mlirt":
        whole["dev_rt"] = pu.trace_rows(dev["rt"])
    label = f"{model} {precision} n_chain=3, 2 shards"
    if precision == "f64":
        _check_oracle(label + " vs unsharded device", dict(res, orc={k[4:]: v for k, v in whole.items() if k.startswith("dev_")}))
        if model == "rtirt":
            _check_oracle(label + " vs oracle", dict(res, orc=su.oracle_chain(model, Y, logT, X, init, T)))
    else:
        _f32_rule(label + " vs unsharded device", model, BK_N, BK_J, res, whole)


@pytest.mark.parametrize("model,precision", BK_CASES)
def test_summary_trace_shards_keep_what_full_trace_shards_keep(model, precision):
    full, _ = _bk(model, precision, 8)
    summ, _ = _bk(model, precision, 8, trace_mode=0)
    for r, (a, b) in enumerate(zip(_snaps(full, model, full=False), _snaps(summ, model, full=False))):
        assert int(a["post_count"]) == 4 and a["item"].shape[0] == 8
        su.assert_same_bits(a, b, f"{model} {precision} shard {r}: summary against full trace")


@pytest.mark.parametrize("model,precision", BK_CASES)
def test_reseeded_shards_equal_fresh_shards(model, precision):
    """reset_trace(); set_seed(s); set_state(init) on a chain that has run, against shards created with seed s.  `init` here is the WHOLE state a created
    engine starts from: make_problem's draws and the constructors' a = 1, b = 0, lambda = 0, sig2t = 1, nu = 1 (erm_set_state leaves a field it is not given
    as the chain left it)."""
    init = su.engine_state(_bk_problem(model)[3])
    init = dict(init, a=np.ones(BK_J), b=np.zeros(BK_J), lambda_=np.zeros(BK_J), sig2t=np.ones(BK_J))
    if model in pu.NU_MODELS:
        init["nu"] = np.ones(BK_N * BK_J if model == "crossqr" else BK_N)
    rows = pu.ge.load_package().parallel.shard_rows(BK_N, 2)

    def script(r, e):
        e.run(4)
        e.reset_trace()
        e.set_seed(99)
        e.set_state(**su.split_state(init, BK_N, *rows[r]))
        e.run(4)
    reused, _ = _bk(model, precision, 4, script=script)
    fresh, _ = _bk(model, precision, 4, seed=99)
    first, _ = _bk(model, precision, 4)
    for r, (a, b, c) in enumerate(zip(_snaps(reused, model), _snaps(fresh, model), _snaps(first, model))):
        su.assert_same_bits(a, b, f"{model} {precision} shard {r}: reseeded against fresh")
        assert not np.array_equal(a["ra"], c["ra"])          # the new seed is another chain


@pytest.mark.parametrize("model,precision", BK_CASES)
def test_state_round_trip_between_sets_of_shards(model, precision):
    """erm_get_state of every shard after run(4), installed in a second set of shards; both sets then run(4).  The random streams are addressed by the
    engine's sweep count, so the second set first makes four sweeps of its own, from ANOTHER initial state: its sweeps 5-8 from the installed state must
    then be the first set's sweeps 5-8, bit for bit in every trace row and in the final state (nu included: erm_get_state returns the nu the next sweep
    reads, and the second set reads exactly those values)."""
    Y, logT, X, init = _bk_problem(model)
    saved = [None, None]

    def first(r, e):
        e.run(4)
        saved[r] = {k: v for k, v in e.get_state().items() if v is not None}
        e.run(4)
    orig, _ = _bk(model, precision, 8, script=first)
    other = dict(init, theta=-np.asarray(init["theta"])[::-1].copy(), zeta=0.5 * np.asarray(init["zeta"])[::-1].copy())

    def second(r, e):
        e.run(4)
        e.set_state(**saved[r])
        e.run(4)
    copy, _ = _bk(model, precision, 8, script=second, init=other)
    for r, (a, b) in enumerate(zip(_snaps(orig, model), _snaps(copy, model))):
        assert not np.array_equal(a["ra"][:4], b["ra"][:4])
        for k in a:
            if k.startswith("state_"):
                assert np.array_equal(a[k], b[k]), (model, r, k)
            elif k in ("ra", "rt", "qr", "ll"):
                assert np.array_equal(a[k][4:], b[k][4:]), (model, r, k)
            elif k == "item":
                assert np.array_equal(a[k][4:], b[k][4:]), (model, r, k)


@pytest.mark.parametrize("model,precision", [(m, "f64") for m in wi.MODELS] + [("latentqr", "f32")])
def test_posterior_means_of_shards(model, precision):
    """erm_get_mean of every shard against pu.expected_mean of that shard's own trace rows within the rounding bound of test_gpu_post_mean.py
    (pu.mean_excess <= 1); the subject blocks concatenate over the shards, item and structural means are identical on every shard, bit for bit."""
    Y, logT, X, init = _bk_problem(model)
    engines, rows = _bk(model, precision, 8)
    Fx = 0 if X is None else X.shape[1]
    means = []
    for r, e in enumerate(engines):
        assert e.post_count == 4
        fields = pu.decode_rows(model, rows[r][1], BK_J, Fx, pu.trace_rows(e.trace(L.TRACE_RA)),
                                None if model == "mlirt" else pu.trace_rows(e.trace(L.TRACE_RT)), pu.trace_rows(e.trace(L.TRACE_QR)))
        mean, asum, n = pu.expected_mean(fields, 4, 1)
        got = e.get_mean()
        worst = {k: float(pu.mean_excess(got[k], mean[k], asum[k], n).max()) for k in fields if fields[k].shape[1]}
        print(f"\n[{model} {precision} shard {r}] n={n} |dev - trace mean| / bound: {worst}")
        assert all(v <= 1.0 for v in worst.values()), (model, r, worst)
        means.append(got)
    for k, v in means[0].items():
        if v is not None and k not in ("theta", "zeta", "nu"):
            assert np.array_equal(v, means[1][k]), k
    if precision == "f64":
        res = dict(su.concat_traces(model, engines, rows, BK_J, Fx), model=model)
        whole = pu.decode_rows(model, BK_N, BK_J, Fx, res["dev_ra"], res.get("dev_rt"), res["dev_qr"])
        mean, asum, n = pu.expected_mean(whole, 4, 1)
        for k in ("theta", "zeta"):
            if k in whole:
                cat = np.concatenate([m[k] for m in means])
                assert pu.mean_excess(cat, mean[k], asum[k], n).max() <= 1.0, k


def _traces(model):
    return [("ra", L.TRACE_RA)] + ([] if model == "mlirt" else [("rt", L.TRACE_RT)]) + [("qr", L.TRACE_QR)]


@pytest.mark.parametrize("model,precision", BK_CASES)
def test_diagnostics_of_a_shard_are_those_of_its_own_trace(model, precision):
    """erm_get_diagnostics / erm_get_convergence on every shard against tests/diag_util.py on the trace that shard returns (8 post-burn-in iterations; the
    bounds of test_gpu_diagnostics.py: ESS 1e-6 relative, R-hat 1e-9 absolute, the NaN pattern exact).  Item and structural columns are identical on every shard."""
    engines, rows = _bk(model, precision, 16)
    got = {}
    for r, e in enumerate(engines):
        for name, which in _traces(model):
            tr = e.trace(which)
            ref = du.reference(tr[8:])
            ess, rhat = e.diagnostics(which)
            c = du.compare(ess, rhat, ref)
            print(f"\nDIAG {model}-{precision}-shard{r}-{name}: columns {tr.shape[1]} compared {c['compared']} skipped {c['skipped']} ess_err {c['ess_err']:.3e} rhat_err {c['rhat_err']:.3e}")
            assert c["bad"].size == 0, (model, r, name, c["bad"][:10])
            assert c["skipped"] <= du.SKIP_CAP * tr.shape[1]
            conv = e.convergence(which)
            assert conv == du.counts(ess, rhat), (model, r, name)
            er, rr = np.asarray(ref["ess"], dtype=np.float64), np.asarray(ref["rhat"], dtype=np.float64)
            with np.errstate(invalid="ignore"):
                near = ~ref["constant"] & ((ref["margin"] < du.MARGIN_MIN) | (np.abs(er - 400.0) <= du.ESS_RTOL * 400.0) | (np.abs(rr - 1.1) <= du.RHAT_ATOL))
            lo = du.counts(np.where(near, np.nan, er), np.where(near, np.nan, rr))       # the reference's counts of the local trace
            assert all(a <= b <= a + int(near.sum()) for a, b in zip(lo, conv)), (model, r, name, conv, lo)
            got[r, name] = (ess, rhat)
    n0, n1 = rows[0][1], rows[1][1]
    for name, _ in _traces(model):
        for v0, v1 in zip(got[0, name], got[1, name]):
            if name == "qr":
                k = {"latentqr": F + 2 + 4, "crossqr": BK_J + 4}.get(model, v0.size)
                assert np.array_equal(v0[:k], v1[:k], equal_nan=True), name
            else:
                assert np.array_equal(v0[n0:], v1[n1:], equal_nan=True), name


def test_dic_is_refused_on_a_shard_and_the_chain_runs_on():
    Y, logT, X, init = _bk_problem("rtirt")
    seen = [None, None]

    def script(r, e):
        e.run(3)
        with pytest.raises(L.ErmError) as err:
            e.dic()
        seen[r] = str(err.value)
        e.run(3)
    engines, rows = _bk("rtirt", "f64", 6, script=script)
    for msg in seen:
        assert int(re.match(r"libertirt error (-?\d+):", msg).group(1)) == ERR_STATE, msg
        assert "erm_get_dic is not available on a shard" in msg, msg
    res = dict(su.concat_traces("rtirt", engines, rows, BK_J, X.shape[1]), model="rtirt", orc=su.oracle_chain("rtirt", Y, logT, X, init, 6))
    _check_oracle("rtirt f64 2 shards, 6 sweeps around a refused erm_get_dic", res)

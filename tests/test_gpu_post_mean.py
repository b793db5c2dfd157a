"""Post.mean, erm_post_count and the final state on every launch schedule.

Post.mean is what a user reads (coef / precis, the simulation studies' RMSE and bias, the D-hat half of every DIC), and the one output the
sweep kernels do not record as a trace: theta / zeta / nu are summed inside the row pass behind a device-side row counter, the divisor is
host arithmetic in erm_run, the item-level part is summed from the item trace.  Here every mean is recomputed from the engine's own FULL
traces (parity_util.decode_rows / expected_mean, pinned without a GPU in test_oracle_post_mean.py) and compared entry by entry:

 1. erm_post_count == max(0, rows_done - n_burnin * n_chain) after EVERY erm_run of a case, and the means read mid-way are the means of
    the rows recorded so far;
 2. every field of erm_get_mean against the trace mean within the rounding bound of parity_util.mean_excess: the device adds n rows in
    fp64 (<= (n - 1) u sum|x_t|) and multiplies by the rounded 1 / n (two more roundings); the reference side is summed in extended
    precision.  |dev - ref| <= (n + 2) u sum|x_t| / n.  The fp32 engine sums what it records, widened exactly, so the bound is the same.
    One row too many or too few moves a mean by ~1 / n of a draw's spread: 1e12 times the bound;
 3. fp64 engines: the same fields against the mean of the ORACLE's trace rows, 1e-8 relative (floor 1e-6), the suite's fp64 parity
    tolerance.  GibbsRtIrtCrossQr is chaotic beyond three sweeps (test_oracle_sweeps.py), so its long cases stop at check 2;
 4. erm_get_state after the last run is the last trace row bit for bit -- except nu: every schedule draws nu_{t+1} at the end of sweep t
    (include/ertirt.h, erm_get_state), so state-nu is positive, finite and becomes the nu ROW of the next recorded sweep
    (test_state_nu_is_the_next_sweeps_row).

Every case names its schedule and asserts it through erm_get_timing (persistent / grid_blocks / block_threads) and the flags it passed, so
a planner change cannot silently move a case to another path.  The graph-replay cases run 88 sweeps in ONE first call, which plan_run
(erm_schedule.hpp) enqueues as prologue + block graphs of 32, 32, 16, 4 and 4 sweeps: block edges at rows 32, 64, 80 and 84."""
import ctypes as C
import functools

import numpy as np
import pytest

import parity_util as pu

pytestmark = pytest.mark.gpu

L = pu.ge.load_package()._lib
N0, J0, F0 = 600, 11, 3                    # a persistent launch by default for the single-pass models
CROSS = ("crossqr", "cross")
FAMILIES = ("rtirt", "latentqr", "mlirt", "crossqr")          # one model per kernel family
FIELDS = {"mlirt": ("theta", "a", "b", "beta"),
          "rtirt": ("theta", "a", "b", "zeta", "lambda_", "sig2t", "beta", "sigp"),
          "null": ("theta", "a", "b", "zeta", "lambda_", "sig2t", "beta", "sigp"),
          "cross": ("theta", "a", "b", "zeta", "lambda_", "sig2t", "rho", "sigp"),
          "crossqr": ("theta", "a", "b", "zeta", "lambda_", "sig2t", "rho", "sigp", "nu"),
          "latent": ("theta", "a", "b", "zeta", "lambda_", "sig2t", "beta", "sigp"),
          "latentqr": ("theta", "a", "b", "zeta", "lambda_", "sig2t", "beta", "sigp", "nu")}
BOUNDARIES = (0, 1, 31, 32, 33, 63, 64, 65, 79, 80, 81, 84, 87)      # of 88 sweeps: on, beside and inside every graph block (32, 32, 16, 4, 4)

# name -> (engine options, what erm_get_timing must say).  "default" is the persistent launch for the single-pass models and the two-pass
# per-sweep schedule (graph replay) for the Cross family.
SCHEDULES = {
    "default": (dict(), dict()),
    "per_sweep": (dict(flags=L.FLAG_NO_PERSIST), dict(persistent=0)),
    "no_graph": (dict(flags=L.FLAG_NO_PERSIST | L.FLAG_NO_GRAPH), dict(persistent=0)),
    "two_kernel": (dict(flags=L.FLAG_NO_FUSE, block_threads=512, grid_blocks=32), dict(persistent=0, block_threads=512, grid_blocks=32)),
    "profile": (dict(profile=1), dict()),
    "many_rounds": (dict(block_threads=128, grid_blocks=1500), dict(persistent=0, block_threads=128, grid_blocks=1500)),
}


@functools.lru_cache(maxsize=None)
def _problem(model, N, J):
    return pu.make_problem(model, N, J, F0, seed=7)


def _nfeat(prob):
    return 0 if prob[2] is None else prob[2].shape[1]


def _engine(model, prob, *, n_iter, n_burnin, n_chain=1, precision="f64", sched="default", full=True, seed=1234, n_subj=None, load=True, **more):
    Y, logT, X, init, _ = prob
    opts, _ = SCHEDULES[sched]
    eng = L.Engine(model=pu.MODELS[model], n_item=Y.shape[1], n_subj=Y.shape[0] if n_subj is None else n_subj, n_feat=_nfeat(prob), n_iter=n_iter,
                   n_chain=n_chain, n_burnin=n_burnin, cov2one=int(model not in ("latentqr", "latent")), q_rt=0.85, seed=seed,
                   precision={"f32": L.PREC_F32, "f64": L.PREC_F64}[precision], trace_mode=L.TRACE_FULL if full else L.TRACE_SUMMARY, **opts, **more)
    if load:
        eng.set_data(Y, logT, X)
        eng.set_state(**_init_state(prob))
    return eng


def _init_state(prob):
    return {("lambda_" if k == "lam" else k): v for k, v in prob[3].items()}


def _assert_schedule(eng, model, sched):
    """The case is on the path it names: the flags it passed are the engine's, erm_get_timing reports the launch it planned."""
    opts, expect = SCHEDULES[sched]
    tm = eng.timing()
    assert eng.cfg.flags == opts.get("flags", 0) and eng.cfg.profile == opts.get("profile", 0)
    for k, v in expect.items():
        if k == "grid_blocks":          # the planner keeps the rows per workgroup of the requested grid and drops the workgroups that would be empty
            rpb = -(-eng.cfg.n_subj // v)
            v = -(-eng.cfg.n_subj // rpb)
        assert tm[k] == v, (sched, k, tm)
    if sched in ("default", "profile"):
        assert tm["persistent"] == (0 if model in CROSS else 1), (sched, tm)
    if sched == "many_rounds":
        assert tm["grid_blocks"] > tm["cu_count"]
    assert tm["persist_fallbacks"] == 0
    return tm


def _pull(eng, fn, which):
    """erm_get_mean / erm_get_state into NaN-filled buffers with a guard behind each: (values, fields the call left untouched)."""
    guard = 4
    raw = {k: (None if v is None else np.full(v.size + guard, np.nan)) for k, v in eng._state_buffers(which).items()}
    view = {k: (None if v is None else v[:v.size - guard]) for k, v in raw.items()}
    st, keep = L.state_struct(view)
    L.check(fn(eng._h, C.byref(st)))
    for k, v in raw.items():
        assert v is None or np.all(np.isnan(v[-guard:])), f"{k}: written past its end"
    untouched = {k for k, v in view.items() if v is not None and np.all(np.isnan(v))}
    return view, untouched


def _mean(eng, model, which=None):
    got, untouched = _pull(eng, L.load().erm_get_mean, FIELDS[model] if which is None else which)
    assert not untouched, untouched
    return got


def _state(eng, model):
    got, untouched = _pull(eng, L.load().erm_get_state, FIELDS[model])
    assert not untouched, untouched
    return got


def _fields(eng, model):
    """The engine's completed FULL traces, decoded: {field: rows x size}, rows in the order the sweeps ran.  A CrossQr engine without the
    budget for its nu trace decodes [rho; vec(Sigp)] from the item trace and has no nu."""
    c = eng.cfg
    N, J = c.n_subj, c.n_item
    ra = pu.trace_rows(eng.trace(L.TRACE_RA))
    rt = None if model == "mlirt" else pu.trace_rows(eng.trace(L.TRACE_RT))
    try:
        qr = pu.trace_rows(eng.trace(L.TRACE_QR))
    except L.ErmError:
        assert model == "crossqr"
        qr = eng.item_trace()[:, 4 * J:]
    return pu.decode_rows(model, N, J, c.n_feat, ra, rt, qr)


def _check_means(label, got, fields, n_burnin, n_chain, upto=None):
    """Check 2.  Prints every figure before it asserts (pytest -s / -rP shows them)."""
    if upto is not None:
        fields = {k: v[:upto] for k, v in fields.items()}
    mean, asum, n = pu.expected_mean(fields, n_burnin, n_chain)
    worst = {}
    for k in fields:
        assert got.get(k) is not None, (label, k)
        assert got[k].shape == mean[k].shape and np.all(np.isfinite(got[k])), (label, k)
        worst[k] = float(pu.mean_excess(got[k], mean[k], asum[k], n).max())
    print(f"{label}: n={n} |dev - trace mean| / bound: " + " ".join(f"{k}={v:.3g}" for k, v in worst.items()))
    bad = {k: v for k, v in worst.items() if not v <= 1.0}
    assert not bad, (label, n, bad)
    return mean


@functools.lru_cache(maxsize=None)
def _oracle_fields(model, N, J, rows, seed=1234):
    prob = _problem(model, N, J)
    Y, logT, X, init, _ = prob
    op = pu.OracleProblem(model, Y, logT, X, init, qRt=0.85, cov2one=model not in ("latentqr", "latent"), seed=seed)
    tr = op.run(rows, with_nu=model in pu.NU_MODELS)
    return pu.decode_rows(model, N, J, _nfeat(prob), tr["ra"], None if model == "mlirt" else tr["rt"], tr["qr"])


def _check_oracle(label, got, model, N, J, rows, n_burnin, n_chain, seed=1234, skip=0):
    """Check 3 (fp64 engines): against the oracle's rows skip .. skip + rows - 1 of the chain with this seed."""
    mean, _, _ = pu.expected_mean({k: v[skip:] for k, v in _oracle_fields(model, N, J, skip + rows, seed).items()}, n_burnin, n_chain)
    worst = {k: float(pu.rel_err(got[k], mean[k].astype(np.float64), 1e-6).max()) for k in mean if got.get(k) is not None}
    print(f"{label}: |dev - oracle mean| rel: " + " ".join(f"{k}={v:.3g}" for k, v in worst.items()))
    bad = {k: v for k, v in worst.items() if not v < 1e-8}
    assert not bad, (label, bad)


def _check_state(label, eng, model, fields):
    """Check 4: the final state is the last recorded row, bit for bit; nu is next sweep's draw (see the module docstring)."""
    st = _state(eng, model)
    for k, v in fields.items():
        if k == "nu":
            assert np.all(np.isfinite(st[k])) and np.all(st[k] > 0), (label, k)
        else:
            assert np.array_equal(st[k], v[-1]), (label, k)
    return st


def _run_case(model, *, n_iter, n_burnin, n_chain=1, precision="f64", sched="default", splits=None, N=N0, J=J0, oracle=None, label=None):
    label = label or f"{model}-{precision}-{sched}-burn{n_burnin}"
    prob = _problem(model, N, J)
    eng = _engine(model, prob, n_iter=n_iter, n_burnin=n_burnin, n_chain=n_chain, precision=precision, sched=sched)
    _assert_schedule(eng, model, sched)
    rows, burn = n_iter * n_chain, n_burnin * n_chain
    splits = (rows,) if splits is None else splits
    assert sum(splits) == rows
    done, midway = 0, []
    assert eng.post_count == 0
    for n in splits:
        eng.run(n)
        done += n
        assert eng.rows_done == done
        assert eng.post_count == max(0, done - burn), (label, done, eng.post_count)       # check 1
        if done > burn and done < rows:
            midway.append((done, _mean(eng, model)))
        elif done <= burn:
            with pytest.raises(L.ErmError, match="post-burn-in"):
                eng.get_mean()
    tm = _assert_schedule(eng, model, sched)
    if sched == "profile":
        assert tm["pass_launches"] > 0
    fields = _fields(eng, model)
    assert set(fields) == set(FIELDS[model])
    for upto, got in midway:
        _check_means(f"{label}@{upto}", got, fields, n_burnin, n_chain, upto=upto)
    got = None
    if rows > burn:
        got = _mean(eng, model)
        _check_means(label, got, fields, n_burnin, n_chain)
        if oracle if oracle is not None else (precision == "f64" and (model != "crossqr" or rows <= 3)):
            _check_oracle(label, got, model, N, J, rows, n_burnin, n_chain)
    _check_state(label, eng, model, fields)
    return eng, fields, got


# ----------------------------------------------------------------------------------------------------------- models, schedules
@pytest.mark.parametrize("precision", ["f64", "f32"])
@pytest.mark.parametrize("model", list(pu.MODELS))
def test_every_model_on_its_default_schedule(model, precision):
    """The persistent launch (single-pass models) / the two-pass schedule (Cross family), 24 sweeps with 9 burn-in, one erm_run."""
    eng, _, _ = _run_case(model, n_iter=24, n_burnin=9, precision=precision)
    eng.close()


def test_crossqr_f64_against_the_oracle_over_three_sweeps():
    eng, _, _ = _run_case("crossqr", n_iter=3, n_burnin=1)
    eng.close()


@pytest.mark.parametrize("precision", ["f64", "f32"])
@pytest.mark.parametrize("sched", ["per_sweep", "no_graph", "two_kernel", "profile", "many_rounds"])
@pytest.mark.parametrize("model", FAMILIES)
def test_schedules(model, sched, precision):
    """Per-sweep fused launches under graph replay, the same enqueued one by one, the two-kernel schedule, profile mode's event-bracketed
    launches and a grid of several rounds (6 000 x 7 in workgroups of two waves: more workgroups than compute units)."""
    size = dict(N=6000, J=7) if sched == "many_rounds" else {}
    eng, _, _ = _run_case(model, n_iter=24, n_burnin=9, precision=precision, sched=sched, **size)
    eng.close()


# ----------------------------------------------------------------------------------------------------------- where the boundary falls
@pytest.mark.parametrize("n_burnin", BOUNDARIES)
@pytest.mark.parametrize("model,precision,sched", [("rtirt", "f64", "per_sweep"), ("latentqr", "f64", "per_sweep"), ("rtirt", "f64", "default"),
                                                   ("latentqr", "f64", "default"), ("crossqr", "f32", "default")])
def test_boundary_positions_in_one_call_of_88_sweeps(model, precision, sched, n_burnin):
    """per_sweep: the burn-in boundary on each edge of, and inside, the replayed 32-sweep graphs, the 16- and the 4-sweep graphs (a graph is
    captured once and replayed with whatever row counter the device holds).  default: the same rows inside ONE persistent launch, where
    burn_rows is handed from sweep to sweep with the parameter block; CrossQr: the same graph blocks, two row passes per sweep."""
    eng, _, _ = _run_case(model, n_iter=88, n_burnin=n_burnin, precision=precision, sched=sched, N=300, J=7)
    eng.close()


@pytest.mark.parametrize("n_burnin", [2, 3, 4, 34, 35, 36, 66, 67, 68, 75, 87])
@pytest.mark.parametrize("model,precision,sched", [("rtirt", "f64", "per_sweep"), ("latentqr", "f64", "per_sweep"), ("rtirt", "f64", "default")])
def test_boundary_positions_in_a_continuing_call(model, precision, sched, n_burnin):
    """3 + 85 sweeps.  per_sweep: the second call finds the statistics resident and is run-begin, two replays of the 32-sweep block graph
    and a TAIL graph of 21 sweeps that also holds the closing step and run-end: block edges at rows 35 and 67, the tail behind.
    default: a persistent launch that starts at row 3 without a prologue."""
    eng, _, _ = _run_case(model, n_iter=88, n_burnin=n_burnin, precision=precision, sched=sched, splits=(3, 85), N=300, J=7)
    eng.close()


@pytest.mark.parametrize("splits", [(17, 23), (16, 1, 23), (18, 22), (5, 5, 5, 5, 20)], ids=lambda s: "+".join(map(str, s)))
@pytest.mark.parametrize("model,precision,sched", [("rtirt", "f64", "default"), ("rtirt", "f64", "per_sweep"), ("latentqr", "f64", "default"),
                                                   ("latentqr", "f64", "per_sweep"), ("latentqr", "f32", "two_kernel"), ("crossqr", "f32", "default")])
def test_boundary_between_calls(model, precision, sched, splits):
    """n_burnin = 17 of 40: the boundary at the end of a call, one row into the next, in a call of one sweep, inside a continuing call.  A
    continuing erm_run skips the prologue (and, per sweep, is ONE graph holding run-begin and run-end), so these are other launches than
    the single-call cases; the means read between the calls are checked too."""
    eng, _, _ = _run_case(model, n_iter=40, n_burnin=17, precision=precision, sched=sched, splits=splits, N=300, J=7)
    eng.close()


@pytest.mark.parametrize("splits", [(16, 20), (1, 14, 2, 19)], ids=lambda s: "+".join(map(str, s)))
@pytest.mark.parametrize("n_burnin", [0, 5, 11])
@pytest.mark.parametrize("model,precision,sched", [("rtirt", "f64", "default"), ("rtirt", "f64", "per_sweep"), ("latentqr", "f64", "default"),
                                                   ("latentqr", "f32", "per_sweep"), ("crossqr", "f32", "default")])
def test_three_interleaved_chains(model, precision, sched, n_burnin, splits):
    """n_chain = 3, n_iter = 12: 36 rows dealt round-robin to three slabs, n_burnin * 3 burn-in rows, calls split at rows that are no
    multiple of 3; the mean is over all slabs."""
    eng, _, _ = _run_case(model, n_iter=12, n_burnin=n_burnin, n_chain=3, precision=precision, sched=sched, splits=splits, N=300, J=7)
    eng.close()


# ----------------------------------------------------------------------------------------------------------- the state's nu
@pytest.mark.parametrize("model,precision,sched", [("latentqr", "f64", "default"), ("latentqr", "f32", "default"), ("latentqr", "f64", "per_sweep"),
                                                   ("latentqr", "f64", "no_graph"), ("latentqr", "f64", "two_kernel"), ("crossqr", "f64", "default"),
                                                   ("crossqr", "f32", "default"), ("crossqr", "f32", "no_graph")])
def test_state_nu_is_the_next_sweeps_row(model, precision, sched):
    """erm_get_state's nu after sweep t is nu_{t+1}: NOT the nu of trace row t (which entered Post.mean), but the nu row of the next
    recorded sweep -- shown by a second engine with one more row of capacity that runs the same chain one sweep further."""
    T = 10
    a, fa, _ = _run_case(model, n_iter=T, n_burnin=4, precision=precision, sched=sched, N=300, J=7)
    b = _engine(model, _problem(model, 300, 7), n_iter=T + 1, n_burnin=4, precision=precision, sched=sched)
    b.run(T)
    sa, sb = _state(a, model), _state(b, model)
    for k in sa:
        assert np.array_equal(sa[k], sb[k]), k
    assert not np.array_equal(sa["nu"], fa["nu"][-1])                 # one sweep ahead of the recorded row
    b.run(1)
    fb = _fields(b, model)
    for k, v in fa.items():
        assert np.array_equal(fb[k][:T], v), k
    assert np.array_equal(fb["nu"][T], sb["nu"])
    _check_means("one more row", _mean(b, model), fb, 4, 1)
    assert b.post_count == T + 1 - 4
    a.close(), b.close()


# ----------------------------------------------------------------------------------------------------------- nothing after burn-in
@pytest.mark.parametrize("model,precision,sched", [("rtirt", "f64", "default"), ("rtirt", "f32", "per_sweep"), ("latentqr", "f64", "default"),
                                                   ("latentqr", "f64", "per_sweep"), ("crossqr", "f32", "default")])
def test_all_rows_burn_in(model, precision, sched):
    """n_burnin == n_iter: no row enters the means; erm_get_mean and erm_get_dic refuse.  The draws are those of an engine with
    n_burnin = 0 (same chain), and an engine with the same burn-in and four more rows has means of exactly those four rows: the
    burn-in rows left the sums untouched."""
    T = 12
    prob = _problem(model, 300, 7)
    eng, f, got = _run_case(model, n_iter=T, n_burnin=T, precision=precision, sched=sched, splits=(7, 5), N=300, J=7)
    assert got is None and eng.post_count == 0
    for call in (eng.get_mean, eng.dic):
        with pytest.raises(L.ErmError, match="post-burn-in"):
            call()
    ref, f0, _ = _run_case(model, n_iter=T, n_burnin=0, precision=precision, sched=sched, N=300, J=7)
    for k, v in f0.items():
        assert np.array_equal(f[k], v), k
    more = _engine(model, prob, n_iter=T + 4, n_burnin=T, precision=precision, sched=sched)
    more.run(T)
    assert more.post_count == 0
    with pytest.raises(L.ErmError, match="post-burn-in"):
        more.get_mean()
    more.run(4)
    assert more.post_count == 4
    fm = _fields(more, model)
    for k, v in f0.items():
        assert np.array_equal(fm[k][:T], v), k
    _check_means("4 rows behind 12 of burn-in", _mean(more, model), fm, T, 1)
    for e in (eng, ref, more):
        e.close()


# ----------------------------------------------------------------------------------------------------------- reset_trace, set_seed
@pytest.mark.parametrize("model,precision,sched", [("rtirt", "f64", "default"), ("rtirt", "f64", "per_sweep"), ("latentqr", "f64", "default"),
                                                   ("latentqr", "f32", "per_sweep"), ("mlirt", "f32", "two_kernel"), ("crossqr", "f32", "default")])
def test_reset_trace_starts_the_means_over(model, precision, sched):
    """erm_reset_trace after post-burn-in rows: no rows, no means; the next n_iter rows burn in again from row 0 and their means hold
    nothing of the rows before."""
    T, nb = 20, 7
    eng, f1, m1 = _run_case(model, n_iter=T, n_burnin=nb, precision=precision, sched=sched, splits=(12, 8), N=300, J=7)
    eng.reset_trace()
    assert eng.rows_done == 0 and eng.post_count == 0
    with pytest.raises(L.ErmError, match="post-burn-in"):
        eng.get_mean()
    done = 0
    for n in (nb - 1, 2, T - nb - 1):
        eng.run(n)
        done += n
        assert eng.rows_done == done and eng.post_count == max(0, done - nb)
    _assert_schedule(eng, model, sched)
    f2 = _fields(eng, model)
    assert not np.array_equal(f2["theta"], f1["theta"])                # the chain went on
    m2 = _mean(eng, model)
    _check_means("after reset_trace", m2, f2, nb, 1)
    _check_state("after reset_trace", eng, model, f2)
    if precision == "f64":
        _check_oracle("after reset_trace", m2, model, 300, 7, T, nb, 1, skip=T)
    assert not np.array_equal(m2["theta"], m1["theta"])
    eng.close()


@pytest.mark.parametrize("model,precision,sched", [("rtirt", "f64", "default"), ("rtirt", "f32", "per_sweep"), ("latentqr", "f64", "default"),
                                                   ("latentqr", "f64", "per_sweep"), ("crossqr", "f32", "default")])
def test_set_seed_set_state_reset_trace_is_a_fresh_engine(model, precision, sched):
    """One engine serves every replication of a simulation condition: erm_set_seed + erm_set_state + erm_reset_trace, and the next run is the
    run of a freshly created engine with that seed, bit for bit -- traces, post count, means, state."""
    T, nb, seed = 20, 7, 99
    prob = _problem(model, 300, 7)
    eng, _, _ = _run_case(model, n_iter=T, n_burnin=nb, precision=precision, sched=sched, N=300, J=7)
    fresh = _engine(model, prob, n_iter=T, n_burnin=nb, precision=precision, sched=sched, seed=seed)
    start = {k: v for k, v in _state(fresh, model).items() if k != "nu"}      # the WHOLE start state, the constructor's a, b, lambda, sig2t included:
    eng.set_seed(seed)                                                          # erm_set_state skips NULL members, and the used engine's have moved
    eng.set_state(**start)                                                      # (nu is redrawn from the state by the first sweep after erm_set_seed)
    eng.reset_trace()
    assert eng.post_count == 0
    for e in (eng, fresh):
        for n in (nb, T - nb):
            e.run(n)
        assert e.post_count == T - nb
        _assert_schedule(e, model, sched)
    f, ff = _fields(eng, model), _fields(fresh, model)
    for k, v in ff.items():
        assert np.array_equal(f[k], v), k
    m, mf = _mean(eng, model), _mean(fresh, model)
    s, sf = _state(eng, model), _state(fresh, model)
    for k in ff:
        assert np.array_equal(m[k], mf[k]) and np.array_equal(s[k], sf[k]), k
    _check_means("after set_seed", m, f, nb, 1)
    _check_state("after set_seed", eng, model, f)
    if precision == "f64":
        _check_oracle("after set_seed", m, model, 300, 7, T, nb, 1, seed=seed)
    eng.close(), fresh.close()


# ----------------------------------------------------------------------------------------------------------- summary engines
@pytest.mark.parametrize("precision", ["f64", "f32"])
@pytest.mark.parametrize("model", list(pu.MODELS))
def test_summary_engine_means_are_the_means_of_the_full_traces(model, precision):
    """ERM_TRACE_SUMMARY keeps no subject-level trace: its means against the traces of a FULL engine on the same chain (the item traces and
    log-likelihood rows, which both keep, are identical)."""
    T, nb = 24, 9
    prob = _problem(model, N0, J0)
    full, fields, _ = _run_case(model, n_iter=T, n_burnin=nb, precision=precision)
    summ = _engine(model, prob, n_iter=T, n_burnin=nb, precision=precision, full=False)
    for n in (nb - 1, 2, T - nb - 1):
        summ.run(n)
    assert summ.post_count == T - nb
    _assert_schedule(summ, model, "default")
    assert np.array_equal(summ.item_trace(), full.item_trace()) and np.array_equal(summ.trace(L.TRACE_LOGLIKE), full.trace(L.TRACE_LOGLIKE))
    with pytest.raises(L.ErmError):
        summ.trace(L.TRACE_RA)
    _check_means(f"summary {model} {precision}", _mean(summ, model), fields, nb, 1)
    st = _state(summ, model)
    for k, v in fields.items():
        assert k == "nu" or np.array_equal(st[k], v[-1]), k
    full.close(), summ.close()


@pytest.mark.parametrize("precision", ["f64", "f32"])
@pytest.mark.parametrize("full", [True, False], ids=["full", "summary"])
def test_crossqr_keeps_the_nu_sums_without_the_nu_trace(full, precision):
    """nu_trace_max_gb too small for vec(nu) per sweep: Post.qr is refused, sum_nu is kept.  All N * J nu means against the nu trace of an
    engine that had the budget; the other fields against the engine's own traces."""
    T, nb = 16, 6
    prob = _problem("crossqr", N0, J0)
    ref, fields, _ = _run_case("crossqr", n_iter=T, n_burnin=nb, precision=precision)
    eng = _engine("crossqr", prob, n_iter=T, n_burnin=nb, precision=precision, full=full, nu_trace_max_gb=1e-9)
    eng.run(T)
    assert eng.post_count == T - nb
    with pytest.raises(L.ErmError):
        eng.trace(L.TRACE_QR)
    assert np.array_equal(eng.item_trace(), ref.item_trace())
    got = _mean(eng, "crossqr")
    assert got["nu"].size == N0 * J0
    _check_means("no nu trace", got, fields, nb, 1)
    if full:
        own = _fields(eng, "crossqr")
        assert "nu" not in own
        _check_means("no nu trace, own rows", got, own, nb, 1)
    ref.close(), eng.close()


# ----------------------------------------------------------------------------------------------------------- partial requests
@pytest.mark.parametrize("model,which", [("rtirt", "a"), ("rtirt", "theta"), ("latentqr", "nu"), ("crossqr", "nu"), ("crossqr", "rho"), ("mlirt", "beta")])
def test_partial_mean_requests(model, which):
    """erm_get_mean with one member set: the values of the full call, nothing written anywhere else (every other member is NULL; the
    requested buffer is followed by a guard)."""
    eng, _, full = _run_case(model, n_iter=12, n_burnin=5, N=300, J=7)
    got, untouched = _pull(eng, L.load().erm_get_mean, (which,))
    assert not untouched
    assert [k for k, v in got.items() if v is not None] == [which]
    assert np.array_equal(got[which], full[which])
    wrapped = eng.get_mean((which,))
    assert np.array_equal(wrapped[which], full[which]) and all(v is None for k, v in wrapped.items() if k != which)
    eng.close()


# ----------------------------------------------------------------------------------------------------------- a sharded chain
@pytest.mark.parametrize("model,precision", [("latentqr", "f64"), ("crossqr", "f64"), ("crossqr", "f32")])
def test_sharded_chain_means(model, precision):
    """Two shards of one chain on the one GPU: each shard's theta / zeta / nu means are the means of its LOCAL trace block (so the
    concatenation is the trace mean of the whole chain); item and structural means are identical on both shards."""
    N, J, T, nb = 301, 7, 3 if model == "crossqr" else 14, 1 if model == "crossqr" else 5
    pkg = pu.ge.load_package()
    prob = _problem(model, N, J)
    Y, logT, X, init, _ = prob

    def make_engine(n_local):
        return _engine(model, prob, n_iter=T, n_burnin=nb, precision=precision, n_subj=n_local, load=False)

    engines = pkg.parallel.run_sharded_threads(make_engine, 2, N, Y, logT, X, _init_state(prob), T)
    rows = pkg.parallel.shard_rows(N, 2)
    means, parts = [], []
    for r, eng in enumerate(engines):
        assert eng.timing()["persistent"] == 0 and eng.cfg.n_subj == rows[r][1]
        assert eng.post_count == T - nb
        f = _fields(eng, model)
        got = _mean(eng, model)
        _check_means(f"shard {r}", got, f, nb, 1)
        _check_state(f"shard {r}", eng, model, f)
        means.append(got)
        parts.append(f)
    for k in FIELDS[model]:
        if k not in ("theta", "zeta", "nu"):
            assert np.array_equal(means[0][k], means[1][k]), k
    # the concatenated local means are the means of the concatenated traces, and (fp64) of the oracle's unsharded chain
    whole = {k: np.concatenate([p[k] for p in parts], axis=1) for k in ("theta", "zeta")}
    cat = {k: np.concatenate([m[k] for m in means]) for k in ("theta", "zeta")}
    if model == "crossqr":
        whole["nu"] = np.concatenate([p["nu"].reshape(T, rows[r][1], J, order="F") for r, p in enumerate(parts)], axis=1).reshape(T, N * J, order="F")
        cat["nu"] = np.concatenate([m["nu"].reshape(rows[r][1], J, order="F") for r, m in enumerate(means)], axis=0).reshape(-1, order="F")
    else:
        whole["nu"] = np.concatenate([p["nu"] for p in parts], axis=1)
        cat["nu"] = np.concatenate([m["nu"] for m in means])
    _check_means("shards concatenated", cat, whole, nb, 1)
    if precision == "f64":
        cat.update({k: means[0][k] for k in FIELDS[model] if k not in cat})
        _check_oracle("shards concatenated", cat, model, N, J, T, nb, 1)
    for eng in engines:
        eng.close()

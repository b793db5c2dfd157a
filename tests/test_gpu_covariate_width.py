"""Sweep parity across covariate counts: every covariate model (mlirt, rtirt, latent, latentqr, null) from n_feat = 1 up to the limit of 14 = PMAX - 2.

n_feat is one of the sweep kernel's three size inputs and the only one the rest of the GPU suite holds at 3.  The structural wave is written in terms of
p = n_feat + 1 and PMAX = 16: GibbsRtIrt's Cholesky is 2p x 2p (30 x 30 at the limit), GibbsRtIrtLatent inverts q = p + 1 = 16 = PMAX columns, LatentQr
with sigp_mode = 1 walks a packed triangle of 136 Gram entries, beta is two columns of leading dimension PMAX whose first ends one slot before the second
begins; every subject parks n_feat + 2 (+ 4) values in LDS, so n_feat alone moves a shape between the planner's schedules.  The reference is the fp64 CPU
oracle, which allocates by nFeat and has no PMAX.

  1. the width axis at 300 x 9, six free-running fp64 sweeps, n_feat in {1, 2, 7, 13, 14}, automatic geometry (the persistent schedule), with
     ERM_FLAG_NO_PERSIST bit for bit the same chain; intercept = True at 14 (the only setting in which slots 0 and p of beta are non-zero at the limit);
     LatentQr with sigp_mode = 1 at 13 and 14; one-wave workgroups (block_threads = 64) at 14.
  2. each edge where n_feat alone changes the plan: 6000 x 7, block_threads = 256, grid_blocks = 8, four sweeps, on the last fused-and-persistent
     n_feat and on the next one (two kernels per sweep), the plan asserted as a property and as what erm_get_timing reports; one refusal
     (grid_blocks = 6, n_feat = 14) in erm_create with the planner's message.
  3. fp32 at the limit: one sweep from the oracle's state at 2000 x 25, test_f32_one_sweep's rule, the structural block included.
  4. what runs behind the sweep at n_feat = 14: DIC, the marginal WAIC (and its refusal of 15), the predictive checks, sharded chains, the chain farm,
     erm_simulate_data, the positions of every beta slot in Post.qr / erm_get_state / Post.mean and the state round trip.
  5. on the CPU (not marked gpu): fused / persist are monotone in n_feat -- once lost, never regained -- and 15 is refused.
     tests/geometry_check.cpp's sweep visits Fk in {0, 1, 3, 7, 14}, LatentQr at each of them with ngx = 0 and with sigp_mode 1's ngx (153 at 14).

No new tolerance: every comparison has the bound the same comparison has at n_feat = 3.  fp64: every trace column of every sweep within 1e-8 relative
(floor 1e-6).  That bound is meaningful at these widths because the reference determines the runs far more tightly -- the oracle against its own twin
started one ulp apart (theta moved by nextafter, the method of test_crossqr_chain_is_chaotic), largest relative difference over ra, rt and qr with the
same floor, on the exact shapes and sweep counts used here:
    300 x 9, six sweeps      mlirt 3.3e-13   rtirt 7.1e-13   latent 6.3e-13   latentqr 2.6e-12   null 3.1e-12   (largest over n_feat in 1, 2, 7, 13, 14)
                             intercept at 14: rtirt 3.8e-12, latent 4.7e-13;   latentqr sigp_mode 1: 4.5e-13 at 13, 3.9e-11 at 14 (sweep 5)
    6000 x 7, four sweeps    mlirt 1.3e-11 / 2.0e-12 (13 / 14)   rtirt 3.8e-11 / 1.1e-11 (13 / 14)   latent 3.7e-12 / 6.9e-12 (11 / 12)
                             latentqr 3.7e-12 / 2.6e-11 (11 / 12)   latentqr sigp_mode 1 5.6e-12 / 2.1e-10 (10 / 11)
    600 x 9, four sweeps     rtirt 2.7e-13   latent 6.0e-13   (14)
The device's own distance from the oracle, largest error by trace part over the cases of each section (measured on an MI355X; every case prints its own
with pytest -s):
    1. 300 x 9, n_feat 1 ... 14      mlirt ra 1.5e-12 qr 8.3e-14 (at 14)   rtirt ra 1.3e-12 rt 3.4e-11 (at 1) qr 1.4e-13   latent ra 5.1e-12 rt 2.9e-12 qr 6.9e-14
                                     latentqr ra 5.1e-12 rt 1.3e-11 qr 2.0e-12   null ra 2.0e-12 rt 5.4e-12 qr 6.5e-13   logLike 4.3e-15 at most
       at 14: intercept              rtirt ra 1.3e-11 rt 1.0e-12 qr 1.2e-13   latent ra 7.3e-13 rt 1.3e-12 qr 6.1e-14
       latentqr sigp_mode 1          13: ra 9.9e-13 rt 2.1e-13 qr 1.1e-13   14: ra 7.3e-13 rt 4.5e-11 qr 7.9e-13 (the twin: 3.9e-11)
       block_threads 64 at 14        rtirt ra 7.0e-14 rt 1.1e-12 qr 1.7e-14   latent ra 8.4e-13 rt 5.3e-13 qr 1.2e-13   latentqr ra 8.4e-13 rt 3.2e-12 qr 1.0e-12
       the ERM_FLAG_NO_PERSIST engine equalled the persistent one bit for bit in all 29 persistent cases
    2. 6000 x 7 (fused / two-kernel) mlirt 13 / 14: ra 1.5e-11 / 2.1e-12 qr 6.0e-14 / 6.7e-14   rtirt 13 / 14: ra 8.6e-11 / 5.3e-12 rt 4.3e-11 / 9.6e-12 qr 9.1e-14 / 2.2e-13
                                     latent 11 / 12: ra 5.3e-11 / 3.9e-11 rt 1.8e-11 / 2.2e-10 qr 8.1e-15 / 1.5e-14
                                     latentqr 11 / 12: ra 5.3e-11 / 3.9e-11 rt 3.3e-11 / 2.5e-10 qr 2.7e-12 / 7.2e-12
                                     latentqr sigp_mode 1, 10 / 11: ra 1.2e-10 / 5.3e-11 rt 9.0e-11 / 2.2e-10 qr 1.7e-11 / 2.6e-12 (the twin: 5.6e-12 / 2.1e-10)
                                     after the refusal, rtirt n_feat 3 with 6 workgroups: ra 9.5e-11 rt 1.6e-11 qr 5.7e-13
    3. fp32, 2000 x 25 at 14         no subject draw beyond 5e-4 in any model (largest 1.2e-4, a nu of latentqr); item draws 7.1e-7, structural block 3.7e-6, logLike 1.6e-8 at most
    4. 600 x 9 at 14, 2 / 3 shards   rtirt ra 1.5e-12 / 1.8e-12 rt 1.2e-12 / 1.0e-12 qr 1.7e-13 / 1.8e-13   latent ra 4.2e-13 / 5.2e-13 rt 7.0e-13 / 2.9e-13 qr 2.4e-14 / 2.3e-14
       (against the unsharded per-sweep device 2.6e-12 at most); DIC: Dhat against the oracle at the trace mean 1.4e-15 (fp64), 9.5e-10 (fp32);
       marginal l_i^(s) 7.6e-16, p_i 7.4e-14; predictive means 1.8e-14, no unit excluded by the margin rule
Every figure is at least a factor of forty inside 1e-8; the largest (2.5e-10, rt of latentqr at 6000 x 7) is the size of the twin's own largest (2.1e-10).
The new cases exposed no defect in the kernels.
Wall time of this file on an MI355X: 3.3 s for its 75 GPU cases (0.05 s the slowest, after 1 s of set-up); its 10 CPU cases take 2 s.

Sharded chains: test_gpu_sharded_regimes.py asserts no bit-for-bit identity between two or more shards and the unsharded engine (the shards' statistics
are summed in another association); its comparison with the unsharded ERM_FLAG_NO_PERSIST device is under the oracle's bound, and so is the one here."""
import functools

import numpy as np
import pytest

import marginal_util as mu
import parity_util as pu
import ppc_util as ppu
import shard_util as su
import test_gpu_dic as tdic
import test_gpu_marginal_waic as tmarg
import test_gpu_predictive as tpred
import test_gpu_wide_items as wi
from parity_util import exe  # noqa: F401  (the compiled planner checker, a fixture)
from test_gpu_wide_items import cu_count  # noqa: F401  (fixture)

gpu = pytest.mark.gpu

COV_MODELS = ["mlirt", "rtirt", "latent", "latentqr", "null"]
FMAX = 14                                       # PMAX - 2 (erm_layout.hpp)
WIDTHS = [1, 2, 7, 13, FMAX]
FLAG_NO_PERSIST = wi.FLAG_NO_PERSIST
LDS_LIMIT = 160 * 1024                          # erm_layout.hpp
TOL, FLOOR = 1e-8, 1e-6                         # the project's fp64 bound (tests/test_gpu_parity.py)
EDGE = dict(block_threads=256, grid_blocks=8)   # section 2's geometry
EDGE_N, EDGE_J = 6000, 7


def nv_of(model, F):
    """Values a subject parks in LDS (erm_layout.hpp, nv_of), over the covariates the kernels see."""
    return pu.kernel_feat(model, F) + (4 if model in ("latentqr", "latent") else 2)


@functools.lru_cache(maxsize=None)
def problem(model, N, J, F):
    return pu.make_problem(model, N, J, F)


@functools.lru_cache(maxsize=None)
def oracle_chain(model, N, J, F, T, intercept=False, sigp_mode=0):
    """The oracle's chain on problem(model, N, J, F): computed once per case and left unchanged."""
    Y, logT, X, init, _ = problem(model, N, J, F)
    op = pu.OracleProblem(model, Y, logT, X, init, qRt=0.85, intercept=intercept, cov2one=model not in ("latentqr", "latent"), sigp_mode=sigp_mode)
    return op.run(T, with_nu=model in pu.NU_MODELS)


def device(model, N, J, F, T, precision="f64", **opts):
    Y, logT, X, init, _ = problem(model, N, J, F)
    return pu.run_device(model, Y, logT, X, init, T, precision=precision, **opts)


def as_pair(model, dev, orc):
    """A device run and an oracle chain in the shape of pu.run_pair's result."""
    res = dict(orc=orc, dev=dev, model=model, dev_ra=dev["ra"][:, :, 0], dev_qr=dev["qr"][:, :, 0], dev_ll=dev["ll"][:, 0, 0])
    if model != "mlirt":
        res["dev_rt"] = dev["rt"][:, :, 0]
    return res


def check_oracle(label, res):
    parts = pu.rel_err_by_part(res, FLOOR)
    print(f"[{label}] largest error by trace part (error, sweep, column): {parts}; bound {TOL:g}")
    assert pu.max_rel_err(res, FLOOR) < TOL, (label, parts)


def free_running(exe, cu_count, model, N, J, F, T, *, intercept=False, also_per_sweep=True, **opts):
    """One fp64 case: the plan (printed), the engine runs it, every trace column of every sweep against the oracle; where the plan is persistent, the
    ERM_FLAG_NO_PERSIST engine must give the same traces bit for bit."""
    p = wi.planned(exe, cu_count, None, model, "f64", N, J, F=F, **opts)
    dev = device(model, N, J, F, T, intercept=intercept, **opts)
    tm = dev["engine"].timing()
    assert tm["cu_count"] == cu_count
    pu.assert_engine_runs_plan(tm, p)
    label = f"{model} f64 {N} x {J} F = {F}" + (" intercept" if intercept else "") + (f" {opts}" if opts else "")
    check_oracle(label, as_pair(model, dev, oracle_chain(model, N, J, F, T, intercept, opts.get("sigp_mode", 0))))
    dev["engine"].close()
    if p["persist"] and also_per_sweep:
        q = pu.engine_plan(exe, model, "f64", N, J, F, cu_count, flags=FLAG_NO_PERSIST, **opts)
        assert q["persist"] == 0 and {k: v for k, v in q.items() if k != "persist"} == {k: v for k, v in p.items() if k != "persist"}
        per = device(model, N, J, F, T, intercept=intercept, flags=FLAG_NO_PERSIST, **opts)
        pu.assert_engine_runs_plan(per["engine"].timing(), q)
        for k in ("ra", "rt", "qr", "ll", "item"):
            if k in per:
                assert np.array_equal(per[k], dev[k]), (label, "ERM_FLAG_NO_PERSIST", k)
        for k, v in dev["state"].items():
            assert v is None or np.array_equal(v, per["state"][k]), (label, "ERM_FLAG_NO_PERSIST state", k)
        per["engine"].close()
    return p


# ---------------------------------------------------------------------------------------------------------------
# 1. the width axis at a small shape
@gpu
@pytest.mark.parametrize("F", WIDTHS)
@pytest.mark.parametrize("model", COV_MODELS)
def test_f64_width_axis(exe, cu_count, model, F):
    p = free_running(exe, cu_count, model, 300, 9, F, 6)
    assert p["persist"] == 1 and p["fused"] == 1, p


@gpu
@pytest.mark.parametrize("model", ["rtirt", "latent"])
def test_f64_intercept_at_the_limit(exe, cu_count, model):
    """intercept = True: slot 0 and (GibbsRtIrt) slot p of beta are drawn, so every one of the 2p = 30 / q = 16 columns of the structural step is live."""
    p = free_running(exe, cu_count, model, 300, 9, FMAX, 6, intercept=True)
    assert p["persist"] == 1
    orc = oracle_chain(model, 300, 9, FMAX, 6, True, 0)
    slots = [0, FMAX + 1] if model == "rtirt" else [0]
    assert np.all(orc["qr"][:, slots] != 0.0) and np.all(oracle_chain(model, 300, 9, FMAX, 6)["qr"][:, slots] == 0.0)      # what the setting is there for


@gpu
@pytest.mark.parametrize("F", [13, FMAX])
def test_f64_latentqr_weighted_gram_triangle(exe, cu_count, F):
    """sigp_mode = 1: q (q + 1) / 2 = 120 and 136 weighted Gram entries, NG = 2p + 8 + 153 global statistics at the limit."""
    assert pu.extra_stats("latentqr", FMAX, 1) == 153
    p = free_running(exe, cu_count, "latentqr", 300, 9, F, 6, sigp_mode=1)
    assert p["persist"] == 1
    a, b = oracle_chain("latentqr", 300, 9, F, 6, False, 1), oracle_chain("latentqr", 300, 9, F, 6)
    assert not np.allclose(a["qr"][:, F + 2 + 3], b["qr"][:, F + 2 + 3])          # Sigp[2,2] differs between the modes


@gpu
@pytest.mark.parametrize("model", ["rtirt", "latent", "latentqr"])
def test_f64_one_wave_at_the_limit(exe, cu_count, model):
    """block_threads = 64: one wave does the 30 x 30 chain (the 16-column inverse) and every row."""
    p = free_running(exe, cu_count, model, 300, 9, FMAX, 6, block_threads=64)
    assert p["block_threads"] == 64 and p["fused"] == 1


# ---------------------------------------------------------------------------------------------------------------
# 2. each edge where n_feat alone changes the plan
def plan_edge(exe, cu_count, model, sigp_mode=0):
    """(last n_feat whose plan is fused and persistent, the plans by n_feat) at section 2's shape."""
    plans = [pu.engine_plan(exe, model, "f64", EDGE_N, EDGE_J, F, cu_count, sigp_mode=sigp_mode, **EDGE) for F in range(FMAX + 1)]
    on = [F for F, p in enumerate(plans) if p["fused"] and p["persist"]]
    assert on and on == list(range(len(on))) and len(on) <= FMAX, f"{model}: no edge below {FMAX} at this shape: fused and persistent at n_feat {on}"
    return on[-1], plans


EDGE_CASES = [("mlirt", 0), ("rtirt", 0), ("latent", 0), ("latentqr", 0), ("latentqr", 1)]


@gpu
@pytest.mark.parametrize("side", ["fused", "two_kernel"])
@pytest.mark.parametrize("model,sigp_mode", EDGE_CASES)
def test_f64_both_sides_of_the_plan_edge(exe, cu_count, model, sigp_mode, side):
    """The fused side holds rows_per_block * nv_of * 8 bytes of parked subject values and ends within the last 16 KB of the LDS limit -- one more covariate
    (rows_per_block * 8 bytes more) no longer fits, which is why the next n_feat is planned as two kernels per sweep.  Properties of the plan: another
    compute-unit count passes, a planner change that moves the edge fails here."""
    last, plans = plan_edge(exe, cu_count, model, sigp_mode)
    F = last if side == "fused" else last + 1
    p = plans[F]
    sub = p["rows_per_block"] * nv_of(model, F) * 8
    print(f"\n[{model} sigp_mode {sigp_mode}] last fused and persistent n_feat {last}; parked subject values {sub} bytes of {p['lds_fused'] or p['lds0']} + {p['lds_static']}")
    if side == "fused":
        total = p["lds_fused"] + p["lds_static"]
        assert LDS_LIMIT - 16 * 1024 < total <= LDS_LIMIT and total + p["rows_per_block"] * 8 > LDS_LIMIT, p
        assert sub < p["lds_fused"]
    else:
        assert p["fused"] == 0 and p["persist"] == 0 and p["lds0"] + p["lds_static"] <= LDS_LIMIT, p
    opts = dict(EDGE, sigp_mode=1) if sigp_mode else dict(EDGE)
    q = free_running(exe, cu_count, model, EDGE_N, EDGE_J, F, 4, also_per_sweep=False, **opts)
    assert q == p


@gpu
def test_refused_plan_fails_in_create_and_the_device_runs_on(exe, cu_count):
    """grid_blocks = 6 at n_feat = 14: 1000 subjects per workgroup park 16 values each; the planner has no layout, erm_create returns its message and
    nothing is launched.  n_feat = 3 at the same geometry is planned, and runs to the oracle's chain afterwards."""
    L = pu.ge.load_package()._lib
    opts = dict(block_threads=256, grid_blocks=6)
    msg = "LDS footprint too large; lower block_threads or raise grid_blocks"
    assert pu.engine_plan(exe, "rtirt", "f64", EDGE_N, EDGE_J, FMAX, cu_count, refusal=True, **opts) == {"error": msg}
    with pytest.raises(L.ErmError, match=msg):
        L.Engine(model=pu.MODELS["rtirt"], n_item=EDGE_J, n_subj=EDGE_N, n_feat=FMAX, n_iter=4, n_chain=1, n_burnin=2, cov2one=1, q_rt=0.85, seed=1234,
                 precision=1, trace_mode=1, **opts)
    free_running(exe, cu_count, "rtirt", EDGE_N, EDGE_J, 3, 4, also_per_sweep=False, **opts)


# ---------------------------------------------------------------------------------------------------------------
# 3. fp32 at the limit
@gpu
@pytest.mark.parametrize("model", COV_MODELS)
def test_f32_one_sweep_at_the_limit(exe, cu_count, model):
    """test_f32_one_sweep's rule at n_feat = 14: subject draws (nu among them) within 5e-4 but for a share of 2e-3 of the subjects, item draws and the
    structural block within 2e-3 absolute (|d - o| / max(|o|, 1)), the log-likelihood within 1e-4 relative."""
    N, J, F = 2000, 25, FMAX
    p = wi.planned(exe, cu_count, None, model, "f32", N, J, F=F)
    dev = device(model, N, J, F, 1, precision="f32")
    pu.assert_engine_runs_plan(dev["engine"].timing(), p)
    res = as_pair(model, dev, oracle_chain(model, N, J, F, 1))
    d = pu.decode_rows(model, N, J, F, res["dev_ra"], res.get("dev_rt"), res["dev_qr"])
    o = pu.decode_rows(model, N, J, F, res["orc"]["ra"], res["orc"]["rt"] if model != "mlirt" else None, res["orc"]["qr"])
    items = {k: float(wi._abs_err(d[k][0], o[k][0]).max()) for k in ("a", "b", "lambda_", "sig2t") if k in d}
    struct = {k: float(wi._abs_err(d[k][0], o[k][0]).max()) for k in ("beta", "sigp") if k in d and d[k].shape[1]}
    subj = {k: wi._abs_err(d[k][0], o[k][0]) for k in ("theta", "zeta", "nu") if k in d}
    shares = {k: float(np.mean(e > 5e-4)) for k, e in subj.items()}
    ll = abs(res["dev_ll"][0] - res["orc"]["ll"][0]) / abs(res["orc"]["ll"][0])
    print(f"[{model} f32 {N} x {J} F = {F}] share of subject draws beyond 5e-4: {shares} (cap 2e-3; largest {({k: float(e.max()) for k, e in subj.items()})}); "
          f"item draws {items}; structural {struct}; logLike {ll:.3g}")
    assert max(shares.values()) < 2e-3, shares
    assert max(items.values()) < 2e-3, items
    assert max(struct.values()) < 2e-3, struct
    assert ll < 1e-4, ll
    dev["engine"].close()


# ---------------------------------------------------------------------------------------------------------------
# 4. what runs behind the sweep
@gpu
@pytest.mark.parametrize("precision", ["f64", "f32"])
@pytest.mark.parametrize("model", ["rtirt", "latent", "latentqr"])
def test_dic_at_the_limit(model, precision):
    tdic.check_device_dic(model, precision, nFeat=FMAX)


@gpu
@pytest.mark.parametrize("model", ["rtirt", "latent"])
def test_marginal_loglik_equals_twin_at_the_limit(model):
    """n_feat = MARG_MAXF: the kernel's x[MARG_MAXF] and both x'beta loops run full length."""
    rows = mu.make_rows(model, 9, FMAX, 3, seed=11)
    Y, logT, X = mu.make_data(model, 600, 9, FMAX, seed=11)
    tmarg._assert_equals_twin(model, Y, logT, X, rows, 61, what=f"{model} F = {FMAX}")


@gpu
def test_marginal_loglik_refuses_fifteen_covariates():
    L = pu.ge.load_package()._lib
    rows = mu.make_rows("rtirt", 9, FMAX + 1, 3, seed=11)
    Y, logT, X = mu.make_data("rtirt", 37, 9, FMAX + 1, seed=11)
    with pytest.raises(L.ErmError, match=r"n_feat \(0 \.\. 14\) out of range"):
        L.marginal_loglik(mu.CODE["rtirt"], Y, logT, X, rows)
    ok = L.marginal_loglik(mu.CODE["rtirt"], Y, logT, X[:, :FMAX], mu.make_rows("rtirt", 9, FMAX, 3, seed=11))       # and the device runs on
    assert np.all(np.isfinite(ok["l"]))


@gpu
@pytest.mark.parametrize("model", ["rtirt", "latentqr"])
def test_predictive_accumulators_equal_the_host_twin_at_the_limit(model):
    """test_device_accumulators_equal_the_host_twin's comparison (1001 x 17, three interleaved pseudo-chains, nine post-burn-in rows, thin 1) at n_feat = 14."""
    Y, logT, X, init, _ = problem(model, 1001, 17, FMAX)
    eng = tpred._engine(model, Y, logT, X, init, n_iter=6, n_chain=3, n_burnin=3, precision="f64", ppc=1)
    eng.run(18)
    assert eng.post_count == 9 and eng.predictive_reps == 9
    host, _ = tpred._twin(eng, model, n_iter=6, n_chain=3, n_burnin=3, thin=1)
    dev = tpred._device(eng, 1)
    ppu.assert_equals_twin(dev, host, what=f"{model} f64 1001x17 F = {FMAX}")
    ppu.check_counts(dev)
    eng.close()


@gpu
@pytest.mark.parametrize("count", [2, 3])
@pytest.mark.parametrize("model", ["rtirt", "latent"])
def test_sharded_chain_at_the_limit(model, count):
    """The statistics row the shards exchange carries the PMAX x PMAX block, all of it live at p = 15.  Callback exchange, all shards in this process; the
    shards are closed before the unsharded engine is opened (never more than three engines at once)."""
    N, J, T = 600, 9, 4
    res = su.sharded(model, N, J, T, count, F=FMAX)
    assert all(e.timing()["persistent"] == 0 for e in res["engines"])
    for e in res["engines"]:
        e.close()
    res["orc"] = oracle_chain(model, N, J, FMAX, T)                                 # (su.sharded ran the oracle on the same make_problem inputs)
    check_oracle(f"{model} f64 {N} x {J} F = {FMAX}, {count} shards", res)
    whole = device(model, N, J, FMAX, T, flags=FLAG_NO_PERSIST)
    w = as_pair(model, whole, None)
    check_oracle(f"{model} f64 {N} x {J} F = {FMAX}, {count} shards vs the unsharded per-sweep device", dict(res, orc={k[4:]: v for k, v in w.items() if k.startswith("dev_")}))
    whole["engine"].close()


@gpu
def test_farm_chains_equal_single_engines_at_the_limit():
    """Two chains on device 0: chain l in slab l, bit for bit the single engine with the same seed and chain id (test_farm_equals_separate_engines)."""
    L = pu.ge.load_package()._lib
    model, N, J, T, nch = "rtirt", 600, 8, 12, 2
    Y, logT, X, init, _ = problem(model, N, J, FMAX)
    g = np.random.default_rng(5)
    inits = [dict(init, theta=g.standard_normal(N)) for _ in range(nch)]
    farm = L.Farm([0] * nch, model=pu.MODELS[model], n_item=J, n_subj=N, n_feat=FMAX, n_iter=T, n_chain=1, n_burnin=T // 2, cov2one=1, q_rt=0.85, seed=1234,
                  precision=1, trace_mode=1)
    farm.set_data(Y, logT, X)
    for l in range(nch):
        farm.set_state(l, **su.engine_state(inits[l]))
    farm.run(T)
    which = (L.TRACE_RA, L.TRACE_RT, L.TRACE_QR, L.TRACE_LOGLIKE)
    ft = {w: farm.trace(w) for w in which}
    states = [farm.get_state(l) for l in range(nch)]
    farm.close()
    for l in range(nch):
        e = L.Engine(model=pu.MODELS[model], n_item=J, n_subj=N, n_feat=FMAX, n_iter=T, n_chain=1, n_burnin=T // 2, cov2one=1, q_rt=0.85, seed=1234, chain_id=l,
                     precision=1, trace_mode=1)
        e.set_data(Y, logT, X)
        e.set_state(**su.engine_state(inits[l]))
        e.run(T)
        for w in which:
            assert ft[w].shape[2] == nch and np.array_equal(ft[w][:, :, l], e.trace(w)[:, :, 0]), (w, l)
        st = e.get_state()
        for k, v in st.items():
            assert v is None or np.array_equal(v, states[l][k]), (k, l)
        e.close()
    assert not np.array_equal(ft[L.TRACE_QR][:, :, 0], ft[L.TRACE_QR][:, :, 1])


@gpu
@pytest.mark.parametrize("name,truth,gen", [("GibbsMlIrt", "setTrueParaMlIrt", 0), ("GibbsRtIrt", "setTrueParaRtIrt", 1), ("GibbsRtIrtLatent", "setTrueParaRtIrtLatent", 4)])
def test_device_generator_equals_the_oracle_at_the_limit(name, truth, gen):
    """test_device_generators_equal_the_oracle_restatement_value_by_value's comparison with nFeat = 14 covariates drawn per subject (the generators that draw any)."""
    pkg = pu.ge.load_package()
    N, J, F = 1000, 9, FMAX
    C = pkg.setCond(nSubj=N, nItem=J, nFeat=F, nIter=4, nChain=1, qRt=0.5)
    tp = getattr(pkg, truth)(C, seed=11)
    if gen == 1:
        tp.Sigp = np.array([[1.3, 0.4], [0.4, 0.8]])
    M = getattr(pkg, name)(C, precision="f64")
    pkg.simulateData(M, tp, type="norm", seed=2024)
    o = pu.orc_simulate(gen, N, J, F, a=tp.a, b=tp.b, lam=tp.lam if gen else None, sig2t=(tp.sig2t if np.size(tp.sig2t) else np.ones(J)) if gen else None,
                        Sigp=np.asarray(tp.Sigp).reshape(-1, order="F") if np.size(tp.Sigp) else None, beta=np.asarray(tp.beta).reshape(-1, order="F"), seed=2024)
    assert np.array_equal(np.asarray(M.Data.Y, dtype=np.uint8), o["Y"])
    assert np.asarray(M.Data.X).shape == (N, F) and np.max(np.abs(np.asarray(M.Data.X) - o["X"])) < 1e-12
    assert np.max(np.abs(tp.theta - o["theta"])) < 1e-12
    if gen:
        assert np.max(np.abs(tp.zeta - o["zeta"])) < 1e-12 and np.max(np.abs(np.asarray(M.Data.logT) - o["logT"])) < 1e-12
    M.close()


_RN, _RJ = 40, 3          # (x'x of [1 X] needs more subjects than its 15 columns)


def _readout_engine(model, precision, intercept):
    L = pu.ge.load_package()._lib
    g = np.random.default_rng(3)
    Y, logT, X = g.random((_RN, _RJ)) < 0.5, g.normal(1.0, 0.3, (_RN, _RJ)), g.standard_normal((_RN, FMAX))
    eng = L.Engine(model=pu.MODELS[model], n_item=_RJ, n_subj=_RN, n_feat=FMAX, n_iter=4, n_chain=1, n_burnin=1, intercept=int(intercept), cov2one=int(model != "latent"),
                   q_rt=0.85, seed=11, precision={"f32": 0, "f64": 1}[precision], trace_mode=1)
    eng.set_data(Y, logT, X)
    return eng


@gpu
@pytest.mark.parametrize("intercept", [False, True])
@pytest.mark.parametrize("precision", ["f64", "f32"])
@pytest.mark.parametrize("model", ["rtirt", "latent"])
def test_every_beta_slot_holds_what_its_position_names(model, precision, intercept):
    """test_every_trace_column_holds_what_its_name_says' construction at F = 14 (N = 40, J = 3, nIter = 4, one erm_run per row).  An item-trace row is
    [a 0:3 | b 3:6 | lambda 6:9 | sig2t 9:12 | the kernels' small part of qr 12:]; Post.qr is vec(beta) (2p = 30: column theta, then column zeta, the first ending
    one slot before the second begins in the device's PMAX-strided copy) and vec(Sigp) for GibbsRtIrt, beta (q = 16: intercept, 14 covariates, theta) and vec(Sigp)
    for GibbsRtIrtLatent.  Row r equals the item trace's columns and what erm_get_state returns after that run, all exactly; the intercept slots (0, and p for
    GibbsRtIrt) are zero exactly when intercept is off and every other slot is a draw different from all others; Post.mean's beta is the mean of rows 1 .. 3;
    and a state with distinct values in every entry survives erm_set_state / erm_get_state exactly."""
    L = pu.ge.load_package()._lib
    N, J, p = _RN, _RJ, FMAX + 1
    nb = 2 * p if model == "rtirt" else p + 1
    f32 = (lambda v: v.astype(np.float32).astype(np.float64)) if precision == "f32" else (lambda v: v)
    eng = _readout_engine(model, precision, intercept)
    st = dict(theta=0.1 + 0.01 * np.arange(N), a=1.0 + 0.1 * np.arange(J), b=-0.5 + 0.1 * np.arange(J), sigp=np.array([1.5, 0.25, 0.375, 2.0]), zeta=-0.3 + 0.02 * np.arange(N),
              lambda_=2.0 + 0.1 * np.arange(J), sig2t=0.5 + 0.1 * np.arange(J), beta=0.7 + 0.03 * np.arange(nb))
    eng.set_state(**st)
    back = eng.get_state()
    for k, v in st.items():
        assert back[k].shape == v.shape and np.array_equal(back[k], f32(v) if k in ("theta", "zeta") else v), (k, back[k], v)
    eng.set_state(theta=st["theta"], zeta=st["zeta"], a=np.ones(J), b=np.zeros(J), lambda_=np.ones(J), sig2t=np.ones(J), sigp=np.array([1.0, 0.0, 0.0, 1.0]), beta=np.zeros(nb))
    beta, sigp = [], []
    for _ in range(4):
        eng.run(1)
        s = eng.get_state(which=("beta", "sigp"))
        beta.append(s["beta"])
        sigp.append(s["sigp"])
    beta, sigp = np.array(beta), np.array(sigp)
    item = eng.item_trace()
    qr = eng.trace(L.TRACE_QR)[:, :, 0]
    assert item.shape == (4, 4 * J + nb + 4) and qr.shape == (4, nb + 4) and np.all(np.isfinite(item))
    assert np.array_equal(qr, item[:, 4 * J:])
    assert np.array_equal(qr[:, :nb], beta) and np.array_equal(qr[:, nb:], sigp)
    zero = np.zeros(nb, dtype=bool)
    if not intercept:
        zero[[0, p] if model == "rtirt" else [0]] = True
    assert np.all(qr[:, :nb][:, zero] == 0.0) and np.all(qr[:, :nb][:, ~zero] != 0.0)
    assert all(len(set(row[~zero])) == nb - zero.sum() for row in qr[:, :nb])
    m = eng.get_mean()
    assert m["beta"].shape == (nb,) and np.allclose(m["beta"], qr[1:, :nb].mean(axis=0), rtol=1e-12, atol=0)
    eng.close()


# ---------------------------------------------------------------------------------------------------------------
# 5. the planner on the CPU
@pytest.mark.parametrize("precision", ["f64", "f32"])
@pytest.mark.parametrize("model", COV_MODELS)
def test_plan_loses_fused_and_persist_once_in_n_feat(exe, model, precision):
    """Section 2's shapes (6000 x 7, 256 threads, 8 and 6 workgroups; 256 compute units) and section 1's (300 x 9, automatic), n_feat from 0 to 14 and, for
    LatentQr, both sigp_mode: fused and persist are non-increasing in n_feat, a refusal is not followed by a plan, and 15 covariates are refused by name.  (The
    kernels of GibbsRtIrtNull see no covariate: its plan does not depend on n_feat, and the planner's refusal is asked for with Fk = 15 directly.)"""
    for N, J, opts in ((EDGE_N, EDGE_J, EDGE), (EDGE_N, EDGE_J, dict(block_threads=256, grid_blocks=6)), (300, 9, {})):
        for sigp_mode in ((0, 1) if model == "latentqr" else (0,)):
            plans = [pu.engine_plan(exe, model, precision, N, J, F, 256, sigp_mode=sigp_mode, refusal=True, **opts) for F in range(FMAX + 1)]
            level = [(-1, -1) if "error" in p else (p["fused"], p["persist"]) for p in plans]
            for F in range(1, FMAX + 1):
                assert level[F][0] <= level[F - 1][0] and level[F][1] <= level[F - 1][1], (model, precision, N, J, opts, sigp_mode, F, level)
            assert "error" not in plans[3], plans[3]
            if model == "null":
                assert all(p == plans[0] for p in plans)
    if precision == "f64" and model != "null":
        assert plan_edge(exe, 256, model)[0] == {"mlirt": 13, "rtirt": 13, "latent": 11, "latentqr": 11}[model]
        assert "LDS footprint too large" in pu.engine_plan(exe, model, "f64", EDGE_N, EDGE_J, FMAX, 256, refusal=True, block_threads=256, grid_blocks=6)["error"]
    if model == "latentqr" and precision == "f64":
        assert plan_edge(exe, 256, model, 1)[0] == 10
    r = pu.plan(exe, pu.MODELS[model], int(precision == "f64"), EDGE_N, EDGE_J, FMAX + 1, bt=256, gb=8)
    assert r == {"error": "n_feat too large (max 14)"}, r

"""Sweep parity at wide item counts (26 <= nItem <= 896): every model, both precisions, in every regime the automatic launch geometry moves through.

Between the reference's own test lengths and the item limit the sweep kernel is several different kernels: the item arrays' LDS stride is a
compile-time 128 up to 128 items and the item count beyond; the planner halves the workgroup so that the per-wave item accumulators fit in LDS
(1024 -> ... -> 64 threads, 768 -> 384 -> 192 for fp64 LatentQr); a one-wave workgroup runs the tiny step and every row of the fused sweep itself; the
sweep leaves the fused schedule when the tiny step's scratch no longer fits; the fp32 engine gives every subject a 64-thread workgroup of its own; and
1024 x 128 is the last size of the persistent schedule.  Every case here

  1. asks the CPU planner (tests/geometry_check.cpp over erm_geometry.hpp) for the plan of its (model, precision, N, J, F, compute units), asserts
     that the plan is in the regime the case is named for -- as a property of the plan, so another CU count passes and a shape that drifts out of
     its regime fails --, and that erm_get_timing reports exactly that plan and schedule;
  2. compares the device with the fp64 CPU oracle on the same seeded inputs.

Bounds (the project's two, tests/test_gpu_parity.py): fp64, every trace column of every free-running sweep within 1e-8 relative (floor 1e-6) up to
400 items and within 1e-7 (floor 1e-5: test_f64_limits_of_the_engine's bound at 896 items) beyond; every model free-runs 4 sweeps, GibbsRtIrtCrossQr
(its chain is chaotic: tests/test_oracle_sweeps.py) 3 under the 1e-7 bound and 2 under the 1e-8 bound -- see crossqr_sweeps -- with its later sweeps
checked teacher-forced at every shape of up to 400 items.  fp32, one sweep from the oracle's state: item draws and the structural block within 2e-3
absolute (|d - o| / max(|o|, 1)), the log-likelihood within 1e-4 relative, subject draws within 5e-4 except for a share of at most 8e-5 * nItem of the
subjects -- test_f32_one_sweep's rule (one flipped Polya-Gamma decision per 5e4 cells, a factor of four of headroom: 2e-3 at its 25 items) written
out for a subject that owns nItem cells.  The quantile weights nu (per subject / per cell) are drawn from the subject draws and fall under the
subject rule.  Every case prints its plan, its largest error by trace part and, in fp32, its out-of-tolerance shares (pytest -s)."""
import functools

import numpy as np
import pytest

import parity_util as pu
from parity_util import exe  # noqa: F401  (the compiled planner checker, a fixture)

pytestmark = pytest.mark.gpu

MODELS = ["mlirt", "rtirt", "latentqr", "crossqr", "null", "cross", "latent"]
SINGLE_PASS = [m for m in MODELS if m not in pu.CQ_MODELS]
F = 3
FLAG_NO_FUSE, FLAG_NO_PERSIST = 1, 8             # include/ertirt.h
OMP_CELLS = 1_000_000                            # sweeps of more cells than this run the oracle in its 16-thread mode


def max_threads(model, precision):
    """The kernels' launch bounds (erm_layout.hpp, max_block_threads)."""
    return 768 if (model == "latentqr" and precision == "f64") else 1024


# ---------------------------------------------------------------------------------------------------------------
# Regimes: name -> properties of a plan, each a (description, holds) pair.  `fused` is the plan's flag; the two-pass Cross family never fuses.
def _regime(name, p, model, precision, N, J):
    waves = p["block_threads"] // 64
    single = model not in pu.CQ_MODELS
    fused_if_single = ("fused exactly for the single-pass models", p["fused"] == int(single))
    per_sweep = ("per-sweep schedule", p["persist"] == 0)
    if name == "stride_const":          # the row-sum loop's immediate-offset form
        return [("J <= ITEM_STRIDE", J <= pu.ITEM_STRIDE), ("several waves", waves >= 2), fused_if_single, per_sweep]
    if name == "stride_runtime":        # one item past the switch: same workgroups, the stride a variable
        return [("J > ITEM_STRIDE", J > pu.ITEM_STRIDE), ("several waves", waves >= 2), fused_if_single, per_sweep]
    if name == "shrunk":                # fewer threads than the launch bound, still several waves
        props = [("J > ITEM_STRIDE", J > pu.ITEM_STRIDE), ("fewer threads than the launch bound", p["block_threads"] < max_threads(model, precision)),
                 ("several waves", waves >= 2), fused_if_single, per_sweep]
        if model == "latentqr" and precision == "f64":
            props.append(("a 384- or 192-thread workgroup (halved from 768)", p["block_threads"] in (384, 192)))
        return props
    if name == "shrunk_to_the_end":     # the halving has (all but) run out: one wave, two for MlIrt's four statistics
        return [("at most two waves", waves <= 2), ("one wave unless MlIrt", waves == 1 or model == "mlirt"), fused_if_single, per_sweep,
                ("several subjects per workgroup", p["rows_per_block"] > 1)]
    if name == "one_wave_fused_odd":    # the wave that runs the tiny step also owns every row; odd J: the scalar row-sum loop past the stride switch
        return [("one wave", waves == 1), ("odd J > ITEM_STRIDE", J % 2 == 1 and J > pu.ITEM_STRIDE), fused_if_single, per_sweep,
                ("several subjects per workgroup", p["rows_per_block"] > 1)]
    if name == "two_kernel_by_lds":     # the tiny step's scratch no longer fits beside the pass layout
        return [("one wave", waves == 1), ("not fused", p["fused"] == 0), ("below the item limit", J < 896), per_sweep]
    if name == "item_limit":
        return [("J == 896", J == 896), ("one wave", waves == 1), ("not fused", p["fused"] == 0), per_sweep]
    if name == "wave1_owns_all_rows":   # fused, two waves: wave 0 runs the tiny step, wave 1's slice holds the whole workgroup
        return [("two waves", waves == 2), ("fused", p["fused"] == 1), ("wave 1's slice holds every row", p["rows_per_wave"] >= p["rows_per_block"]),
                ("more than a hundred rows per workgroup", p["rows_per_block"] > 100), per_sweep]
    if name == "persistent":
        return [("persistent", p["persist"] == 1), ("fused", p["fused"] == 1), ("J <= ITEM_STRIDE", J <= pu.ITEM_STRIDE), ("one round", p["rounds"] == 1)]
    if name == "just_not_persistent":
        return [per_sweep, ("fused", p["fused"] == 1), ("several waves", waves >= 2),
                ("one subject or one item beyond the persistent sizes", J - 1 <= pu.ITEM_STRIDE and min((N - 1) * J, N * (J - 1)) <= 2 ** 17 < N * J or J == pu.ITEM_STRIDE + 1)]
    # ---- fp32 (one workgroup per subject needs N resident 64-thread workgroups, 16 per compute unit: 125 compute units at these N = 2 000)
    if name == "f32_one_subject_fused":         # grid_blocks = N; MlIrt's four statistics still leave it two subjects per workgroup at 512 items
        one = [("one subject per 64-thread workgroup", p["rows_per_block"] == 1 and waves == 1 and p["grid_blocks"] == N)]
        if model == "mlirt" and J <= 512:
            one = [("two waves, two subjects", waves == 2 and p["rows_per_block"] == 2)]
        return one + [fused_if_single, per_sweep]
    if name == "f32_one_subject_fuse_edge":     # 700 items: only MlIrt's scratch still fits
        return [("one subject per 64-thread workgroup", p["rows_per_block"] == 1 and waves == 1 and p["grid_blocks"] == N),
                ("fused only for MlIrt", p["fused"] == int(model == "mlirt")), per_sweep]
    if name == "f32_one_subject_two_kernel":
        return [("one subject per 64-thread workgroup", p["rows_per_block"] == 1 and waves == 1 and p["grid_blocks"] == N), ("not fused", p["fused"] == 0), per_sweep]
    raise KeyError(name)


def planned(exe, cu_count, regime, model, precision, N, J, F=F, **overrides):
    """The CPU planner's plan for the case, checked against the case's regime and printed."""
    p = pu.engine_plan(exe, model, precision, N, J, F, cu_count, **overrides)
    print(f"\n[{model} {precision} {N} x {J}{'' if F == 3 else f' F = {F}'} {overrides or ''}] regime {regime or '-'}; plan {p}")
    if regime:
        bad = [what for what, ok in _regime(regime, p, model, precision, N, J) if not ok]
        assert not bad, f"{model} {precision} {N} x {J} is not in regime '{regime}': {bad}; plan {p}"
    return p


@pytest.fixture(scope="module")
def cu_count():
    """Compute units of the card, as the engine counts them (erm_get_timing)."""
    L = pu.ge.load_package()._lib
    eng = L.Engine(model=1, n_item=5, n_subj=30, n_feat=0, n_iter=1, n_chain=1, n_burnin=0, cov2one=1, q_rt=0.85, seed=1, precision=1, trace_mode=0)
    cu = eng.timing()["cu_count"]
    eng.close()
    assert cu >= 1
    return cu


@functools.lru_cache(maxsize=2)
def problem(model, N, J, F=F):
    return pu.make_problem(model, N, J, F)


def bound(J):
    """(relative bound, absolute floor) of the fp64 comparisons."""
    return (1e-8, 1e-6) if J <= 400 else (1e-7, 1e-5)


def crossqr_sweeps(J):
    """Free-running sweeps of GibbsRtIrtCrossQr.  The issue of chaos is the REFERENCE's: the oracle against its own twin started 1 ulp apart (theta or
    zeta moved by nextafter, the method of test_crossqr_chain_is_chaotic), largest relative difference over ra, rt and qr with this file's floors, by sweep:
        3000 x 127  4e-11  1e-10  1.5e-8      3000 x 200  5e-11  2e-10  1.4e-8      2000 x 513  7e-12  3e-11  2e-9
        3000 x 128  3e-12  2e-9   4e-9        2000 x 300  7e-11  7e-11  1.1e-8      700 x 641   7e-11  3e-11  1e-9
        3000 x 129  2e-11  3e-10  2e-9        2000 x 400  7e-11  1e-10  3.2e-8      500 x 896   3e-12  4e-11  1e-9
    At these sizes the third sweep is not determined to 1e-8 by the reference itself (the device differs from the oracle by summation order, a perturbation of
    the same kind: its third sweep of 3 000 x 200 came to 1.07e-8, in one nu_ij), while it stays a factor of forty inside 1e-7.  So CrossQr free-runs
    three sweeps where the bound is 1e-7 and two where it is 1e-8; there its later sweeps are checked teacher-forced (test_f64_wide_teacher_forced)."""
    return 2 if J <= 400 else 3


def device_and_oracle(model, N, J, nsweeps, precision, **opts):
    """pu.run_pair on the cached problem (the oracle in its 16-thread mode for large sweeps)."""
    Y, logT, X, init, _ = problem(model, N, J)
    dev = pu.run_device(model, Y, logT, X, init, nsweeps, precision=precision, **opts)
    with pu.oracle_threads(16 if N * J > OMP_CELLS else 1):
        op = pu.OracleProblem(model, Y, logT, X, init, qRt=0.85, cov2one=model not in ("latentqr", "latent"))
        orc = op.run(nsweeps, with_nu=model in pu.NU_MODELS)
    res = dict(orc=orc, dev=dev, model=model, dev_ra=dev["ra"][:, :, 0], dev_qr=dev["qr"][:, :, 0], dev_ll=dev["ll"][:, 0, 0])
    if model != "mlirt":
        res["dev_rt"] = dev["rt"][:, :, 0]
    return res


def free_running(exe, cu_count, regime, model, N, J, **opts):
    """One fp64 case: regime, plan == engine, then every trace column of every free-running sweep against the oracle."""
    p = planned(exe, cu_count, regime, model, "f64", N, J, **opts)
    res = device_and_oracle(model, N, J, crossqr_sweeps(J) if model == "crossqr" else 4, "f64", **opts)
    tm = res["dev"]["engine"].timing()
    assert tm["cu_count"] == cu_count
    pu.assert_engine_runs_plan(tm, p)
    tol, floor = bound(J)
    parts = pu.rel_err_by_part(res, floor)
    print(f"[{model} f64 {N} x {J}] largest error by trace part (error, sweep, column): {parts}; bound {tol:g}")
    assert pu.max_rel_err(res, floor) < tol, parts
    return res


# ---------------------------------------------------------------------------------------------------------------
# fp64, every model
F64_CASES = [("stride_const", 3000, 127), ("stride_const", 3000, 128), ("stride_runtime", 3000, 129),
             ("shrunk", 3000, 200), ("shrunk", 2000, 300), ("shrunk_to_the_end", 2000, 400),
             ("one_wave_fused_odd", 2000, 513), ("two_kernel_by_lds", 700, 641), ("item_limit", 500, 896)]


@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("regime,N,J", F64_CASES)
def test_f64_wide_free_running(exe, cu_count, regime, N, J, model):
    free_running(exe, cu_count, regime, model, N, J)


@pytest.mark.parametrize("model", ["rtirt", "latent"])
def test_f64_wave_one_owns_every_row(exe, cu_count, model):
    """40 000 x 300: a fused two-wave workgroup of ~157 subjects -- wave 0 runs the tiny step, wave 1's LDS slice holds all of them."""
    free_running(exe, cu_count, "wave1_owns_all_rows", model, 40_000, 300)


@pytest.mark.parametrize("model", SINGLE_PASS)
@pytest.mark.parametrize("regime,N,J", [("persistent", 1024, 128), ("persistent", 900, 127), ("just_not_persistent", 1025, 128), ("just_not_persistent", 1000, 129)])
def test_f64_persistent_edge(exe, cu_count, regime, N, J, model):
    """2^17 cells of 128 items is the last persistent size; one subject or one item more takes the per-sweep schedule.  The persistent chain is also the
    ERM_FLAG_NO_PERSIST chain at the same geometry, bit for bit."""
    res = free_running(exe, cu_count, regime, model, N, J)
    if regime != "persistent":
        return
    p = planned(exe, cu_count, None, model, "f64", N, J, flags=FLAG_NO_PERSIST)
    Y, logT, X, init, _ = problem(model, N, J)
    per = pu.run_device(model, Y, logT, X, init, 4, precision="f64", flags=FLAG_NO_PERSIST)
    pu.assert_engine_runs_plan(per["engine"].timing(), p)
    q = pu.engine_plan(exe, model, "f64", N, J, F, cu_count)
    assert p["persist"] == 0 and {k: v for k, v in p.items() if k != "persist"} == {k: v for k, v in q.items() if k != "persist"}       # the flag changes the schedule only
    for k in ("ra", "rt", "qr", "ll", "item"):
        if k in per:
            assert np.array_equal(per[k], res["dev"][k]), k


@pytest.mark.parametrize("opts", [dict(lanes_per_row=1), dict(lanes_per_row=64), dict(flags=FLAG_NO_FUSE)], ids=["W1", "W64", "nofuse"])
@pytest.mark.parametrize("model", MODELS)
def test_f64_overrides_at_300_items(exe, cu_count, opts, model):
    """2 000 x 300 with 300 and 5 items per lane in the row-sum phase, and on the two-kernel schedule: the same bound against the oracle."""
    p = planned(exe, cu_count, None, model, "f64", 2000, 300, **opts)
    if "lanes_per_row" in opts:
        assert p["W"] == opts["lanes_per_row"] and p["fused"] == int(model not in pu.CQ_MODELS)
    else:
        assert p["fused"] == 0 and p["persist"] == 0
    free_running(exe, cu_count, None, model, 2000, 300, **opts)


TF_CASES = [(r, N, J, m) for r, N, J in [("shrunk_to_the_end", 2000, 400), ("item_limit", 500, 896)] for m in MODELS]
TF_CASES += [(r, N, J, "crossqr") for r, N, J in F64_CASES if J < 400]        # where CrossQr free-runs two sweeps only (crossqr_sweeps)


@pytest.mark.parametrize("regime,N,J,model", TF_CASES)
def test_f64_wide_teacher_forced(exe, cu_count, regime, N, J, model):
    """Four sweeps, each started from the oracle's state of the sweep before (pu.teacher_forced): GibbsRtIrtCrossQr's later sweeps without its chaos."""
    p = planned(exe, cu_count, regime, model, "f64", N, J)
    Y, logT, X, init, _ = problem(model, N, J)
    tol, floor = bound(J)
    worst = {}

    def check(t, dev, orc):
        for k in dev:
            if dev[k] is None or k == "nu":         # the device's nu is already the next sweep's draw: checked through that sweep
                continue
            e = float(pu.rel_err(dev[k], orc[k], floor).max())
            if e >= worst.get(k, (0.0, 0))[0]:
                worst[k] = (e, t)
            assert e < tol, (model, t, k, e)
    try:
        out = pu.teacher_forced(model, Y, logT, X, init, 4, "f64", check)
    finally:
        print(f"[{model} f64 {N} x {J} teacher-forced] largest error by field (error, sweep): {worst}; bound {tol:g}")
    pu.assert_engine_runs_plan(out["engine"].timing(), p)


# ---------------------------------------------------------------------------------------------------------------
# fp32, every model: one sweep from the oracle's state
F32_CASES = [("stride_runtime", 3000, 129), ("shrunk", 2000, 300), ("f32_one_subject_fused", 2000, 512), ("f32_one_subject_fused", 2000, 640),
             ("f32_one_subject_fuse_edge", 2000, 700), ("f32_one_subject_two_kernel", 2000, 896)]
ITEM_TOL, SUBJ_TOL, LL_TOL = 2e-3, 5e-4, 1e-4


def share_cap(J):
    """Share of subjects allowed beyond SUBJ_TOL: one flipped Polya-Gamma decision per 5e4 cells, a factor of four of headroom, J cells per subject."""
    return 8e-5 * J


def _abs_err(d, o):
    return np.abs(d - o) / np.maximum(np.abs(o), 1.0)


@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("regime,N,J", F32_CASES)
def test_f32_wide_one_sweep(exe, cu_count, regime, N, J, model):
    p = planned(exe, cu_count, regime, model, "f32", N, J)
    res = device_and_oracle(model, N, J, 1, "f32")
    tm = res["dev"]["engine"].timing()
    assert tm["cu_count"] == cu_count
    pu.assert_engine_runs_plan(tm, p)
    dev = pu.decode_rows(model, N, J, F, res["dev_ra"], res.get("dev_rt"), res["dev_qr"])
    orc = pu.decode_rows(model, N, J, F, res["orc"]["ra"], res["orc"]["rt"] if model != "mlirt" else None, res["orc"]["qr"])
    items = {k: float(_abs_err(dev[k][0], orc[k][0]).max()) for k in ("a", "b", "lambda_", "sig2t") if k in dev}
    struct = {k: float(_abs_err(dev[k][0], orc[k][0]).max()) for k in ("beta", "rho", "sigp") if k in dev and dev[k].shape[1]}
    subj_err = {k: _abs_err(dev[k][0], orc[k][0]) for k in ("theta", "zeta", "nu") if k in dev}
    shares = {k: float(np.mean(e > SUBJ_TOL)) for k, e in subj_err.items()}
    ll = abs(res["dev_ll"][0] - res["orc"]["ll"][0]) / abs(res["orc"]["ll"][0])
    cap = share_cap(J)
    print(f"[{model} f32 {N} x {J}] share of subject draws beyond {SUBJ_TOL:g}: {shares} (cap {cap:.3g}; largest {({k: float(e.max()) for k, e in subj_err.items()})}); "
          f"item draws {items}; structural {struct}; logLike {ll:.3g}")
    assert max(items.values()) < ITEM_TOL, items
    assert not struct or max(struct.values()) < ITEM_TOL, struct
    assert ll < LL_TOL, ll
    assert max(shares.values()) < cap, shares

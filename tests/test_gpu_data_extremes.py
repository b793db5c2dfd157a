"""Sweep-level parity on data that drives the samplers into their edge regions (parity_util.make_extreme_problem): separated items (cells
with z >= 8 take the reference form of the Polya-Gamma attempt inside the row kernels; every proposal bin is used), a saturated state
(|eta| up to ~2 000: p and 2 e^{-z} underflow, exp_neg_ll's clamp at 700), degenerate response patterns, raw log-millisecond response
times and covariates with a large offset -- on every schedule: the persistent launch (queue loop and team loop), the per-sweep fused
kernel, the two-kernel schedule and the Cross family's two-pass schedule.

Teacher forced (parity_util.teacher_forced) in runs of two sweeps: every sweep is compared with one oracle sweep from the state it
started from -- the first sweep of a run checks the prologue's row pass, the second the Polya-Gamma draws the sweep kernel itself made.  Tolerances are those of test_gpu_parity.py::test_teacher_forced:
  * fp64: every state and trace entry within 1e-8 relative (floor 1e-6);
  * fp32: >= 99.8 % of the subject draws and every item-level draw within 5e-4 (floor 1e-2), the log-likelihood within 1e-4 relative."""
import numpy as np
import pytest

import parity_util as pu

pytestmark = pytest.mark.gpu

N, J = 1200, 24                 # a persistent launch by default (<= 6 000 subjects, <= 2^17 cells)
T = 6
CROSS = ("crossqr", "cross")


def _L():
    return pu.ge.load_package()._lib


def _schedule(name):
    L = _L()
    return {"persistent": dict(), "per_sweep": dict(flags=L.FLAG_NO_PERSIST),
            "two_kernel": dict(flags=L.FLAG_NO_FUSE, block_threads=512, grid_blocks=32), "two_pass": dict()}[name]


def _cases(kinds):
    out = []
    for kind in kinds:
        for model in pu.extreme_models(kind):
            for sched in (("two_pass",) if model in CROSS else ("persistent", "per_sweep", "two_kernel")):
                for precision in ("f64", "f32"):
                    out.append(pytest.param(kind, model, sched, precision, id=f"{kind}-{model}-{sched}-{precision}"))
    return out


# Documented fp32 limits ("fp32 on extreme data"), measured on an MI355X with every sweep teacher forced; the fp64 engine meets
# 1e-8 on the same data.  Each entry bounds the sweeps that miss the fp32 tolerances: how many may, and by how much (measured -> bound).
#  * a Polya-Gamma decision flip: the fp32 attempt decides without guard bands (erm_rng.hpp pg1_attempt; about one cell in 5e4 --
#    test_gpu_samplers.py::test_pg1_f32_matches_oracle_except_rare_flips).  One flipped omega_ij moves that one item's b_j by ~omega / S0
#    and, through the item, the subjects; on separated items (a up to 8) by most.  Seen in one sweep of 6 (the same addressed cell):
#    separated Latent / LatentQr: 2.9 % of theta beyond 5e-4 (max 0.023), b_18 4.1e-3;  degenerate MlIrt: b_12 1.9e-3.
#  * response times at a log-millisecond offset with sigma2_t ~ 1e-4: fp32 C (logT) and the RT statistics' expanded squares lose ~1e-4 of
#    the log-likelihood (RtIrt 1.2e-4, Null 1.7e-4, in several sweeps); CrossQr's first sweep (nu drawn from the installed state) moves
#    71 % of zeta beyond 5e-4 (max 0.03), sigma2_t of the tiny-variance item by 0.35 and ll by 4.9e-3; later sweeps that item's sigma2_t by <= 1.1e-3.
FP32_LIMITS = {
    ("separated", "latentqr"): dict(sweeps=1, subj_frac=0.06, subj_max=0.05, item_max=1e-2, ll=1e-4),
    ("separated", "latent"): dict(sweeps=1, subj_frac=0.06, subj_max=0.05, item_max=1e-2, ll=1e-4),
    ("degenerate", "mlirt"): dict(sweeps=1, subj_frac=2e-3, subj_max=2e-3, item_max=5e-3, ll=1e-4),
    ("rt_offset", "rtirt"): dict(sweeps=6, subj_frac=2e-3, subj_max=2e-3, item_max=5e-4, ll=3e-4),
    ("rt_offset", "null"): dict(sweeps=6, subj_frac=2e-3, subj_max=2e-3, item_max=5e-4, ll=3e-4),
    ("rt_offset", "crossqr"): dict(sweeps=3, subj_frac=0.8, subj_max=0.1, item_max=0.7, ll=1e-2),
}


def _checker(model, precision):
    tol, floor = (1e-8, 1e-6) if precision == "f64" else (5e-4, 1e-2)

    def check(t, dev, orc):
        for k, v in dev.items():
            if v is None or k == "nu":         # device nu is already next run's draw; it is checked through the draws that use it
                continue
            assert np.all(np.isfinite(v)), (model, t, k)
            if precision == "f32":
                continue                       # the same values are the last trace row of the block: checked sweep by sweep in _check_traces
            e = pu.rel_err(v, orc[k], floor)
            assert e.max() < tol, (model, t, k, e.max())
    return check, tol, floor


def _check_traces(res, kind, model, precision, tol, floor):
    dev, orc = res["dev"], res["orc"]
    T_ = dev["ra"].shape[0]
    subj_frac, subj_max, item_max = np.zeros(T_), np.zeros(T_), np.zeros(T_)
    for k in ("ra", "rt"):
        if k not in dev:
            continue
        d, o = dev[k], orc[k]
        assert d.shape == o.shape and np.all(np.isfinite(d)), k
        e = pu.rel_err(d, o, floor)
        if precision == "f64":
            assert e.max() < tol, (k, e.max())
        subj_frac = np.maximum(subj_frac, np.mean(e[:, :N] > tol, axis=1))
        subj_max = np.maximum(subj_max, e[:, :N].max(axis=1))
        item_max = np.maximum(item_max, e[:, N:].max(axis=1))
    # Post.qr: the structural / item-level part, and vec(nu) behind it (CrossQr, LatentQr) -- every weight in fp64; fp32 draws the quantile
    # weights in fp32 (test_gpu_samplers.py::test_invgauss_and_qr_weight: about 1e-3 of them beyond 1e-3), checked through the draws that use them
    assert dev["qr"].shape == orc["qr"].shape and np.all(np.isfinite(dev["qr"]))
    w = orc["qr"].shape[1] - {"crossqr": N * J, "latentqr": N}.get(model, 0)
    eq = pu.rel_err(dev["qr"][:, :w], orc["qr"][:, :w], floor).max(axis=1)
    assert np.all(np.isfinite(dev["ll"]))
    ll = np.abs(dev["ll"] - orc["ll"]) / np.abs(orc["ll"])
    if precision == "f64":
        assert eq.max() < tol and ll.max() < 1e-8, (eq.max(), ll.max())
        if w < orc["qr"].shape[1]:
            assert pu.rel_err(dev["qr"][:, w:], orc["qr"][:, w:], floor).max() < tol
        return
    item_max = np.maximum(item_max, eq)
    miss = (subj_frac >= 2e-3) | (item_max >= tol) | (ll >= 1e-4)
    lim = FP32_LIMITS.get((kind, model), dict(sweeps=0))
    assert miss.sum() <= lim["sweeps"], (kind, model, np.flatnonzero(miss), subj_frac, subj_max, item_max, ll)
    if miss.any():
        assert subj_frac[miss].max() < lim["subj_frac"] and subj_max[miss].max() < lim["subj_max"], (subj_frac, subj_max)
        assert item_max[miss].max() < lim["item_max"] and ll[miss].max() < lim["ll"], (item_max, ll)


def _run(kind, model, sched, precision, nsweeps):
    Y, logT, X, init, _ = pu.make_extreme_problem(kind, model, N, J)
    check, tol, floor = _checker(model, precision)
    res = pu.teacher_forced(model, Y, logT, X, init, nsweeps, precision, check, chunk=2, **_schedule(sched))
    assert res["engine"].timing()["persistent"] == (1 if sched == "persistent" else 0)
    _check_traces(res, kind, model, precision, tol, floor)
    return res


@pytest.mark.parametrize("kind,model,sched,precision", _cases(("separated", "degenerate", "rt_offset", "x_offset")))
def test_teacher_forced_extremes(kind, model, sched, precision):
    _run(kind, model, sched, precision, T)


@pytest.mark.parametrize("kind,model,sched,precision", _cases(("saturated",)))
def test_saturated_state(kind, model, sched, precision):
    """One run of two sweeps from the injected state: cells with z > 745 (p / (p + 2 e^{-z}) is 0 / 0 and the IG proposal is taken), |eta|
    beyond exp_neg_ll's clamp at 700 in the log-likelihood, PG weights ~1 / (4 z) in the item draws -- every draw finite and on the oracle's."""
    _run(kind, model, sched, precision, 2)


@pytest.mark.parametrize("model", pu.MODELS)
def test_degenerate_free_running(model):
    """All-1 / all-0 items and subjects through the engine's sufficient statistics and fused head for 20 sweeps: erm_run succeeds, nothing
    non-finite, and the item traces of the degenerate items are the oracle's over the first three sweeps (free-running parity; CrossQr is
    chaotic beyond that -- test_gpu_parity.py)."""
    Y, logT, X, init, _ = pu.make_extreme_problem("degenerate", model, N, J)
    dev = pu.run_device(model, Y, logT, X, init, 20, precision="f64")          # raises on a non-zero return of erm_run
    for k in ("ra", "rt", "qr", "ll"):
        if k in dev:
            assert np.all(np.isfinite(dev[k])), k
    for v in dev["state"].values():
        assert v is None or np.all(np.isfinite(v))
    op = pu.OracleProblem(model, Y, logT, X, init, qRt=0.85, cov2one=model not in ("latentqr", "latent"))       # run_device's qRt
    orc = op.run(3)
    items = [0, 1, 2, 3, 4]
    for off in (N, N + J):                     # a, b of the degenerate items in Post.ra
        cols = [off + j for j in items]
        assert pu.rel_err(dev["ra"][:3, cols, 0], orc["ra"][:, cols]).max() < 1e-8
    if model != "mlirt":
        for off in (N, N + J):                 # lambda, sigma2_t
            cols = [off + j for j in items]
            assert pu.rel_err(dev["rt"][:3, cols, 0], orc["rt"][:, cols]).max() < 1e-8

"""The passes behind a sweep and DIC's loglik_kernel on extreme data (parity_util.make_extreme_problem at 1 200 x 24: |eta| up to ~2 000, sigma2_t ~ 1e-4, a constant
logT column, all-0 / all-1 units): where p underflows, y eta - log1pexp(eta) cancels and (logT - mu)^2 / var is huge.  6 free-running sweeps, burn-in 2, WAIC in
subject units next to the replicate pass, then WAIC in cell units, DIC at the end; fp64 on every kind and model, fp32 on GibbsRtIrt and GibbsRtIrtCrossQr.

The reference is NOT the fp64 twin but the same definitions in np.longdouble from the engine's own traces (pass_util.Extended), with the response term in the form
that does not cancel and, beside every unit's value, its condition sum cond_u = sum |y eta| + |log1pexp(eta)| + |rt terms|.  Bounds, all derived from cond_u:
  unit sums (subject and cell l per row -- through lppd_u and p_u --, D_obs and D^T_obs, DIC's log-likelihood):   |dev - ref| <= c 2^-53 cond_u + 2^-1022,
      c = 8 x pass_util.EXTREME_C[kind] (the fp64 numpy twins' own largest ratio on the oracle chain, measured by tests/test_pass_geometry_host.py), at least 8;
  lppd_u within the largest per-row bound delta_u of the unit plus the finish's own (n + 4 + 2 log n) 2^-53 (pass_util.waic_bounds says why); p_u within
      2 sd_u delta' + delta'^2 + 2^-1022, delta' = delta_u sqrt(n / (n - 1)), sd_u from the reference (defined where the reference variance is exactly zero);
  replicate means (D_rep, D^T_rep, T_rep) within the bound of their unit sums; counts equal to the twin's under ppc_util's margin rule with its 0.1 % cap.
Every figure is printed before it is asserted (pytest -s)."""
import numpy as np
import pytest

import parity_util as pu
import pass_util as pa
import test_gpu_predictive as tp

pytestmark = pytest.mark.gpu

N, J = pa.EXTREME_SHAPE


def _cases():
    out = []
    for kind in pu.EXTREME_KINDS:
        for model in pu.extreme_models(kind):
            for precision in ("f64", "f32") if model in ("rtirt", "crossqr") else ("f64",):
                out.append(pytest.param(kind, model, precision, id=f"{kind}-{model}-{precision}"))
    return out


def _traces(eng, model):
    L = pu.ge.load_package()._lib
    return eng.trace(L.TRACE_RA), None if model == "mlirt" else eng.trace(L.TRACE_RT), eng.trace(L.TRACE_QR)


def _excess(got, ref, bound):
    """Largest (|got - ref| / bound) over the entries; an entry with a zero bound must be met exactly."""
    d = np.abs(np.asarray(got).astype(pa.LD) - ref)
    b = np.asarray(bound, dtype=pa.LD)
    r = np.where(d > 0, d / np.where(b > 0, b, 1), 0)
    r = np.where((d > 0) & ~(b > 0), np.inf, r)
    return float(np.max(r))


@pytest.mark.parametrize("kind,model,precision", _cases())
def test_passes_on_extreme_data_meet_the_bounds_derived_from_the_condition_sums(kind, model, precision):
    Y, logT, X, init, _ = pu.make_extreme_problem(kind, model, N, J)
    c = pa.device_c(kind)
    n_iter, burn = pa.EXTREME_CHAIN["n_iter"], pa.EXTREME_CHAIN["n_burnin"]
    what = f"{kind} {model} {precision}"
    worst = {}
    # ---- engine 1: WAIC in subject units next to the replicate pass; DIC at the end
    eng = tp._engine(model, Y, logT, X, init, precision=precision, waic="subject", ppc=1, **pa.EXTREME_CHAIN)
    eng.run(n_iter)
    Yd, logTd, Xd = eng.get_data()                 # (the fp32 engine's data set is the rounded one, covariates included)
    ra, rt, qr = _traces(eng, model)
    ref = pa.extended_reference(model, Yd, logTd, ra, rt, qr, n_iter=n_iter, n_burnin=burn)
    lppd_u, p_u = eng.pointwise()
    w = eng.waic()
    assert np.all(np.isfinite(lppd_u)) and np.all(np.isfinite(p_u)) and all(np.isfinite(v) for v in w.values()), what
    lppd, dl, p, dp = pa.waic_bounds(ref["L_subj"], ref["C_subj"], c)
    worst["lppd subject"], worst["p subject"] = _excess(lppd_u, lppd, dl), _excess(p_u, p, dp)
    dev = tp._device(eng, 1)
    for a in (dev.item, dev.subj, dev.total):
        assert np.all(np.isfinite(a) | np.isnan(a) & (model == "mlirt")), what
    arr = {"subject": dev.subj, "item": dev.item, "total": dev.total}
    for unit, slots in pa.PPC_SLOTS.items():
        for name, (comp, q) in slots.items():
            if name in ref["ppc"][unit]:
                v, cv = ref["ppc"][unit][name]
                worst[f"{unit} {name}"] = _excess(arr[unit][comp, q], v, c * pa.U53 * cv + pa.FLOOR)
    host, _ = tp._twin(eng, model, n_chain=1, thin=1, **pa.EXTREME_CHAIN)
    d, m = eng.dic(), eng.get_mean()
    assert all(np.isfinite(v) for v in d.values()), (what, d)
    F = 0 if model in pu.CQ_MODELS or model == "null" else 3
    v, cv = pa.Extended(model, Yd, logTd).loglik(m, Xd, F)
    worst["DIC loglik"] = _excess(-0.5 * d["Dhat"], v, c * pa.U53 * cv + pa.FLOOR)
    eng.close()
    # ---- engine 2: WAIC in cell units
    eng = tp._engine(model, Y, logT, X, init, precision=precision, waic="cell", **pa.EXTREME_CHAIN)
    eng.run(n_iter)
    Yd, logTd, _ = eng.get_data()
    ra, rt, qr = _traces(eng, model)
    ref2 = pa.extended_reference(model, Yd, logTd, ra, rt, qr, n_iter=n_iter, n_burnin=burn)
    lppd_c, p_c = eng.pointwise()
    assert np.all(np.isfinite(lppd_c)) and np.all(np.isfinite(p_c)) and all(np.isfinite(x) for x in eng.waic().values()), what
    lppd, dl, p, dp = pa.waic_bounds(ref2["L_cell"], ref2["C_cell"], c)
    worst["lppd cell"], worst["p cell"] = _excess(lppd_c, lppd, dl), _excess(p_c, p, dp)
    n_zero = int(np.sum(p == 0))
    eng.close()
    print(f"{what}: c = {c:g}; |dev - ref| / bound by quantity: " + ", ".join(f"{k} {x:.3g}" for k, x in worst.items()) + f"; cells of exactly zero reference variance {n_zero}")
    assert max(worst.values()) <= 1.0, (what, max(worst, key=worst.get), max(worst.values()))
    pa.assert_counts_equal_twin(dev, host, what=what)

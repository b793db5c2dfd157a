"""The passes behind a sweep (WAIC in subject and in cell units, the replicate pass and its item step) and DIC's loglik_kernel at the edges of their launch geometry:
every lane width on both sides of every switch, subject tails down to one subject, the item step's empty and half-full parts, all three grid caps, the LDS edge of
the replicate pass (163 696 of 163 840 bytes at 787 items) and loglik_kernel's workgroup ranges -- pass_util's table, each case asserted from the plan (pass_util.pass_geom
with the card's compute units; tests/test_pass_geometry_host.py holds that to erm_geometry.hpp) to be in the regime its id claims.

Compared as tests/test_gpu_waic.py, tests/test_gpu_predictive.py and tests/test_gpu_dic.py compare, with their helpers and tolerances: getWaicHost / getPpcHost on
erm_get_data's data set and the engine's own traces (1e-10 relative for means, lppd_u, p_u and totals, LPPD_FLOOR, counts exact under ppc_util's margin rule),
erm_get_dic's D-hat against getLogLikelihood at the pulled Post.mean (1e-10; fp32 2e-6) and D-bar against the pulled logLike rows (1e-12).  Chains of 4 sweeps,
burn-in 1: three rows, three replicates.  One engine runs WAIC in subject units next to the replicate pass, a second WAIC in cell units."""
import numpy as np
import pytest

import parity_util as pu
import pass_util as pa
import ppc_util as ppu
import waic_util as wu
import test_gpu_predictive as tp
import test_gpu_waic as tw

pytestmark = pytest.mark.gpu

REF_CU = 256                    # the ids of the parametrised cases are those of an MI355X; the cap cases' sizes are computed again from the card (below)


@pytest.fixture(scope="module")
def cu_count():
    L = pu.ge.load_package()._lib
    eng = L.Engine(model=1, n_item=5, n_subj=30, n_feat=0, n_iter=1, n_chain=1, n_burnin=0, cov2one=1, q_rt=0.85, seed=1, precision=1, trace_mode=0)
    cu = eng.timing()["cu_count"]
    eng.close()
    assert cu >= 1
    return cu


def _on_this_card(case, cu):
    """The case as the card's compute-unit count makes it (the WAIC cap cases), and its plan, asserted to be in the case's regime."""
    case = next(c for c in pa.replicate_cases(cu) + pa.dic_cases() if c.id == case.id)
    p = pa.pass_geom(case.model, case.N, case.J, cu)
    miss = pa.regime_misses(case, p, cu)
    print(f"\n[{case.id}] {case.N} x {case.J}, {cu} compute units; plan {p}")
    assert not miss, f"{case.id} is not in its regime: {miss}; plan {p}"
    return case


def _x(X):
    return None if X is None or X.shape[1] == 0 else X


@pytest.mark.parametrize("case", [pytest.param(c, id=c.id) for c in pa.replicate_cases(REF_CU)])
def test_waic_and_replicates_equal_the_twins_at_the_edges_of_the_geometry(case, cu_count):
    case = _on_this_card(case, cu_count)
    Y, logT, X, init, _ = pa.problem(case.model, case.N, case.J, case.F, case.seed)
    kw = dict(n_chain=1, **pa.CHAIN)
    eng = tp._engine(case.model, Y, logT, _x(X), init, precision=case.precision, waic="subject", ppc=1, **pa.CHAIN)
    eng.run(pa.CHAIN["n_iter"])
    assert eng.post_count == 3 and eng.predictive_reps == 3
    tw._assert_equals_twin(eng, tw._twin(eng, case.model, unit="subject", **kw), what=f"{case.id} subject")
    host, _ = tp._twin(eng, case.model, thin=1, **kw)
    dev = tp._device(eng, 1)
    ppu.assert_equals_twin(dev, host, what=case.id)
    ppu.check_counts(dev)
    eng.close()
    eng = tp._engine(case.model, Y, logT, _x(X), init, precision=case.precision, waic="cell", **pa.CHAIN)
    eng.run(pa.CHAIN["n_iter"])
    tw._assert_equals_twin(eng, tw._twin(eng, case.model, unit="cell", **kw), what=f"{case.id} cell")
    eng.close()


@pytest.mark.parametrize("case", [pytest.param(c, id=c.id) for c in pa.dic_cases()])
def test_dic_equals_the_host_evaluation_at_every_workgroup_split(case, cu_count):
    case = _on_this_card(case, cu_count)
    pkg = pu.ge.load_package()
    Y, logT, X, init, _ = pa.problem(case.model, case.N, case.J, case.F, case.seed)
    N, J = Y.shape
    r = pu.run_device(case.model, Y, logT, _x(X), init, pa.CHAIN["n_iter"], precision=case.precision, n_burnin=pa.CHAIN["n_burnin"])
    eng = r["engine"]
    d, m = eng.dic(), eng.get_mean()
    # what getLogLikelihood reads of a sampler, on the ORIGINAL data (the fp32 engine's is the rounded one: tests/test_gpu_dic.py's 2e-6)
    M = wu.as_sampler(case.model, Y, logT, None, None, None, nIter=pa.CHAIN["n_iter"], nChain=1, nBurnin=pa.CHAIN["n_burnin"])
    M.Cond.nFeat, M.Data.X = 0, np.zeros((N, 0))
    P = pkg.InputPara(theta=m["theta"], a=m["a"], b=m["b"])
    for k_src, k_dst in (("zeta", "zeta"), ("lambda_", "lam"), ("sig2t", "sig2t"), ("sigp", "Sigp"), ("beta", "beta"), ("rho", "rho"), ("nu", "nu")):
        if m.get(k_src) is not None:
            setattr(P, k_dst, m[k_src])
    Dhat, Dbar = -2.0 * pkg.getLogLikelihood(M, P), -2.0 * float(np.mean(r["ll"]))
    tol = 1e-10 if case.precision == "f64" else 2e-6
    print(f"{case.id}: Dhat {d['Dhat']!r} / {Dhat!r} rel {abs(d['Dhat'] - Dhat) / abs(Dhat):.3g}, Dbar {d['Dbar']!r} / {Dbar!r} rel {abs(d['Dbar'] - Dbar) / abs(Dbar):.3g}")
    assert np.isfinite(d["Dhat"]) and np.isfinite(d["Dbar"])
    assert abs(d["Dhat"] - Dhat) <= tol * abs(Dhat) and abs(d["Dbar"] - Dbar) <= 1e-12 * abs(Dbar)
    eng.close()

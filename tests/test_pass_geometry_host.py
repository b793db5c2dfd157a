"""The geometry of the passes behind a sweep and of DIC's loglik_kernel on the CPU (no GPU): erm_geometry.hpp's pass_geom compiled by g++ with
UndefinedBehaviorSanitizer and -ftrapv into tests/pass_geom_check.cpp, which replays the kernels' index loops on every plan of N in 1 ... 10 000 (and a few large
values) x J in 1 ... 896 x {1, 64, 256, 304} compute units; every GPU case of tests/test_gpu_pass_geometry.py lands in the regime its id claims, in the C++ plan and
in its Python restatement (pass_util.pass_geom) alike; the oracle chain stays finite at every case's shape; ppc_util's margin rule excludes at most 0.1 % of the units
at every replicate-pass case and on the oracle chain of every extreme-data case, where the constants c of the device's bounds (pass_util.EXTREME_C) are measured again.

Seeds: a case whose oracle chain decides a unit within the margin gets another seed in pass_util's table -- the cap is a condition and is never changed."""
import os
import subprocess

import numpy as np
import pytest

import parity_util as pu
import pass_util as pa
import ppc_util as ppu

pkg = pu.ge.load_package()
HOST_CU = 256                   # the cap cases are computed from the card's compute units on the GPU; here from an MI355X's
SRC = os.path.join(pu.ROOT, "tests", "pass_geom_check.cpp")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("passgeom") / "pass_geom_check")
    subprocess.run(["g++", "-std=c++17", "-O2", "-g", "-fsanitize=undefined", "-fno-sanitize-recover=all", "-ftrapv", "-I", pu.GEOMETRY_INC, SRC, "-o", out], check=True)
    return out


def cpp_plan(exe, model, N, J, cu):
    r = subprocess.run([exe, "case", str(pu.MODELS[model]), str(N), str(J), str(cu)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and not r.stdout.startswith("error="), r.stdout + r.stderr
    return {k: int(v) for k, v in (kv.split("=", 1) for kv in r.stdout.split())}


def test_sweep_replays_every_index_loop_without_undefined_behaviour(exe):
    r = subprocess.run([exe], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "invariant failures 0" in r.stdout, r.stdout


def test_python_side_of_the_plan_equals_the_header(exe):
    g = np.random.default_rng(5)
    shapes = [(int(N), int(J)) for N, J in zip(g.integers(1, 300_000, 60), g.integers(1, 897, 60))] + [(1, 1), (4294967295, 896), (9, 787), (5, 788), (65537, 1), (4101, 129)]
    shapes += [(257, J) for J in range(1, 131)]              # every switch of the lane width, both sides
    for N, J in shapes:
        for model in ("mlirt", "rtirt", "crossqr", "latent"):
            for cu in (1, 256, 304):
                assert pa.pass_geom(model, N, J, cu) == cpp_plan(exe, model, N, J, cu), (model, N, J, cu)


@pytest.mark.parametrize("cu", [1, 64, 256, 304])
def test_every_gpu_case_lands_in_the_regime_its_id_claims(exe, cu):
    cases = pa.replicate_cases(cu) + pa.dic_cases()
    assert len({c.id for c in cases}) == len(cases)
    for c in cases:
        p = cpp_plan(exe, c.model, c.N, c.J, cu)
        assert p == pa.pass_geom(c.model, c.N, c.J, cu), c.id
        if cu == HOST_CU:
            print(c.id, f"{c.N} x {c.J}", p)
        # (with one compute unit every grid is capped early: the regimes that name an uncapped WAIC grid are properties of a real card)
        if cu >= 64 or c.regime[0] in ("cap_pred", "cap_waic", "lds_edge", "lds_ra", "dic", "dic_past_end"):
            assert not pa.regime_misses(c, p, cu), (c.id, pa.regime_misses(c, p, cu), p)


def test_the_lds_edge_is_where_the_issue_found_it():
    assert pa.pass_geom("rtirt", 9, 787, 256)["lds_pred"] == 163_696 and pa.pass_geom("rtirt", 9, 787, 256)["T"] == 256
    assert pa.pass_geom("rtirt", 9, 788, 256)["T"] == 128 and pa.pass_geom("mlirt", 9, 896, 256)["lds_pred"] == 129_024
    assert pa.pass_geom("rtirt", 300, 896, 256)["T"] == 128 and pa.pass_geom("rtirt", 300, 896, 256)["lds_pred"] == 114_688


@pytest.mark.parametrize("model", pa.X_SINGULAR_AT_ONE_SUBJECT)
def test_one_subject_with_a_covariate_is_no_model(model):
    """Why the N = 1 tail cases of GibbsMlIrt and GibbsRtIrt run without covariates: the regression of one subject's theta on [1 x] is singular, beta is NaN after the
    first step of the first sweep and the chain never recovers (the oracle's samplers return NaN for a NaN argument).  Without covariates the chain is finite."""
    Y, logT, X, init, _ = pu.make_problem(model, 1, 4, 1, seed=17)
    t = pu.OracleProblem(model, Y, logT, X, init, qRt=0.85).run(4)
    assert not np.all(np.isfinite(t["ra"])) and not np.all(np.isfinite(t["qr"]))
    M = pa.oracle_sampler(pa.Case("x", ("tail", "one"), model, "f64", 1, 4, 0, 17), 4, 1)
    assert np.all(np.isfinite(M.Post.ra)) and np.all(np.isfinite(M.Post.qr))


@pytest.mark.parametrize("J", [5, 257])
def test_one_subject_under_latentqr_is_no_model(J):
    """Why GibbsRtIrtLatentQr has no N = 1 DIC case: zeta is regressed on [1 theta], singular with one subject also without covariates -- the oracle chain is not
    finite at 1 x 5 and 1 x 257, while GibbsRtIrtLatent's (no weights) is."""
    c = pa.Case("x", ("dic",), "latentqr", "f64", 1, J, 0, 17)
    M = pa.oracle_sampler(c, **pa.CHAIN)
    assert not (np.all(np.isfinite(M.Post.ra)) and np.all(np.isfinite(M.Post.rt)) and np.all(np.isfinite(M.Post.qr)))
    M = pa.oracle_sampler(c._replace(model="latent"), **pa.CHAIN)
    assert np.all(np.isfinite(M.Post.ra)) and np.all(np.isfinite(M.Post.rt)) and np.all(np.isfinite(M.Post.qr))


def _replicate_case_ids():
    return [pytest.param(c, id=c.id) for c in pa.replicate_cases(HOST_CU) if c.precision == "f64"]


@pytest.mark.parametrize("case", _replicate_case_ids())
def test_oracle_chain_is_finite_and_decides_every_count_at_the_gpu_cases(case):
    """tests/test_gpu_pass_geometry.py compares counts exactly except for units whose smallest non-zero |D_rep - D_obs| is within 1e-9 of the compared magnitudes, at
    most 0.1 % of a case's units: on the oracle chain of the case (same data, initial values, seed, chain length and thinning) the rule stays within that cap."""
    M = pa.oracle_sampler(case, **pa.CHAIN)
    for tr in (M.Post.ra, M.Post.rt, M.Post.qr):
        assert tr is None or np.all(np.isfinite(tr)), case.id
    P = pkg.getPpcHost(M, thin=1, seed=1234)
    n_ex, n = pa.excluded_share(P)
    print(f"{case.id}: {case.N} x {case.J}, excluded {n_ex} of {n}, smallest margin {min(float(np.min(v)) for v in P.margin.values()):.3g}")
    assert P.R == 3 and n_ex <= ppu.MAX_EXCLUDED * n
    W = pkg.getWaicHost(M, "subject")
    assert np.all(np.isfinite(W.lppd_u)) and np.all(W.p_u > 0)       # (the purely relative bound on p_u needs a non-zero variance: benign data)


@pytest.mark.parametrize("case", [pytest.param(c, id=c.id) for c in pa.dic_cases() if c.precision == "f64" and c.N < 1000])
def test_oracle_chain_is_finite_at_the_dic_cases(case):
    M = pa.oracle_sampler(case, **pa.CHAIN)
    for tr in (M.Post.ra, M.Post.rt, M.Post.qr):
        assert tr is None or np.all(np.isfinite(tr)), case.id


# ----------------------------------------------------------------------------------------------------------------- extreme data
def _extreme_cases():
    return [pytest.param(kind, model, id=f"{kind}-{model}") for kind in pu.EXTREME_KINDS for model in pu.extreme_models(kind)]


def extreme_measurement(kind, model):
    """The oracle chain of tests/test_gpu_pass_extremes.py's case, the twins on it, and their largest ratio against the extended reference by quantity."""
    N, J = pa.EXTREME_SHAPE
    prob = pu.make_extreme_problem(kind, model, N, J)
    Y, logT, X, init, _ = prob
    n_iter, burn = pa.EXTREME_CHAIN["n_iter"], pa.EXTREME_CHAIN["n_burnin"]
    M = pa.oracle_sampler(pa.Case("x", (), model, "f64", N, J, 3, 0), n_iter, burn, prob=prob)
    ref = pa.extended_reference(model, Y, logT, M.Post.ra, M.Post.rt, M.Post.qr, n_iter=n_iter, n_burnin=burn)
    G = pkg.twins
    ratios = {"l subject": pa.worst_ratio(G.pointwiseLogLikHost(M, "subject"), ref["L_subj"], ref["C_subj"]),
              "l cell": pa.worst_ratio(G.pointwiseLogLikHost(M, "cell").reshape(ref["n"], J, N).transpose(0, 2, 1), ref["L_cell"], ref["C_cell"])}
    P = pkg.getPpcHost(M, thin=1, seed=1234)
    ratios.update({f"{u} {q}": r for (u, q), r in pa.ppc_ratios(P, ref).items()})
    # DIC's log-likelihood at the mean of the post-burn-in rows
    F = 0 if model in pu.CQ_MODELS else 3
    f = pu.decode_rows(model, N, J, F, pu.trace_rows(M.Post.ra), None if model == "mlirt" else pu.trace_rows(M.Post.rt), pu.trace_rows(M.Post.qr))
    mean, _, _ = pu.expected_mean(f, burn, 1)
    m = {k: v.astype(np.float64) for k, v in mean.items()}
    e = np.zeros(0)
    Pm = pkg.InputPara(theta=m["theta"], a=m["a"], b=m["b"], zeta=m.get("zeta", e), lam=m.get("lambda_", e), sig2t=m.get("sig2t", e), Sigp=m.get("sigp", e), beta=m.get("beta", e),
                       rho=m.get("rho", e), nu=m.get("nu", e))
    M.Cond.nFeat, M.Data.X = 3, X if X is not None else np.zeros((N, 3))
    v, cv = pa.Extended(model, Y, logT).loglik(m, X, 0 if model in pu.CQ_MODELS or model == "null" else 3)
    ratios["DIC loglik"] = pa.worst_ratio(pkg.getLogLikelihood(M, Pm), v, cv)
    return M, P, ref, ratios


@pytest.mark.parametrize("kind,model", _extreme_cases())
def test_extreme_data_cap_of_the_margin_rule_and_the_measured_constant(kind, model):
    """On the oracle chain of every extreme case: everything finite, the margin rule within its 0.1 % cap, and the fp64 numpy twins within pass_util.EXTREME_C[kind]
    (in units of 2^-53 cond_u) of the extended reference -- the constant the device's bound is eight times of."""
    M, P, ref, ratios = extreme_measurement(kind, model)
    n_ex, n = pa.excluded_share(P)
    print(f"MEASURED {kind} {model}: excluded {n_ex} of {n}; c by quantity " + ", ".join(f"{k} {v:.3g}" for k, v in ratios.items()))
    assert n_ex <= ppu.MAX_EXCLUDED * n
    assert np.all(np.isfinite(ref["L_cell"].astype(np.float64)))
    assert max(ratios.values()) <= pa.EXTREME_C[kind], (max(ratios, key=ratios.get), max(ratios.values()))

"""The person fit on the CPU: csrc/erm_fit.hpp, the header fit_kernel is built on, compiled by g++ with UndefinedBehaviorSanitizer and -ftrapv into
the stand-alone tests/fit_check.cpp, and personFitHost, the numpy twin the device is compared with in tests/test_gpu_person_fit.py.
  - fit_check self: the response pieces by enumeration of all 2^J patterns (theta far from every b_j at a_j = 8 included), Wilson-Hilferty against its formula,
    the FitMS merge against one-pass long-double sums and its symmetry bit for bit, FitAcc against two passes, fit_finish's NaN rules.
  - the quadratic form against numpy.linalg.solve on the dense covariance: v = 0, rho != 0, J in {1, 7, 65}.
  - the chi^2 tail, the header's and the twin's, against scipy.stats.chi2.sf on n in {1, 2, 3, 4, 9, 10, 65, 448, 895, 896}, x from 0 to 6 n + 60 and 1e-300,
    1399.9, 1400.1, 1e4, 1e6: measured 5.4e-15 (header) and 4.3e-15 (twin) absolute; pinned at 10 x the header's.
  - the twin against scipy.integrate.quad with scipy's own chi2.sf and norm.cdf (fit_util.quad_fit): one subject per model, J = 7 and 50, Q = 61, both
    weightings, and n_i = 7 of 50 masked.  Measured worst 2.7e-7 (pResp of rtirt at J = 7; the scores' twin stands 5.3e-6 from its quadrature); pinned at 10 x.
  - the masked twin against the unmasked twin on every subject's reduced data set; n_i = 0 against the NaN rule.
  - on data simulated from the model at its generating parameters (fixed seeds): the chi^2 pivot at the true theta passes a KS test, clean respondents are
    flagged at no more than the nominal rate plus a binomial margin, planted guessers and planted time shifts are flagged at least five times as often as clean
    respondents, and the component that was not touched stays below three times the nominal rate.
  - the preconditions of tests/test_gpu_person_fit.py: the twin's conditioning on its cases against numpy.longdouble, and every S at least 0.1 from 2.
  - the plumbing: the four symbols, ABI 4, obs=None, the fifth pass's words."""
import os
import subprocess

import numpy as np
import pytest

import fit_util as fu
import marginal_util as mu
import obs_util as ou
import parity_util as pu

SRC = os.path.join(pu.ROOT, "tests", "fit_check.cpp")
INC = os.path.join(pu.ROOT, "extendedrtirtmodeling.jl_amd", "csrc")
TAIL_NS = (1, 2, 3, 4, 9, 10, 65, 448, 895, 896)
TAIL_MEASURED = 5.5e-15          # the header's largest absolute error against chi2.sf on the grid below (the twin: 4.3e-15)
QUAD_MEASURED = 2.7e-7           # the twin's largest error against fit_util.quad_fit over test_twin_equals_quadrature's cases
ALPHA = 0.05


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("fit") / "fit_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=undefined", "-fno-sanitize-recover=all", "-ftrapv", "-I", INC, SRC, "-o", out], check=True)
    return out


def _run(exe, args):
    r = subprocess.run([exe, *map(str, args)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "runtime error" not in r.stderr, r.stdout[-2000:] + r.stderr[-2000:]
    return r.stdout.split("\n")[:-1]


def test_header_against_long_double(exe):
    assert _run(exe, ["self"])[-1] == "failures 0"


@pytest.mark.parametrize("J", [1, 7, 65])
@pytest.mark.parametrize("kind", ["plain", "v0", "rho"])
def test_quadratic_form_equals_the_dense_solve(exe, kind, J):
    g = np.random.default_rng(J + 17)
    sg, lam, t = g.uniform(0.1, 0.6, J), 4.0 + 0.3 * g.normal(size=J), 4.0 + 0.7 * g.normal(size=J)
    rho = 0.3 * g.normal(size=J) if kind == "rho" else np.zeros(J)
    m0, m1, v, th = 0.2, -0.4, 0.0 if kind == "v0" else 0.35, 0.8
    out = _run(exe, ["quad", J, repr(th), repr(m0), repr(m1), repr(v), *(repr(float(x)) for j in range(J) for x in (sg[j], lam[j], t[j], rho[j]))])
    qf, back = float(out[0]), float(out[1])
    want = fu.dense_quad(sg, lam, t, rho, m0, m1, v, th)
    print(f"{kind} J={J}: Qf {qf:.12g}, dense solve {want:.12g}, -2 (marg_T - constants) {back:.12g}")
    assert abs(qf - want) <= 1e-11 * want and abs(back - qf) <= 1e-12 * qf


def _tail_grid():
    xs, ns = [], []
    for n in TAIL_NS:
        x = np.concatenate([np.linspace(0.0, 6.0 * n + 60.0, 400), [1e-300, 1399.9, 1400.1, 1e4, 1e6]])
        xs.append(x)
        ns.append(np.full(x.size, n))
    return np.concatenate(xs), np.concatenate(ns)


def test_tail_equals_scipy(exe):
    from scipy.stats import chi2
    xs, ns = _tail_grid()
    want = chi2.sf(xs, ns)
    head = np.array([float(v) for v in _run(exe, ["tail", *(a for x, n in zip(xs, ns) for a in (repr(float(x)), int(n)))])])
    twin = fu.pkg().twins.chi2TailHost(xs, ns)
    e_head, e_twin = float(np.max(np.abs(head - want))), float(np.max(np.abs(twin - want)))
    print(f"chi^2 tail against scipy on {xs.size} points: header {e_head:.3g}, twin {e_twin:.3g} absolute")
    assert e_head <= 10 * TAIL_MEASURED and e_twin <= 10 * TAIL_MEASURED
    assert np.all(head[xs > 1400.0] == 0.0) and np.all((head >= 0.0) & (head <= 1.0 + 10 * TAIL_MEASURED))      # (the sum is not clamped: it may pass 1 by its rounding)


def test_wilson_hilferty_is_descriptive_only():
    """Its tail error against the exact chi^2 (DESIGN.md 7n's table; no bound of any test): 0.037 at n = 1, 1.0e-3 at n = 12, 1.2e-5 at n = 896."""
    from scipy.stats import chi2, norm
    T = fu.pkg().twins
    seen = []
    for n in (1, 12, 896):
        x = np.linspace(0.0, 6.0 * n + 60.0, 4001)[1:]
        z = T.wilsonHilfertyHost(x, n)
        c = 2.0 / (9.0 * n)
        assert np.max(np.abs(z - ((x / n) ** (1.0 / 3.0) - (1.0 - c)) / np.sqrt(c))) <= 1e-12 * np.max(np.abs(z))          # its formula
        seen.append(float(np.max(np.abs(norm.sf(z) - chi2.sf(x, n)))))
        print(f"Wilson-Hilferty n={n}: tail error {seen[-1]:.3g}")
    assert seen[0] > seen[1] > seen[2] > 0.0          # an approximation, better with n: the reason the p-value does not use it
    assert np.isnan(T.wilsonHilfertyHost(3.0, 0))


@pytest.mark.parametrize("model", mu.MODELS)
def test_twin_equals_quadrature(model):
    P = fu.pkg()
    worst = {}
    for J in (7, 50):
        rows = mu.make_rows(model, J, 3, 3, seed=3)
        Y, logT, X = mu.make_data(model, 1, J, 3, seed=3)
        Xk = ou.kernel_x(model, X)
        masks = [None]
        if J == 50:
            o = np.zeros((1, 50), dtype=np.uint8)
            o[0, np.random.default_rng(5).choice(50, 7, replace=False)] = 1
            masks.append(o)
        for o in masks:
            for w in fu.WEIGHTINGS:
                ref = fu.quad_fit(model, Y, logT, Xk, rows, w, obs=o)
                tw = P.personFitHost(mu.CODE[model], Y, logT, Xk, rows, 61, w, obs=o)
                for c, e in fu.errors(tw, ref, fu.COLS).items():
                    worst[c] = max(worst.get(c, 0.0), e)
                assert tw.nCoarse == 0 and (o is None or tw.nObs[0] == 7)
    print(f"{model}: personFitHost against quad, worst " + ", ".join(f"{c} {e:.3g}" for c, e in worst.items()))
    assert max(worst.values()) <= 10 * QUAD_MEASURED


@pytest.mark.parametrize("model", mu.MODELS)
def test_masked_twin_equals_the_twin_on_the_reduced_data(model):
    P = fu.pkg()
    Y, logT, X, rows, obs = ou.problem(model, 12, 9, 3, seed=29)
    Yp, lp = ou.poison(Y, logT, obs)
    for w in fu.WEIGHTINGS:
        got = P.personFitHost(mu.CODE[model], Yp, lp, X, rows, 61, w, obs=obs)
        assert np.array_equal(got.nObs, obs.sum(axis=1))
        for i in range(12):
            red = ou.reduced_subject(model, Y, logT, X, rows, obs, i)
            if red is None:      # n_i = 0: NaN in the four statistics, the rows' size and the flag as ever
                assert all(np.isnan(getattr(got, c)[i]) for c in fu.STATS) and np.isfinite(got.rowEss[i]) and got.coarse[i] in (False, True)
                continue
            one = P.personFitHost(mu.CODE[model], *red[:3], red[3], 61, w)
            for c in fu.COLS:
                a, b = getattr(got, c)[i], getattr(one, c)[0]
                assert (np.isnan(a) and np.isnan(b)) or abs(a - b) <= 1e-12 * max(abs(b), 1.0), (c, i, a, b)
            assert got.coarse[i] == one.coarse[0]
    same = P.personFitHost(mu.CODE[model], Y, logT, X, rows, 61, "equal", obs=np.ones_like(obs))
    plain = P.personFitHost(mu.CODE[model], Y, logT, X, rows, 61, "equal")
    for c in fu.COLS:
        assert np.array_equal(getattr(same, c), getattr(plain, c), equal_nan=True), c
    assert plain.nObs is None and np.all(same.nObs == 9)
    l_twin = P.marginalLogLikHost(mu.CODE[model], Y, logT, X, rows, 61, obs=obs)
    _, S = P.personFitHost(mu.CODE[model], Y, logT, X, rows, 61, "equal", obs=obs, with_S=True)
    assert S.shape == l_twin.shape


# ------------------------------------------------------------------------------------------------------------ calibration, flag rate, power: the twin alone
SIM_N, SIM_PLANTED = 2000, 400
MARGIN = 3.0 * np.sqrt(ALPHA * (1.0 - ALPHA) / SIM_N)          # three binomial standard deviations at the nominal rate: 0.0146
POWER_FACTOR, UNTOUCHED_MAX = 5.0, 3.0 * ALPHA


@pytest.mark.parametrize("J", [9, 20, 65])
@pytest.mark.parametrize("model", ["rtirt", "cross"])
def test_calibration_flag_rate_and_power_on_simulated_respondents(model, J):
    """Measured with this twin (N = 2000 clean, 400 planted, one row = the generating parameters, seeds 100 + J), J = 9 / 20 / 65:
         rtirt  KS p 0.24 / 0.74 / 0.41; clean pResp < 0.05: 0.030 / 0.047 / 0.034, pTime: 0.045 / 0.047 / 0.048;
                guessers 0.33 / 0.64 / 1.00 (their pTime 0.043 / 0.060 / 0.068); a 2 sigma shift on half the items 0.57 / 0.90 / 1.00 (their pResp 0.020 / 0.058 / 0.025)
         cross  KS p 0.37 / 0.75 / 0.54; clean 0.039 / 0.040 / 0.035 and 0.043 / 0.047 / 0.048;
                guessers 0.33 / 0.64 / 1.00 (pTime 0.048 / 0.060 / 0.107: the times depend on theta through rho, and guessing moves theta); shift 0.47 / 0.89 / 1.00
       pResp is conservative, as a posterior predictive p-value with an estimated theta is; pTime is exact given theta and sits at the nominal rate."""
    from scipy.stats import kstest
    P = fu.pkg()
    Y, logT, X, row, theta, zeta = fu.simulate(model, SIM_N, J, seed=100 + J)
    code = mu.CODE[model]

    def fit(Y, logT):
        parts = [P.personFitHost(code, Y[k:k + 500], logT[k:k + 500], None, row, 61) for k in range(0, len(Y), 500)]
        assert sum(p.nCoarse for p in parts) == 0
        return np.concatenate([p.pResp for p in parts]), np.concatenate([p.pTime for p in parts])

    r = row[0]
    rho = r[4 * J:5 * J] if model == "cross" else np.zeros(J)
    _, _, m0, m1, v = mu.law(model, r, J, 0, None)
    qf = np.array([fu.dense_quad(r[3 * J:4 * J], r[2 * J:3 * J], logT[i], rho, m0, m1, v, theta[i]) for i in range(SIM_N)])
    ks = kstest(P.twins.chi2TailHost(qf, J), "uniform")
    rate = lambda p: float(np.mean(p < ALPHA))
    pr, pt = fit(Y, logT)
    who = np.arange(SIM_PLANTED)
    gr, gt = fit(fu.plant_guessers(Y, who, 5)[:SIM_PLANTED], logT[:SIM_PLANTED])
    sr, st = fit(Y[:SIM_PLANTED], fu.plant_time_shift(logT, row, who)[:SIM_PLANTED])
    print(f"{model} J={J}: KS p {ks.pvalue:.3f}; clean pResp {rate(pr):.4f} pTime {rate(pt):.4f} (margin {MARGIN:.4f}); guessers {rate(gr):.3f} (pTime {rate(gt):.3f}); "
          f"shifted {rate(st):.3f} (pResp {rate(sr):.3f})")
    assert ks.pvalue > 0.01
    assert rate(pr) <= ALPHA + MARGIN and rate(pt) <= ALPHA + MARGIN
    assert rate(gr) >= POWER_FACTOR * max(rate(pr), 0.02) and rate(st) >= POWER_FACTOR * max(rate(pt), 0.02)
    assert rate(gt) <= UNTOUCHED_MAX and rate(sr) <= UNTOUCHED_MAX


# ------------------------------------------------------------------------------------------------------------ the preconditions of the GPU cases
def test_twin_conditioning_on_the_gpu_cases():
    """The float64 twin against the same twin in numpy.longdouble on every case of fit_util.CASES: measured 1.5e-13 (ltz at J = 1, where the cube root is steep
    near Qf = 0); fit_util.TWIN_COND pins it, and the kernel's tolerance is max(1e-10, 10 x TWIN_COND) = 1e-10."""
    worst, where = 0.0, None
    for case in fu.CASES:
        for w in fu.WEIGHTINGS:
            a, S = fu.twin(case, w)
            b, _ = fu.twin(case, w, True)
            e = max(fu.errors(a, b, fu.COLS).values())
            if e > worst:
                worst, where = e, (case, w)
        margin = float(np.min(np.abs(S - fu.COARSE_S)))
        assert margin >= fu.S_MARGIN, (case, margin)
    print(f"twin conditioning over {len(fu.CASES)} cases: {worst:.3g} at {where}; pinned {fu.TWIN_COND:.3g}, kernel tolerance {fu.KERNEL_TOL:.3g}")
    assert worst <= fu.TWIN_COND and fu.KERNEL_TOL == 1e-10


def test_the_cases_cover_what_they_name():
    for m in mu.MODELS:
        _, Y, logT, X, rows, Q, obs = fu.problem(("masked", m, 65))
        n = obs.sum(axis=1)
        assert {0, 1, 65 - 8, 65}.issubset(set(n.tolist())) and np.any((n > 25) & (n < 40))
        _, Y, _, _, rows, _, _ = fu.problem(("a8", m))
        assert np.all(rows[:, :9] == 8.0) and np.all(Y[5] == 1) and np.all(Y[6] == 0)
    for m in mu.MODELS[1:]:
        model, Y, logT, X, rows, Q, obs = fu.problem(("v0", m))
        v = mu.law(m, rows[0], 9, 3 if X is not None else 0, None if X is None else X[0])[4]
        assert v == 0.0 and Q == 127
    a8, _ = fu.twin(("a8", "rtirt"), "equal")
    assert a8.pResp[5] > 0.3 and np.all(np.isfinite(a8.lz))      # all correct against a = 8: nothing improbable, and no digit lost
    far, _ = fu.twin(("far", "cross"), "equal")
    assert far.pTime[3] == 0.0 and far.ltz[3] > 30.0              # 22 log-seconds off: beyond every tail


def test_end_to_end_seed_holds_with_margin_on_the_oracle_chain():
    """fit_util.aberrant_problem at E2E_SEED = 74, the twin on the oracle's chain (200 sweeps, 100 post-burn-in rows): the respondent with reversed responses has
    pResp 3.2e-4 against 0.095 for the next respondent and pTime 0.61; the respondent with shifted times has pTime 8.5e-59 against 0.114 and pResp 0.81.  (Seeds 70
    to 79 all hold the condition; the next respondent's pResp lies between 0.018 and 0.097 there.)"""
    P = fu.pkg()
    Y, logT, X, who_r, who_t = fu.aberrant_problem()
    init = pu.make_problem("rtirt", fu.E2E_N, fu.E2E_J, 3, seed=fu.E2E_SEED)[3]
    f = P.personFitHost(mu.CODE["rtirt"], Y, logT, X, fu.oracle_rows("rtirt", Y, logT, X, init, fu.E2E_SWEEPS, fu.E2E_BURNIN), 61)
    next_r, next_t = float(np.delete(f.pResp, who_r).min()), float(np.delete(f.pTime, who_t).min())
    print(f"pResp[{who_r}] {f.pResp[who_r]:.3g} (next {next_r:.3g}), pTime[{who_t}] {f.pTime[who_t]:.3g} (next {next_t:.3g}); pTime[{who_r}] {f.pTime[who_r]:.3f}, "
          f"pResp[{who_t}] {f.pResp[who_t]:.3f}")
    assert f.nCoarse == 0 and f.nRows == fu.E2E_SWEEPS - fu.E2E_BURNIN
    assert f.pResp[who_r] < 0.1 * next_r and f.pTime[who_t] < 0.1 * next_t              # the smallest, by a factor of ten
    assert f.pTime[who_r] > 4 * ALPHA and f.pResp[who_t] > 4 * ALPHA                    # and not flagged on the other component, with room


def test_rank_correlation_with_the_predictive_check_has_its_floor():
    """GibbsMlIrt: the sampler's theta is the model's own, so pResp tracks the subject ppp_mid of getPpcHost's response deviance on the same chain."""
    from scipy.stats import spearmanr
    import score_util as su
    import waic_util as wu
    P = fu.pkg()
    seen = []
    for seed in fu.PPC_SEEDS:
        Y, X, init = wu.spread_problem(seed=seed)
        M = wu.oracle_sampler("mlirt", Y, None, X, init, wu.SPREAD_ITER)
        f = P.personFitHost(mu.CODE["mlirt"], Y, None, X, su.mlirt_rows(M), 61)
        seen.append(float(spearmanr(P.getPpcHost(M, seed=1234).ppp_mid("subject", "ra"), f.pResp).correlation))
    print("rank correlation of pResp with the subject ppp_mid at five seeds: " + ", ".join(f"{r:.4f}" for r in seen) + f"; floor {fu.PPC_FLOOR:.4f}")
    assert abs(min(seen) - fu.PPC_MIN_MEASURED) <= 5e-4 and fu.PPC_FLOOR == fu.PPC_MIN_MEASURED - fu.PPC_MARGIN


# ------------------------------------------------------------------------------------------------------------ plumbing
def test_symbols_abi_and_words(tmp_path):
    P = fu.pkg()
    L = P._lib
    lib = L.load()
    header = open(os.path.join(pu.ROOT, "include", "ertirt.h")).read()
    for name in ("erm_get_person_fit", "erm_farm_get_person_fit", "erm_person_fit", "erm_person_fit_masked"):
        assert name in L.EXPORTS and hasattr(lib, name) and f"int {name}(" in header, name
    assert lib.erm_abi_version() == L.ABI_VERSION == 4 and "#define ERM_ABI_VERSION 4" in header
    assert L.FIT_COLUMNS == ("lz", "pResp", "ltz", "pTime", "rowEss", "coarse")
    assert "ERM_FIT_LZ = 0, ERM_FIT_P_RESP = 1, ERM_FIT_LTZ = 2, ERM_FIT_P_TIME = 3, ERM_FIT_ROW_ESS = 4, ERM_FIT_COARSE = 5, ERM_FIT_COLS = 6" in header
    for name in ("getPersonFit", "personFit", "personFitHost", "OutputPersonFit"):
        assert name in P.__all__ and hasattr(P, name)
    # the fifth pass's refusals, from its row of the header's table
    src = tmp_path / "words.cpp"
    src.write_text('#include <cstdio>\n#include "erm_item_pass.hpp"\nint main() { using namespace erm; static_assert(PASS_FIT == 4 && PASS_ITEM_FIT == 5 && N_ITEM_PASSES == 6, "");\n'
                   'printf("%s\\n%s\\n%s\\n%d %d\\n", ITEM_PASSES[PASS_FIT].noun, item_pass_on_shard(PASS_FIT).c_str(), item_pass_needs_rows(PASS_FIT).c_str(),\n'
                   'ITEM_PASSES[PASS_FIT].engine_rows, ITEM_PASSES[PASS_FIT].farm_rows);\n'
                   'return 0; }\n')
    exe = str(tmp_path / "words")
    subprocess.run(["g++", "-std=c++17", "-O1", "-fsanitize=undefined", "-fno-sanitize-recover=all", "-ftrapv", "-I", INC, str(src), "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split("\n")
    assert out[:4] == ["the person fit", "the person fit is not available on a shard (every subject's data must be resident on one device)",
                       "the person fit needs at least one post-burn-in row", "1 1"]
    # argument checks that touch no device
    with pytest.raises(ValueError, match="quantile"):
        P.personFit(L.MODEL_CROSSQR, np.zeros((2, 3)), np.zeros((2, 3)), None, np.zeros((1, 19)))
    with pytest.raises(ValueError, match="weighting"):
        P.personFit(L.MODEL_RTIRT, np.zeros((2, 3)), np.zeros((2, 3)), None, np.zeros((1, 20)), weighting="both")
    with pytest.raises(ValueError, match="odd"):
        P.personFit(L.MODEL_RTIRT, np.zeros((2, 3)), np.zeros((2, 3)), None, np.zeros((1, 20)), nodes=60)
    with pytest.raises(ValueError, match="quantile"):
        P.personFitHost(L.MODEL_LATENTQR, np.zeros((2, 3)), np.zeros((2, 3)), None, np.zeros((1, 20)))
    fr, ft = P.OutputPersonFit(pResp=np.array([0.01, 0.5, np.nan]), pTime=np.array([np.nan, 0.049, 0.05])).flagged()
    assert fr.tolist() == [True, False, False] and ft.tolist() == [False, True, False]

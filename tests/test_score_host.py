"""The scores of respondents on the CPU (include/ertirt.h: erm_get_scores).
  - csrc/erm_score.hpp, the header score_kernel includes, compiled by g++ with UndefinedBehaviorSanitizer into tests/score_check.cpp: (c0, c1, u) against a
    brute-force zeta grid in long double (1e-11 relative; J in {1, 7, 65}, v = 0 included, rho != 0 for Cross), the (M, S, S1, S2) merge over eight lanes against
    one-pass long-double sums over terms spanning -1400 ... 0, the weighted row accumulator against a two-pass long-double computation (weights spanning
    e^-1400 ... 1, one row, all rows identical: row_ess = n and a between-row variance of 0, exactly).
  - scoresHost, the numpy twin the GPU tests compare the kernel with, against independent code (score_util.quad_row): scipy.integrate.quad over theta of
    marginal_util.quad_l's integrand, zeta given theta by numpy Gaussian conditioning; five models, J = 7 and J = 50, Q = 61, three subjects x two rows, both
    weightings, no coarse unit.  Bound: the larger of 1e-9 and ten times the error measured at J = 50; errors of theta, zeta and cov relative to max(|ref|, 1).
    Measured on the CPU (max over the six columns, the subjects and both weightings):
        J = 50:  mlirt 3.4e-10, rtirt 7.1e-14, null 9.8e-13, cross 5.3e-7, latent 6.4e-9        J = 7:  mlirt 3.0e-12, rtirt 1.8e-12, null 1.2e-13, cross 2.3e-14, latent 2.2e-15
    so the bound is 5.3e-6.  As for the marginal log-likelihood (tests/test_marginal_host.py: 2.9e-10 for Cross at J = 50) the larger figures are the rule's own
    error, not rounding, on a posterior of standard deviation about one node spacing; Cross's largest is in thetaSd (theta 4.4e-8, zetaSd 5.4e-9): the rule's
    aliasing term, differentiated twice for the second moment, gains a factor of the order of (2 pi r^2)^2 over its share of the integral itself.
  - known answers: with Sigma_12 = 0 and rho = 0 an RtIrt row gives MlIrt's theta and thetaSd (1e-10), and zeta is the conjugate normal written out in numpy.
  - the narrow posterior of tests/test_marginal_host.py (J = 200, a = 2): coarse subjects at Q = 21 and none at Q = 201; thetaSd meets the bound against quad at
    Q = 201 and misses it at Q = 21.
  - agreement with the chain, GibbsMlIrt only (the one model whose theta draw is the model's own conditional), on waic_util.spread_problem() with the oracle chain:
    r = RMS_i (theta_score - Post.mean theta) / thetaSd <= 0.5 and |log(median sd of the draws / median thetaSd)| <= log 1.1.  Measured: r = 0.1348, ratio 1.0083.
  - the argument checks touch no device; the three symbols are in EXPORTS, in the header and in the library."""
import os
import subprocess
import types

import numpy as np
import pytest

import marginal_util as mu
import parity_util as pu
import score_util as su
import waic_util as wu

pkg = pu.ge.load_package()
SRC = os.path.join(pu.ROOT, "tests", "score_check.cpp")
INC = os.path.join(pu.ROOT, "extendedrtirtmodeling.jl_amd", "csrc")
QUAD_BOUND = 5.3e-6
WEIGHTINGS = ("equal", "likelihood")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("sc") / "score_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=undefined", "-fno-sanitize-recover=all", "-I", INC, SRC, "-o", out], check=True)
    return out


def test_closed_forms_equal_brute_force_without_undefined_behaviour(exe):
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert "failures 0" in r.stdout and "runtime error" not in r.stderr, r.stdout[-2000:] + r.stderr[-2000:]


def _kernel_x(model, X):
    return X if model in ("mlirt", "rtirt", "latent") else None


@pytest.mark.parametrize("J", [7, 50])
@pytest.mark.parametrize("model", mu.MODELS)
def test_twin_equals_quad(model, J):
    F, N, R = 3, 3, 2
    rows = mu.make_rows(model, J, F, R, seed=J)
    Y, logT, X = mu.make_data(model, N, J, F, seed=J)
    Xk = _kernel_x(model, X)
    worst = 0.0
    for weighting in WEIGHTINGS:
        got = pkg.scoresHost(mu.CODE[model], Y, logT, Xk, rows, 61, weighting)
        assert got.nCoarse == 0 and not np.any(got.coarse) and got.nRows == R and got.nNodes == 61      # the bound speaks of the rule where it claims to hold
        err = su.errors(got, su.quad_scores(model, Y, logT, Xk, rows, weighting), rt=model != "mlirt")
        print(f"{model} J={J} {weighting}: max err against quad " + ", ".join(f"{c} {e:.3g}" for c, e in err.items()))
        worst = max(worst, *err.values())
    print(f"{model} J={J}: worst {worst:.3g}")
    assert worst <= QUAD_BOUND


def test_rtirt_without_correlation_gives_mlirt_theta_and_the_conjugate_zeta():
    J, N, F, R, s22 = 9, 5, 3, 3, 0.36
    rows_m = mu.make_rows("mlirt", J, F, R, seed=61)
    Y, logT, X = mu.make_data("rtirt", N, J, F, seed=61)
    g = np.random.default_rng(62)
    b2 = 0.4 * g.normal(0, 1, (R, F + 1))                                    # beta[:, 2]: the mean of zeta
    lam_sig = np.hstack([4.0 + 0.3 * g.normal(0, 1, (R, J)), g.uniform(0.1, 0.6, (R, J))])
    rows_r = np.hstack([rows_m[:, :2 * J], lam_sig, rows_m[:, 4 * J:], b2, np.tile([1.0, 0.0, 0.0, s22], (R, 1))])
    # equal weights (under likelihood weights the response times move the weights of the rows, though not theta within a row)
    m = pkg.scoresHost(mu.CODE["mlirt"], Y, None, X, rows_m, 61)
    r = pkg.scoresHost(mu.CODE["rtirt"], Y, logT, X, rows_r, 61)
    assert np.max(np.abs(r.theta - m.theta)) <= 1e-10 and np.max(np.abs(r.thetaSd - m.thetaSd)) <= 1e-10
    assert np.all(np.isnan(m.zeta)) and np.all(np.isnan(m.zetaSd)) and np.all(np.isnan(m.cov)) and np.isnan(m.relZeta) and 0.0 < m.relTheta < 1.0
    assert np.all(np.isfinite(r.zeta)) and 0.0 < r.relZeta < 1.0
    # one row: zeta is the conjugate normal, independent of theta
    one = pkg.scoresHost(mu.CODE["rtirt"], Y, logT, X, rows_r[:1], 61)
    lam, sg = rows_r[0, 2 * J:3 * J], rows_r[0, 3 * J:4 * J]
    m0 = np.hstack([np.ones((N, 1)), X]) @ b2[0]
    P, R0 = np.sum(1.0 / sg), np.sum((lam[None, :] - logT) / sg[None, :], axis=1)
    assert np.max(np.abs(one.zeta - (m0 / s22 + R0) / (1.0 / s22 + P))) <= 1e-10
    assert np.max(np.abs(one.zetaSd - np.sqrt(1.0 / (1.0 / s22 + P)))) <= 1e-10 and np.max(np.abs(one.cov)) <= 1e-15 and np.all(one.rowEss == 1.0)


def test_narrow_posterior_is_flagged_and_cured_by_more_nodes():
    J, N = 200, 3
    rows = mu.make_rows("rtirt", J, 0, 2, seed=3, a=2.0)
    Y, logT, _ = mu.make_data("rtirt", N, J, 0, seed=3)
    ref = su.quad_scores("rtirt", Y, logT, None, rows, "equal")
    err = {}
    for Q in (21, 201):
        got = pkg.scoresHost(mu.CODE["rtirt"], Y, logT, None, rows, Q)
        err[Q] = float(np.max(np.abs(got.thetaSd - ref["thetaSd"]) / ref["thetaSd"]))
        print(f"Q={Q}: coarse units {got.nCoarse} of {N}, thetaSd max rel err against quad {err[Q]:.3g}")
        assert (got.nCoarse > 0) if Q == 21 else (got.nCoarse == 0)
        assert got.nCoarse == int(np.sum(got.coarse))
    assert err[201] <= QUAD_BOUND < err[21]


def test_scores_agree_with_the_chain_for_mlirt():
    """GibbsMlIrt's theta draw is the model's own conditional, so the Rao-Blackwell scores and the chain's draws estimate the same posterior.
    Measured on the CPU (oracle chain, 600 x 12, 200 sweeps, 100 post-burn-in): r = 0.1348, sd ratio 1.0083."""
    Y, X, init = wu.spread_problem()
    M = wu.oracle_sampler("mlirt", Y, None, X, init, wu.SPREAD_ITER)
    sc = pkg.scoresHost(0, Y, None, X, su.mlirt_rows(M), 61)
    draws = M.Post.ra[M.Cond.nBurnin:, :wu.SPREAD_N, 0]
    r, ratio = su.chain_agreement(sc, draws)
    print(f"r = {r:.4f}, median sd of the draws / median thetaSd = {ratio:.4f}; relTheta {sc.relTheta:.4f}, coarse {sc.nCoarse}")
    assert sc.nCoarse == 0 and np.all(sc.rowEss == wu.SPREAD_ITER // 2)
    assert r <= 0.5 and abs(np.log(ratio)) <= np.log(1.1)


def test_argument_checks_touch_no_device():
    Cond = pkg.setCond(nSubj=20, nItem=5, nFeat=1, nIter=10, nChain=1)
    for cls in (pkg.GibbsRtIrtCrossQr, pkg.GibbsRtIrtLatentQr):
        with pytest.raises(ValueError, match="getScores is not available .* quantile"):
            pkg.getScores(cls(Cond))
    M = pkg.GibbsRtIrt(Cond)
    for bad in (60, 1, 1027, -3, 61.5):
        with pytest.raises(ValueError, match="odd and in 3 .. 1025"):
            pkg.getScores(M, nodes=bad)
        with pytest.raises(ValueError, match="odd and in 3 .. 1025"):
            pkg.scoreRespondents(1, np.zeros((2, 3)), np.zeros((2, 3)), None, np.zeros((2, 18)), nodes=bad)
    with pytest.raises(ValueError, match=r"run sample! first \(getScores"):
        pkg.getScores(M)
    sharded = types.SimpleNamespace(_model=1, shard=(0, 2, 40, 0, None))
    with pytest.raises(ValueError, match="getScores is not available for a subject-sharded"):
        pkg.getScores(sharded)
    for fn in (pkg.scoreRespondents, pkg.scoresHost):
        with pytest.raises(ValueError, match="weighting"):
            fn(1, np.zeros((2, 3)), np.zeros((2, 3)), None, np.zeros((2, 18)), weighting="posterior")
        with pytest.raises(ValueError, match="quantile"):
            fn(pkg._lib.MODEL_CROSSQR, np.zeros((2, 3)), np.zeros((2, 3)), None, np.zeros((2, 19)))
    with pytest.raises(ValueError, match="columns"):
        pkg.scoresHost(1, np.zeros((2, 3)), np.zeros((2, 3)), None, np.zeros((2, 5)))
    with pytest.raises(ValueError, match="rows must be"):
        pkg.scoreRespondents(1, np.zeros((2, 3)), np.zeros((2, 3)), None, np.zeros((2, 5)))


def test_symbols_are_exported():
    lib, L = pkg._lib.load(), pkg._lib
    header = open(os.path.join(pu.ROOT, "include", "ertirt.h")).read()
    for name in ("erm_get_scores", "erm_farm_get_scores", "erm_score"):
        assert name in L.EXPORTS and hasattr(lib, name) and f"int {name}(" in header, name
    assert L.SCORE_COLUMNS == ("theta", "thetaSd", "zeta", "zetaSd", "cov", "rowEss", "coarse") and (L.SCORE_EQUAL, L.SCORE_LIKELIHOOD) == (0, 1)
    assert "ERM_SCORE_EQUAL = 0, ERM_SCORE_LIKELIHOOD = 1" in header and "ERM_SCORE_COARSE = 6" in header and lib.erm_abi_version() == 4
    assert L.score_weighting("equal") == 0 and L.score_weighting("likelihood") == 1 and L.score_weighting(1) == 1
    for name in ("getScores", "scoreRespondents", "scoresHost", "OutputScores"):
        assert name in pkg.__all__ and hasattr(pkg, name)

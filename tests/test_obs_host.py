"""Incomplete response patterns on the CPU (include/ertirt.h: erm_score_masked).
  - csrc/erm_obs.hpp, the header the caller-data source maker compacts the cells with, compiled by g++ with UndefinedBehaviorSanitizer and -ftrapv into
    tests/obs_check.cpp: offsets, item indices, responses and log-times (every bit) against numpy's nonzero for J in {1, 7, 8, 9, 65, 896} with the patterns all,
    none, last item only, only items >= 8, alternating and random side by side, the unobserved cells poisoned (Y = 255, logT = NaN); every refusal of the masked
    validation: a mask value above 1, a NaN in logT and a Y above 1 at an observed cell (the cell is named), the NaN before the bad Y wherever they stand.
  - the masked twin (marginalLogLikHost, scoresHost with obs=) against the unmasked twin on the subject's reduced data set (obs_util.reduced_subject): five models,
    both weightings, l and all score columns.  numpy's summation order changes with the length, so this is a tolerance, relative to max(|ref|, 1).  Measured on the
    CPU, the worst over J in {9, 65}, 12 subjects, 3 rows: l 2.9e-16 (mlirt, J = 9), scores 4.3e-15 (rtirt, J = 65); pinned at ten times that, 4.3e-14 -- three
    orders below the kernel-vs-twin 1e-10.
  - the masked twin against scipy.integrate.quad (score_util.quad_scores, test_score_host.py's independent reference, zeta by Gaussian conditioning) on the reduced
    data set: one masked subject per model, n_i = 7 of J = 50, Q = 61, both weightings.  A masked subject with 7 observed items IS a 7-item subject, so the bound is
    test_score_host.py's own, 5.3e-6.  Measured (the worst column, both weightings): mlirt 3.3e-13, rtirt 3.5e-11, null 1.8e-15, cross 2.4e-16,
    latent 8.0e-16.
  - n_i = 0: theta = the row average of mu, thetaSd^2 = mean(sd^2) + the between-row variance of mu, zeta = mean(m0 + m1 mu), zetaSd^2 = mean(v + m1^2 sd^2) + the
    between-row variance of m0 + m1 mu, l = log sum_q h phi(z_q).  The rule stands for N(0, 1) cut at +-6: the second moment it misses is 2 (6 phi(6) + Phi(-6)) =
    7.5e-8 and its aliasing error at h = 0.2 is far below that, so the moments are held to 1e-6 and l (against the rule's own total weight) to 1e-13.
  - plausibleValuesHost with obs= draws from the posterior scoresHost with obs= summarises: the same node rule, so equal nodes as the reduced subject; the cases of
    tests/test_gpu_incomplete.py (obs_util.PV_CASES) have no draw closer than pv_util.GAP_MIN.
  - observedMask; the three symbols are in EXPORTS, in the header and in the library; erm_abi_version() == 4; obs=None leaves the three twins' results identical."""
import os
import subprocess

import numpy as np
import pytest

import marginal_util as mu
import obs_util as ou
import parity_util as pu
import score_util as su

pkg = pu.ge.load_package()
SRC = os.path.join(pu.ROOT, "tests", "obs_check.cpp")
INC = os.path.join(pu.ROOT, "extendedrtirtmodeling.jl_amd", "csrc")
OK, BAD_MASK, NAN_LOGT, BAD_Y = 0, 1, 2, 3
TWIN_BOUND = 4.3e-14          # ten times the worst measured difference of the masked twin from the unmasked twin on the reduced data
QUAD_BOUND = 5.3e-6           # tests/test_score_host.py's
WEIGHTINGS = ("equal", "likelihood")
SCORE_COLS = su.COLS + ("coarse",)


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("obs") / "obs_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=undefined", "-fno-sanitize-recover=all", "-ftrapv", "-I", INC, SRC, "-o", out], check=True)
    return out


def _run(exe, tmp_path, obs, Y, logT):
    """obs_check on column-major copies of the arrays; returns its lines split into words."""
    N, J = obs.shape
    path = str(tmp_path / "cells.bin")
    with open(path, "wb") as f:
        f.write(np.array([N, J, logT is not None], dtype=np.int64).tobytes())
        f.write(np.asfortranarray(obs, dtype=np.uint8).tobytes(order="F"))
        f.write(np.asfortranarray(Y, dtype=np.uint8).tobytes(order="F"))
        if logT is not None:
            f.write(np.asfortranarray(logT, dtype=np.float64).tobytes(order="F"))
    r = subprocess.run([exe, path], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "runtime error" not in r.stderr, r.stdout[-2000:] + r.stderr[-2000:]
    return [line.split() for line in r.stdout.split("\n")[:-1]]


@pytest.mark.parametrize("rt", [True, False])
@pytest.mark.parametrize("J", [1, 7, 8, 9, 65, 896])
def test_compaction_equals_numpy_nonzero(exe, tmp_path, J, rt):
    N = 13                                                     # every pattern twice (the random ones differ), and one more "all"
    g = np.random.default_rng(J)
    obs = ou.masks(N, J, seed=J)
    Y = (g.uniform(size=(N, J)) < 0.5).astype(np.uint8)
    logT = 4.0 + g.normal(0, 0.7, (N, J)) if rt else None
    Yp, lp = ou.poison(Y, logT, obs)                           # what the header must never read
    out = _run(exe, tmp_path, obs, Yp, lp)
    assert out[0] == ["0", "-1"] and out[1] == ["0", "-1"], out[:2]
    n = obs.sum(axis=1)
    assert [int(v) for v in out[2][1:]] == [0] + list(np.cumsum(n))
    ii, jj = np.nonzero(obs)                                   # row-major: subject by subject, the items rising
    assert [int(v) for v in out[3][1:]] == list(jj)
    assert [int(v) for v in out[4][1:]] == list(Y[ii, jj])
    t = [float.fromhex(v) for v in out[5][1:]]
    assert t == (list(logT[ii, jj]) if rt else [])
    assert set(n) >= {0, 1, J} and (J < 9 or J - 8 in n)


def test_every_refusal_of_the_masked_validation(exe, tmp_path):
    N, J = 5, 9
    g = np.random.default_rng(3)
    obs = ou.masks(N, J, seed=3)                               # subject 0 all, 1 none, 2 the last item, 3 items >= 8, 4 alternating
    Y = (g.uniform(size=(N, J)) < 0.5).astype(np.uint8)
    logT = 4.0 + g.normal(0, 0.7, (N, J))
    cell = lambda i, j: str(j * N + i)
    bad = obs.copy(); bad[1, 4] = 2
    assert _run(exe, tmp_path, bad, Y, logT) == [[str(BAD_MASK), cell(1, 4)]]
    bad = obs.copy(); bad[4, 8] = 255; bad[0, 0] = 3           # the first in the walk (item by item) is named
    assert _run(exe, tmp_path, bad, Y, logT) == [[str(BAD_MASK), cell(0, 0)]]
    t = logT.copy(); t[2, 8] = np.nan                          # observed: subject 2's only cell
    assert _run(exe, tmp_path, obs, Y, t)[:2] == [["0", "-1"], [str(NAN_LOGT), cell(2, 8)]]
    t = logT.copy(); t[2, 7] = np.nan; t[1, :] = np.nan        # unobserved: not read
    assert _run(exe, tmp_path, obs, Y, t)[1] == ["0", "-1"]
    y = Y.copy(); y[4, 2] = 2
    assert _run(exe, tmp_path, obs, y, logT)[1] == [str(BAD_Y), cell(4, 2)]
    assert _run(exe, tmp_path, obs, y, None)[1] == [str(BAD_Y), cell(4, 2)]
    y = Y.copy(); y[4, 1] = 2; y[3, 0] = 7
    assert _run(exe, tmp_path, obs, y, logT)[1] == ["0", "-1"]
    y = Y.copy(); y[0, 0] = 2; t = logT.copy(); t[0, 8] = np.nan      # a NaN anywhere goes before a value outside the domain, as in the complete validation
    assert _run(exe, tmp_path, obs, y, t)[1] == [str(NAN_LOGT), cell(0, 8)]
    t = logT.copy(); t[0, 3] = np.inf                          # an infinity is no NaN: the complete validation lets it through as well
    assert _run(exe, tmp_path, obs, Y, t)[1] == ["0", "-1"]


# ------------------------------------------------------------------------------------------------------------ the masked twin
def _score_cols(sc, i=None):
    return {c: np.asarray(getattr(sc, c), dtype=np.float64) if i is None else np.asarray(getattr(sc, c), dtype=np.float64)[i:i + 1] for c in SCORE_COLS}


@pytest.mark.parametrize("J", [9, 65])
@pytest.mark.parametrize("model", mu.MODELS)
def test_masked_twin_equals_unmasked_twin_on_the_reduced_data(model, J):
    N, R, Q = 12, 3, 61
    Y, logT, X, rows, obs = ou.problem(model, N, J, R, seed=40 + J)
    Yp, lp = ou.poison(Y, logT, obs)
    code = mu.CODE[model]
    l = pkg.marginalLogLikHost(code, Yp, lp, X, rows, Q, obs=obs)
    sc = {w: pkg.scoresHost(code, Yp, lp, X, rows, Q, w, obs=obs) for w in WEIGHTINGS}
    assert np.array_equal(sc["equal"].nObs, obs.sum(axis=1)) and np.all(np.isfinite(l))
    worst_l = worst_s = 0.0
    for i in range(N):
        red = ou.reduced_subject(model, Y, logT, X, rows, obs, i)
        if red is None:
            continue
        worst_l = max(worst_l, ou.rel(l[:, i], pkg.marginalLogLikHost(code, *red, Q)[:, 0]))
        for w in WEIGHTINGS:
            ref, got = _score_cols(pkg.scoresHost(code, *red, Q, w)), _score_cols(sc[w], i)
            worst_s = max(worst_s, *(ou.rel(got[c], ref[c]) for c in SCORE_COLS))
    print(f"{model} J={J}: masked twin against the reduced data: l {worst_l:.3g}, scores {worst_s:.3g}")
    assert worst_l <= TWIN_BOUND and worst_s <= TWIN_BOUND


@pytest.mark.parametrize("model", mu.MODELS)
def test_masked_twin_equals_quad(model):
    J, F, R, Q = 50, 3, 2, 61
    rows = mu.make_rows(model, J, F, R, seed=7)
    Y, logT, X = mu.make_data(model, 1, J, F, seed=7)
    X = ou.kernel_x(model, X)
    obs = np.zeros((1, J), dtype=np.uint8)
    obs[0, np.random.default_rng(7).choice(J, size=7, replace=False)] = 1
    Yr, lr, Xr, rr = ou.reduced_subject(model, Y, logT, X, rows, obs, 0)
    Yp, lp = ou.poison(Y, logT, obs)
    worst = 0.0
    for weighting in WEIGHTINGS:
        got = pkg.scoresHost(mu.CODE[model], Yp, lp, X, rows, Q, weighting, obs=obs)
        assert got.nCoarse == 0 and got.nObs[0] == 7
        err = su.errors(got, su.quad_scores(model, Yr, lr, Xr, rr, weighting), rt=model != "mlirt")
        print(f"{model} n_i=7 of J={J} {weighting}: max err against quad " + ", ".join(f"{c} {e:.3g}" for c, e in err.items()))
        worst = max(worst, *err.values())
    assert worst <= QUAD_BOUND


@pytest.mark.parametrize("model", mu.MODELS)
def test_no_observed_cell_gives_the_population_law(model):
    J, F, R, Q, N = 9, 3, 4, 61, 3
    rows = mu.make_rows(model, J, F, R, seed=17)
    Y, logT, X = mu.make_data(model, N, J, F, seed=17)
    X = ou.kernel_x(model, X)
    obs = np.zeros((N, J), dtype=np.uint8)
    Yp, lp = ou.poison(Y, logT, obs)
    law = np.array([[mu.law(model, r, J, 0 if X is None else F, None if X is None else X[i]) for r in rows] for i in range(N)])      # (N, R, 5): mu, s11, m0, m1, v
    m, s11, m0, m1, v = (law[:, :, k] for k in range(5))
    h = 12.0 / (Q - 1)
    z = -6.0 + h * np.arange(Q)
    l = pkg.marginalLogLikHost(mu.CODE[model], Yp, lp, X, rows, Q, obs=obs)
    assert ou.rel(l, np.full((R, N), np.log(np.sum(h * np.exp(-0.5 * z * z) / np.sqrt(2 * np.pi))))) <= 1e-13
    sc = pkg.scoresHost(mu.CODE[model], Yp, lp, X, rows, Q, obs=obs)
    assert np.all(sc.nObs == 0) and sc.nCoarse == 0 and np.all(sc.rowEss == R)
    assert ou.rel(sc.theta, m.mean(axis=1)) <= 1e-6 and ou.rel(sc.thetaSd ** 2, s11.mean(axis=1) + m.var(axis=1)) <= 1e-6
    if model == "mlirt":
        assert np.all(np.isnan(sc.zeta)) and np.all(np.isnan(sc.zetaSd)) and np.all(np.isnan(sc.cov))
        return
    ez = m0 + m1 * m
    assert ou.rel(sc.zeta, ez.mean(axis=1)) <= 1e-6
    assert ou.rel(sc.zetaSd ** 2, (v + m1 * m1 * s11).mean(axis=1) + ez.var(axis=1)) <= 1e-6
    assert ou.rel(sc.cov, (m1 * s11).mean(axis=1) + ((m - m.mean(axis=1, keepdims=True)) * (ez - ez.mean(axis=1, keepdims=True))).mean(axis=1)) <= 1e-6


@pytest.mark.parametrize("model", ["mlirt", "rtirt", "cross"])
def test_masked_pv_twin_picks_the_reduced_subjects_nodes(model):
    N, J, R, Q, K = 6, 9, 3, 61, 5
    Y, logT, X, rows, obs = ou.problem(model, N, J, R, seed=51)
    Yp, lp = ou.poison(Y, logT, obs)
    pv, gap = pkg.plausibleValuesHost(mu.CODE[model], Yp, lp, X, rows, K, 20191, Q, with_gap=True, obs=obs)
    assert np.array_equal(pv.nObs, obs.sum(axis=1)) and np.all(np.isfinite(pv.theta)) and np.all(np.isfinite(pv.zeta)) == (model != "mlirt")
    for i in range(N):
        red = ou.reduced_subject(model, Y, logT, X, rows, obs, i)
        if red is None:
            continue
        ref = pkg.plausibleValuesHost(mu.CODE[model], *red, K, 20191, Q, i_base=i)
        sure = gap[i] > 1e-8
        assert np.array_equal(pv.node[i][sure], ref.node[0][sure])
        assert ou.rel(pv.theta[i][sure], ref.theta[0][sure]) <= 1e-10 and ou.rel(pv.zeta[i][sure], ref.zeta[0][sure]) <= 1e-10


@pytest.mark.parametrize("J,R,Q,K", ou.PV_CASES)
@pytest.mark.parametrize("model", mu.MODELS)
def test_masked_pv_cases_of_the_gpu_test_are_decidable(model, J, R, Q, K):
    import pv_util as pvu
    Y, logT, X, rows, obs = ou.pv_problem(model, J, R)
    _, gap = pkg.plausibleValuesHost(mu.CODE[model], Y, logT, X, rows, K, ou.PV_SEED, Q, with_gap=True, obs=obs)
    assert gap.min() >= pvu.GAP_MIN, gap.min()


# ------------------------------------------------------------------------------------------------------------ the surface
def test_observed_mask_helper():
    Y = np.array([[0.0, 1.0, np.nan], [1.0, 2.0, 0.0]])
    logT = np.array([[4.0, np.nan, 4.0], [np.inf, 4.0, 4.0]])
    assert np.array_equal(pkg.observedMask(Y), [[1, 1, 0], [1, 0, 1]]) and pkg.observedMask(Y).dtype == np.uint8
    assert np.array_equal(pkg.observedMask(Y, logT), [[1, 0, 0], [0, 0, 1]])
    with pytest.raises(ValueError, match="logT does not match"):
        pkg.observedMask(Y, logT[:1])


def test_obs_none_leaves_the_twins_as_they_were():
    Y, logT, X, rows, _ = ou.problem("rtirt", 5, 9, 3, seed=61)
    a, b = pkg.marginalLogLikHost(1, Y, logT, X, rows, 61), pkg.marginalLogLikHost(1, Y, logT, X, rows, 61, obs=None)
    assert np.array_equal(a, b)
    a, b = pkg.scoresHost(1, Y, logT, X, rows, 61, "likelihood"), pkg.scoresHost(1, Y, logT, X, rows, 61, "likelihood", obs=None)
    assert all(np.array_equal(getattr(a, c), getattr(b, c)) for c in SCORE_COLS) and a.nObs is None and b.nObs is None
    a, b = pkg.plausibleValuesHost(1, Y, logT, X, rows, 5, 11, 61), pkg.plausibleValuesHost(1, Y, logT, X, rows, 5, 11, 61, obs=None)
    assert np.array_equal(a.theta, b.theta) and np.array_equal(a.zeta, b.zeta) and np.array_equal(a.node, b.node) and a.nObs is None
    # all cells observed: the masked sums are the complete ones up to numpy's order of summation
    full, ref = pkg.scoresHost(1, Y, logT, X, rows, 61, "likelihood", obs=np.ones_like(Y)), pkg.scoresHost(1, Y, logT, X, rows, 61, "likelihood")
    assert all(ou.rel(getattr(full, c), getattr(ref, c)) <= TWIN_BOUND for c in SCORE_COLS) and np.all(full.nObs == 9)


def test_argument_checks_touch_no_device():
    Y, lt, rows = np.zeros((2, 3)), np.zeros((2, 3)), np.zeros((2, 18))
    for fn in (pkg.scoresHost, pkg.marginalLogLikHost, pkg.plausibleValuesHost):
        with pytest.raises(ValueError, match="obs does not match Y"):
            fn(1, Y, lt, None, rows, obs=np.ones((2, 4)))
        with pytest.raises(ValueError, match="obs must be 0/1"):
            fn(1, Y, lt, None, rows, obs=np.full((2, 3), 2))
    for fn in (pkg.scoreRespondents, pkg.drawPlausibleValues):
        with pytest.raises(ValueError, match="obs does not match Y"):
            fn(1, Y, lt, None, rows, obs=np.ones((3, 3)))
        with pytest.raises(ValueError, match="quantile"):
            fn(pkg._lib.MODEL_LATENTQR, Y, lt, None, rows, obs=np.ones((2, 3)))
    with pytest.raises(ValueError, match="without quantile weights only"):      # the quantile family's twin has no masked form
        next(pkg.twins._marginal_rows_host(pkg._lib.MODEL_LATENTQR, Y, lt, None, rows, 61, pkg.twins._quantile_rt_term(0.5), obs=np.ones((2, 3))))


def test_symbols_are_exported():
    lib, L = pkg._lib.load(), pkg._lib
    header = open(os.path.join(pu.ROOT, "include", "ertirt.h")).read()
    for name in ("erm_marginal_loglik_masked", "erm_score_masked", "erm_plausible_values_masked"):
        assert name in L.EXPORTS and hasattr(lib, name) and f"int {name}(" in header, name
    assert lib.erm_abi_version() == 4 and L.ABI_VERSION == 4
    assert "observedMask" in pkg.__all__ and hasattr(pkg, "observedMask")
    for out in (pkg.OutputScores(), pkg.OutputPv()):
        assert out.nObs is None

"""The item fit on the CPU: csrc/erm_ifit.hpp, the header item_fit_kernel and its reduction are built on, compiled by g++ with
UndefinedBehaviorSanitizer and -ftrapv into the stand-alone tests/ifit_check.cpp, and itemFitHost, the numpy twin the device is compared with in
tests/test_gpu_item_fit.py.
  - ifit_check self: the cell's values against long-double direct forms (|eta| up to 1e4, v = 0, n_i = 1, sig2t = 1e-8), ifit_finish's NaN rules, the reduction
    order as a partition at several chunk caps.
  - the twin against scipy's quadrature (ifit_util.quad_cells: fit_util.quad_row's integrand and break points, the conditional residual by numpy.linalg.solve):
    one subject's six cell means per model, J = 7 and 50, Q = 61, and n_i = 7 of 50 masked.  Measured worst 2.5e-8 (E[z^2] of cross at J = 50, where the
    rule's 61 nodes carry a posterior of sd 0.25; 2.5e-9 for d); pinned at 10 x.
  - the masked twin against the unmasked twin on every subject's reduced data set, to 1e-12.
  - calibration on fit_util.simulate data (RtIrt and Cross, J in {9, 20}, N = 2000, one row at the generating parameters): clean RESP_Z and RT_Z within +-4,
    infit and RT_MSQ within 1 +- 5 sqrt(2 / N).  Measured: |z| at most 2.54, infit 0.965 .. 1.027, RT_MSQ 0.932 .. 1.096: nothing had to be widened.
  - a new sample of 400 with one b_j + 1 and one lambda_j + sigma_j / 2 against the unchanged row: the planted item's |z| at least twice the largest other and
    at least 5.  Measured over four seeds: RESP_Z -7.1 .. -13.3 against at most 2.8, RT_Z 8.0 .. 11.4 against at most 3.6; infit of the shifted item 1.05 .. 1.69.
  - the preconditions of tests/test_gpu_item_fit.py: the twin's conditioning on its cases against numpy.longdouble, every S at least 0.1 from 2, and the
    end-to-end seed on the oracle's chain.
  - the plumbing: the three symbols, ABI 4, obs=None, the sixth pass's words."""
import os
import subprocess

import numpy as np
import pytest

import fit_util as fu
import ifit_util as iu
import marginal_util as mu
import obs_util as ou
import parity_util as pu

SRC = os.path.join(pu.ROOT, "tests", "ifit_check.cpp")
INC = os.path.join(pu.ROOT, "extendedrtirtmodeling.jl_amd", "csrc")
QUAD_MEASURED = 2.5e-8           # the twin's largest error against ifit_util.quad_cells over test_twin_equals_quadrature's cases
UBSAN = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=undefined", "-fno-sanitize-recover=all", "-ftrapv", "-I", INC]


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("ifit") / "ifit_check")
    subprocess.run(UBSAN + [SRC, "-o", out], check=True)
    return out


def test_header_against_long_double(exe):
    r = subprocess.run([exe, "self"], capture_output=True, text=True, timeout=300)
    print(r.stdout[-400:])
    assert r.returncode == 0 and "runtime error" not in r.stderr and r.stdout.split("\n")[-2] == "failures 0", r.stdout[-2000:] + r.stderr[-2000:]


@pytest.mark.parametrize("model", mu.MODELS)
def test_twin_equals_quadrature(model):
    P = iu.pkg()
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
            _, cells = P.itemFitHost(mu.CODE[model], Y, logT, Xk, rows, 61, obs=o, with_cells=True)
            if o is None:
                yi, ti, xi, ri, items = Y[0], None if logT is None else logT[0], None if Xk is None else Xk[0], rows, np.arange(J)
            else:
                red = ou.reduced_subject(model, Y, logT, Xk, rows, o, 0)
                yi, ti, xi, ri, items = red[0][0], None if red[1] is None else red[1][0], None if red[2] is None else red[2][0], red[3], np.flatnonzero(o[0])
                assert np.all(cells[0, o[0] == 0] == 0.0)
            ref = np.mean([iu.quad_cells(model, yi.astype(np.float64), ti, xi, r) for r in ri], axis=0)
            err = np.max(np.abs(cells[0, items] - ref) / np.maximum(np.abs(ref), 1.0), axis=0)
            for c, e in zip(iu.CELLS, err):
                worst[c] = max(worst.get(c, 0.0), float(e))
    print(f"{model}: itemFitHost's cells against quad, worst " + ", ".join(f"{c} {e:.3g}" for c, e in worst.items()))
    assert max(worst.values()) <= 10 * QUAD_MEASURED


@pytest.mark.parametrize("model", mu.MODELS)
def test_masked_twin_equals_the_twin_on_the_reduced_data(model):
    P = iu.pkg()
    Y, logT, X, rows, obs = ou.problem(model, 12, 9, 3, seed=29)
    Yp, lp = ou.poison(Y, logT, obs)
    got, cells = P.itemFitHost(mu.CODE[model], Yp, lp, X, rows, 61, obs=obs, with_cells=True)
    assert np.array_equal(got.nObs, obs.sum(axis=0))
    for i in range(12):
        red = ou.reduced_subject(model, Y, logT, X, rows, obs, i)
        if red is None:
            assert np.all(cells[i] == 0.0)
            continue
        _, one = P.itemFitHost(mu.CODE[model], *red[:3], red[3], 61, with_cells=True)
        items = np.flatnonzero(obs[i])
        assert np.all(np.abs(cells[i, items] - one[0]) <= 1e-12 * np.maximum(np.abs(one[0]), 1.0)), i
        assert np.all(cells[i, obs[i] == 0] == 0.0)
    same = P.itemFitHost(mu.CODE[model], Y, logT, X, rows, 61, obs=np.ones_like(obs))
    plain = P.itemFitHost(mu.CODE[model], Y, logT, X, rows, 61)
    for c in iu.COLS + ("nObs",):
        assert np.array_equal(getattr(same, c), getattr(plain, c), equal_nan=True), c
    # the items' sums are the sums of the cells: the columns from the table
    s, n = cells.sum(axis=0), obs.sum(axis=0)
    with np.errstate(invalid="ignore", divide="ignore"):
        assert np.allclose(got.infit, s[:, 1] / s[:, 2], rtol=1e-13, equal_nan=True) and np.allclose(got.outfit, s[:, 3] / n, rtol=1e-13, equal_nan=True)


# ------------------------------------------------------------------------------------------------------------ calibration and power: the twin alone
SIM_N, NEW_N = 2000, 400
MSQ_BAND = 5.0 * np.sqrt(2.0 / SIM_N)            # five standard deviations of a chi^2_1 mean over N: 0.158
Z_BAND, PLANT_B, PLANT_LAM = 4.0, 2, 5


@pytest.mark.parametrize("J", [9, 20])
@pytest.mark.parametrize("model", ["rtirt", "cross"])
def test_calibration_and_planted_drift_on_simulated_data(model, J):
    P = iu.pkg()
    Y, logT, X, row, theta, zeta = fu.simulate(model, SIM_N, J, seed=100 + J)
    f = P.itemFitHost(mu.CODE[model], Y, logT, None, row, 61)
    print(f"{model} J={J} clean: infit {f.infit.min():.3f} .. {f.infit.max():.3f}, outfit {f.outfit.min():.3f} .. {f.outfit.max():.3f}, RESP_Z {f.respZ.min():.2f} .. "
          f"{f.respZ.max():.2f}, RT_MSQ {f.rtMsq.min():.3f} .. {f.rtMsq.max():.3f}, RT_Z {f.rtZ.min():.2f} .. {f.rtZ.max():.2f}")
    assert f.nCoarse == 0 and np.all(f.nObs == SIM_N)
    assert np.all(np.abs(f.respZ) <= Z_BAND) and np.all(np.abs(f.rtZ) <= Z_BAND)
    assert np.all(np.abs(f.infit - 1.0) <= MSQ_BAND) and np.all(np.abs(f.rtMsq - 1.0) <= MSQ_BAND)
    fr, ft = f.flagged()
    assert not fr.any() and not ft.any()
    for seed in (1, 2, 3, 4):
        Y2, l2 = iu.drifted_sample(model, NEW_N, J, 500 + seed, row, item_b=PLANT_B, item_lam=PLANT_LAM)
        g = P.itemFitHost(mu.CODE[model], Y2, l2, None, row, 61)
        rz, tz = np.abs(g.respZ), np.abs(g.rtZ)
        print(f"   new sample {seed}: RESP_Z[{PLANT_B}] {g.respZ[PLANT_B]:.2f} (others at most {np.delete(rz, PLANT_B).max():.2f}), RT_Z[{PLANT_LAM}] {g.rtZ[PLANT_LAM]:.2f} "
              f"(others at most {np.delete(tz, PLANT_LAM).max():.2f}); infit[{PLANT_B}] {g.infit[PLANT_B]:.2f}")
        assert g.respZ[PLANT_B] < 0.0 and rz[PLANT_B] >= 5.0 and rz[PLANT_B] >= 2.0 * np.delete(rz, PLANT_B).max()      # harder than calibrated
        assert g.rtZ[PLANT_LAM] > 0.0 and tz[PLANT_LAM] >= 5.0 and tz[PLANT_LAM] >= 2.0 * np.delete(tz, PLANT_LAM).max()  # slower than calibrated
        fr, ft = g.flagged()
        assert fr[PLANT_B] and ft[PLANT_LAM]


# ------------------------------------------------------------------------------------------------------------ the preconditions of the GPU cases
def test_twin_conditioning_on_the_gpu_cases():
    """The float64 twin against the same twin in numpy.longdouble on every case of ifit_util.CASES: measured 4.9e-14 (the "far" case of latent: times 22 off);
    ifit_util.TWIN_COND pins it, and the kernels' tolerance is max(1e-10, 10 x TWIN_COND) = 1e-10."""
    worst, where = 0.0, None
    for case in iu.CASES:
        a, _, S = iu.twin(case)
        b, _, _ = iu.twin(case, True)
        e = max(iu.errors(a, b).values())
        if e > worst:
            worst, where = e, case
        margin = float(np.min(np.abs(S - iu.COARSE_S)))
        assert margin >= iu.S_MARGIN, (case, margin)
    print(f"twin conditioning over {len(iu.CASES)} cases: {worst:.3g} at {where}; pinned {iu.TWIN_COND:.3g}, kernel tolerance {iu.KERNEL_TOL:.3g}")
    assert worst <= iu.TWIN_COND and iu.KERNEL_TOL == 1e-10


def test_the_cases_cover_what_they_name():
    assert {c[2] for c in iu.CASES if c[0] == "shape"} == {1, 33, 257} and len([c for c in iu.CASES if c[0] == "shape"]) == 5 * 54
    for m in mu.MODELS:
        _, Y, logT, X, rows, Q, obs = iu.problem(("nobody", m))
        assert np.all(obs[:, 4] == 0) and obs.sum() > 0
        f, _, _ = iu.twin(("nobody", m))
        assert f.nObs[4] == 0 and all(np.isnan(getattr(f, c)[4]) for c in iu.COLS) and np.isfinite(f.infit[0])
        _, Y, logT, X, rows, Q, obs = iu.problem(("masked", m, 65))
        n = obs.sum(axis=1)
        assert {0, 1, 65 - 8, 65}.issubset(set(n.tolist())) and np.any((n > 25) & (n < 40))
    _, Y, _, _, rows, Q, _ = iu.problem(("wide", "rtirt"))
    assert Y.shape == (33, 896) and rows.shape[0] == 1
    a8, _, _ = iu.twin(("a8", "rtirt"))
    assert np.all(np.isfinite(a8.outfit)) and a8.outfit.max() > 1e3      # an all-wrong respondent against a = 8: outfit's tail, finite
    ml, _, _ = iu.twin(("shape", "mlirt", 33, 9, 3, 61))
    assert np.all(np.isnan(ml.rtMsq)) and np.all(np.isnan(ml.rtZ)) and np.all(np.isfinite(ml.infit))


def test_end_to_end_seed_holds_with_margin_on_the_oracle_chain():
    """ifit_util.e2e_problem at E2E_SEED = 76, the twin on the oracle's chain (200 sweeps, 100 post-burn-in rows): see ifit_util for the figures.  On the
    calibration sample itself every |RESP_Z| and |RT_Z| stays below 0.5: the item parameters were fitted to it."""
    P = iu.pkg()
    (Y, logT, X, init), (Y2, l2, X2) = iu.e2e_problem()
    rows = iu.e2e_oracle_rows()
    f = P.itemFitHost(mu.CODE["rtirt"], Y2, l2, X2, rows, 61)
    rz, tz = np.abs(f.respZ), np.abs(f.rtZ)
    fr, ft = rz[iu.E2E_ITEM_B] / np.delete(rz, iu.E2E_ITEM_B).max(), tz[iu.E2E_ITEM_LAM] / np.delete(tz, iu.E2E_ITEM_LAM).max()
    print(f"RESP_Z[{iu.E2E_ITEM_B}] {f.respZ[iu.E2E_ITEM_B]:.2f} (factor {fr:.2f}), RT_Z[{iu.E2E_ITEM_LAM}] {f.rtZ[iu.E2E_ITEM_LAM]:.2f} (factor {ft:.2f})")
    assert f.nCoarse == 0 and f.nRows == iu.E2E_SWEEPS - iu.E2E_BURNIN
    assert abs(fr - iu.E2E_RESP_FACTOR) <= 0.01 and abs(ft - iu.E2E_RT_FACTOR) <= 0.01
    assert f.respZ[iu.E2E_ITEM_B] < -5.0 and f.rtZ[iu.E2E_ITEM_LAM] > 5.0
    assert iu.E2E_RESP_FACTOR - iu.E2E_MARGIN >= 2.0 and iu.E2E_RT_FACTOR - iu.E2E_MARGIN >= 2.0
    own = P.itemFitHost(mu.CODE["rtirt"], Y, logT, X, rows, 61)
    assert np.all(np.abs(own.respZ) < 0.5) and np.all(np.abs(own.rtZ) < 0.5)


# ------------------------------------------------------------------------------------------------------------ plumbing
def test_symbols_abi_and_words(tmp_path):
    P = iu.pkg()
    L = P._lib
    lib = L.load()
    header = open(os.path.join(pu.ROOT, "include", "ertirt.h")).read()
    for name in ("erm_get_item_fit", "erm_farm_get_item_fit", "erm_item_fit"):
        assert name in L.EXPORTS and hasattr(lib, name) and f"int {name}(" in header, name
    assert lib.erm_abi_version() == L.ABI_VERSION == 4 and "#define ERM_ABI_VERSION 4" in header
    assert L.IFIT_COLUMNS == ("infit", "outfit", "respZ", "rtMsq", "rtZ", "nObs")
    assert "ERM_IFIT_INFIT = 0, ERM_IFIT_OUTFIT = 1, ERM_IFIT_RESP_Z = 2, ERM_IFIT_RT_MSQ = 3, ERM_IFIT_RT_Z = 4, ERM_IFIT_N_OBS = 5, ERM_IFIT_COLS = 6" in header
    for name in ("getItemFit", "itemFit", "itemFitHost", "OutputItemFit"):
        assert name in P.__all__ and hasattr(P, name)
    # the sixth pass's refusals, from its row of the header's table; the fifth keeps its noun
    src = tmp_path / "words.cpp"
    src.write_text('#include <cstdio>\n#include "erm_item_pass.hpp"\nint main() { using namespace erm; static_assert(PASS_FIT == 4 && PASS_ITEM_FIT == 5 && N_ITEM_PASSES == 6, "");\n'
                   'printf("%s\\n%s\\n%s\\n%d %d\\n%s\\n", ITEM_PASSES[PASS_ITEM_FIT].noun, item_pass_on_shard(PASS_ITEM_FIT).c_str(), item_pass_needs_rows(PASS_ITEM_FIT).c_str(),\n'
                   'ITEM_PASSES[PASS_ITEM_FIT].engine_rows, ITEM_PASSES[PASS_ITEM_FIT].farm_rows, ITEM_PASSES[PASS_FIT].noun);\n'
                   'return 0; }\n')
    exe = str(tmp_path / "words")
    subprocess.run(UBSAN + [str(src), "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split("\n")
    assert out[:5] == ["the item fit", "the item fit is not available on a shard (every subject's data must be resident on one device)",
                       "the item fit needs at least one post-burn-in row", "1 1", "the person fit"]
    # argument checks that touch no device
    with pytest.raises(ValueError, match="quantile"):
        P.itemFit(L.MODEL_CROSSQR, np.zeros((2, 3)), np.zeros((2, 3)), None, np.zeros((1, 19)))
    with pytest.raises(ValueError, match="odd"):
        P.itemFit(L.MODEL_RTIRT, np.zeros((2, 3)), np.zeros((2, 3)), None, np.zeros((1, 20)), nodes=60)
    with pytest.raises(ValueError, match="quantile"):
        P.itemFitHost(L.MODEL_LATENTQR, np.zeros((2, 3)), np.zeros((2, 3)), None, np.zeros((1, 20)))
    with pytest.raises(TypeError):
        P.itemFit(L.MODEL_RTIRT, np.zeros((2, 3)), np.zeros((2, 3)), None, np.zeros((1, 20)), weighting="likelihood")      # the rows count equally: no such argument
    fr, ft = P.OutputItemFit(infit=np.array([1.0, 1.4, np.nan, 1.0]), respZ=np.array([-3.5, 0.0, np.nan, 2.9]), rtMsq=np.array([1.0, 1.0, np.nan, 0.6]),
                             rtZ=np.array([0.0, 3.0, np.nan, 0.0])).flagged()
    assert fr.tolist() == [True, True, False, False] and ft.tolist() == [False, True, False, True]

"""Plausible values on the CPU (include/ertirt.h: erm_get_plausible_values).
  - csrc/erm_pv.hpp, the header pv_kernel includes, compiled by g++ with UndefinedBehaviorSanitizer into tests/pv_check.cpp, against the twin's own pieces (pvRow,
    pvGumbel, pvFinish) on hand-made values: the row index for K below, equal to and above n_rows, K = 1 and n_rows = 1; the key of the words 0 and 2^32 - 1 (and
    that g stays inside [-3.14, 22.88]); the merge being symmetric, its tie rule and the empty pair; eight lanes joined by the kernel's butterfly against numpy's
    argmax, ties included; the finish at V = 0 (theta = E exactly) and at u = 0 (zeta = c0 + c1 theta exactly), and with NaN for a model without zeta.
  - plausibleValuesHost, the numpy twin the GPU tests compare the kernel with, against scoresHost, which knows nothing of this feature's definition: five models,
    64 subjects x 9 items, 40 rows, Q = 61, K = 25 x 40 so that every row is used 25 times.
      mean            |mean_k draw - score| <= 6 sd / sqrt(K) for theta and zeta, every subject (the draws are stratified over the rows: conservative).
      second moments  |s^2 / sd^2 - 1| for theta and zeta, |sample cov - cov| / (thetaSd zetaSd).  Their spread was MEASURED on the twin over 24 other seeds
                      (seeds 1 .. 24, five models, 64 subjects each: 7680 subject-seeds per figure); largest seen: var_theta 0.166, var_zeta 0.160, cov 0.126.  The
                      bound is 1.5 x the largest: 0.25 for the variances, 0.19 for the covariance (a variance estimated from 1000 draws has a relative sd of
                      sqrt(2 / 1000) = 0.045, so the largest of 7680 lies near 4 sd; 1.5 x leaves room for the seed of the test being one more sample).
      per row         K = 2000 x 2 on two rows at Q = 9, where the node's cell is wide (h = 1.5): per row the mean of theta within 6 sqrt(V_s / 2000) of E_s and the
                      sample variance within VAR_ROW_BOUND of V_s.  Measured over 24 other seeds (16 subjects, five models): largest 0.148; bound 1.5 x = 0.22.  The jitter's variance
                      sd^2 h^2 / 12 is more than 0.30 V_s for every subject and row of the test (asserted), so the test fails if the shrink factor c is left out.
  - the argument checks touch no device; the three symbols are in EXPORTS, in the header and in the library; the ABI version is 4."""
import os
import subprocess
import types

import numpy as np
import pytest

import marginal_util as mu
import parity_util as pu
import pv_util as pvu

pkg = pu.ge.load_package()
SRC = os.path.join(pu.ROOT, "tests", "pv_check.cpp")
INC = os.path.join(pu.ROOT, "extendedrtirtmodeling.jl_amd", "csrc")
VAR_BOUND, COV_BOUND, VAR_ROW_BOUND = 0.25, 0.19, 0.22
SEED = 20191          # the test's seed; the spreads above were measured on seeds 1 .. 24


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("pv") / "pv_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=undefined", "-fno-sanitize-recover=all", "-I", INC, SRC, "-o", out], check=True)
    return out


def _run(exe, args, text=""):
    r = subprocess.run([exe, *map(str, args)], input=text, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "runtime error" not in r.stderr, r.stdout[-2000:] + r.stderr[-2000:]
    return r.stdout.split("\n")[:-1]


# ------------------------------------------------------------------------------------------------------------ the header against the twin's pieces
@pytest.mark.parametrize("K,n_rows", [(5, 40), (7, 7), (21, 7), (1, 40), (1, 1), (5, 1), (4096, 3), (4096, 8192), (3, 1 << 40)])
def test_row_index(exe, K, n_rows):
    got = np.array([int(v) for v in _run(exe, ["row", K, n_rows])])
    ref = np.array([((2 * k + 1) * n_rows) // (2 * K) for k in range(K)])                 # python integers: no overflow
    assert np.array_equal(got, ref) and np.array_equal(got, pkg.twins.pvRow(np.arange(K), K, n_rows))
    assert np.all(np.diff(got) >= 0) and got[0] >= 0 and got[-1] < n_rows
    if K <= n_rows:
        assert np.unique(got).size == K                                                   # distinct
    if K % n_rows == 0:
        assert np.array_equal(np.bincount(got, minlength=n_rows), np.full(n_rows, K // n_rows))      # K = m n_rows: each row m times


def test_gumbel_key_of_a_word(exe):
    words = [0, 1, 2 ** 31, 2 ** 32 - 2, 2 ** 32 - 1, 123456789]
    got = np.array([float.fromhex(v) for v in _run(exe, ["key", *words])])
    ref = pkg.twins.pvGumbel(np.array(words, dtype=np.uint64))
    assert np.max(np.abs(got - ref)) <= 1e-14 * 23.0
    assert abs(got[0] + np.log(33.0 * np.log(2.0))) <= 1e-13                              # u = 2^-33: g = -log(33 log 2) = -3.13
    assert abs(got[4] - 33.0 * np.log(2.0)) <= 1e-6 and got[4] < 22.88                    # u = 1 - 2^-33: g = 33 log 2 - O(2^-34) = 22.87
    assert np.all(np.diff(got[:5]) > 0)


def test_merge_is_symmetric_and_the_smaller_node_wins_a_tie(exe):
    h = float.hex
    cases = [(1.5, 3, 2.5, 9, 9), (2.5, 3, 1.5, 9, 3), (0.25, 12, 0.25, 4, 4), (0.25, 4, 0.25, 12, 4), (-700.0, 0, -700.0, 60, 0),
             (0.0, -1, -5.0, 7, 7), (-5.0, 7, 0.0, -1, 7), (0.0, -1, 0.0, -1, -1), (-0.0, 5, 0.0, 2, 2)]
    out = _run(exe, ["merge"], "".join(f"{h(ka)} {qa} {h(kb)} {qb}\n" for ka, qa, kb, qb, _ in cases))
    for (ka, qa, kb, qb, want), line in zip(cases, out):
        k1, q1, k2, q2 = line.split()
        assert int(q1) == int(q2) == want, (ka, qa, kb, qb, line)
        if want >= 0:
            assert k1 == k2 and float.fromhex(k1) == (ka if want == qa else kb)           # both orders: the same pair, bit for bit


@pytest.mark.parametrize("Q", [3, 9, 61, 129])
def test_eight_lanes_pick_what_argmax_picks(exe, Q):
    g = np.random.default_rng(Q)
    for trial in range(4):
        key = g.normal(0, 3, Q)
        if trial >= 2:
            key[g.integers(0, Q, 3)] = key.max() + 1.0                                     # ties at the top, on whatever lanes they fall
        out = _run(exe, ["pick"], f"{Q}\n" + "\n".join(float.hex(float(k)) for k in key) + "\n")
        assert [int(v) for v in out[0].split()] == [int(np.argmax(key))] * 8, (Q, trial)


def test_finish_of_a_draw(exe):
    h = float.hex
    g = np.random.default_rng(7)
    rows = []
    for n in range(12):
        E, V, mu_, sd = g.normal(), g.uniform(0.05, 0.8), g.normal(0, 0.3), g.uniform(0.7, 1.3)
        c0, c1, u = g.normal(), g.normal(0, 0.3), g.uniform(0.01, 0.3)
        Q = int(g.choice([9, 61, 129]))
        if n == 0: V = 0.0                    # a row whose posterior sits on one node
        if n == 1: u = 0.0                    # v = 0: zeta is a function of theta
        rows.append((E, V, mu_, sd, c0, c1, u, int(g.integers(0, Q)), Q, 0 if n == 2 else 1, *[int(w) for w in g.integers(0, 2 ** 32, 3)]))
    rows.append((0.3, 0.2, 0.0, 1.0, 0.1, 0.2, 0.3, 4, 9, 1, 0, 0, 2 ** 32 - 1))          # the words at their ends
    rows.append((0.3, 0.2, 0.0, 1.0, 0.1, 0.2, 0.3, 4, 9, 1, 2 ** 32 - 1, 2 ** 32 - 1, 0))
    out = _run(exe, ["finish"], "".join(" ".join(h(v) if isinstance(v, float) else str(v) for v in r) + "\n" for r in rows))
    assert len(out) == len(rows)
    for r, line in zip(rows, out):
        E, V, mu_, sd, c0, c1, u, q, Q, has_zeta, w0, w1, w2 = r
        th, ze = (float.fromhex(v) if "nan" not in v else np.nan for v in line.split())
        W = lambda w: np.array([w], dtype=np.uint64)
        rt, rz = (float(v[0]) for v in pkg.twins.pvFinish(E, V, mu_, sd, c0, c1, u, q, 12.0 / (Q - 1), W(w0), W(w1), W(w2)))
        assert abs(th - rt) <= 1e-14 * max(abs(rt), 1.0), r
        if not has_zeta:
            assert np.isnan(ze)
        else:
            assert abs(ze - rz) <= 1e-13 * max(abs(rz), 1.0), r
        if V == 0.0:
            assert th == E
        if u == 0.0:
            assert ze == c0 + c1 * th
        # theta* lies inside the node's cell, and the shrink towards E only moves it nearer to E
        centre, half = mu_ + sd * (-6.0 + q * 12.0 / (Q - 1)), 0.5 * sd * 12.0 / (Q - 1)
        assert min(E, centre - half) - 1e-12 <= th <= max(E, centre + half) + 1e-12


# ------------------------------------------------------------------------------------------------------------ the twin against scoresHost
@pytest.mark.parametrize("model", mu.MODELS)
def test_twin_has_the_moments_of_the_scores(model):
    N, J, F, R, m = 64, 9, 3, 40, 25
    Y, logT, X, rows = pvu.problem(model, N, J, F, R, seed=71)
    sc = pkg.scoresHost(mu.CODE[model], Y, logT, X, rows, 61)
    pv = pkg.plausibleValuesHost(mu.CODE[model], Y, logT, X, rows, m * R, SEED, 61)
    assert pv.theta.shape == pv.zeta.shape == pv.node.shape == (N, m * R) and (pv.nRows, pv.nNodes, pv.seed) == (R, 61, SEED)
    assert np.array_equal(pv.coarse, sc.coarse) and pv.nCoarse == sc.nCoarse              # every row is used: the flags are the scores'
    rt = model != "mlirt"
    assert np.all(np.isfinite(pv.theta)) and (np.all(np.isfinite(pv.zeta)) if rt else np.all(np.isnan(pv.zeta)))
    fig = pvu.moment_figures(pv, sc, rt)
    print(f"{model}: " + ", ".join(f"{k} {v:.3g}" for k, v in fig.items()))
    assert fig["z_theta"] <= 6.0 and fig["var_theta"] <= VAR_BOUND
    if rt:
        assert fig["z_zeta"] <= 6.0 and fig["var_zeta"] <= VAR_BOUND and fig["cov"] <= COV_BOUND


@pytest.mark.parametrize("model", mu.MODELS)
def test_every_row_has_its_own_mean_and_variance(model):
    N, J, F, m, Q = 16, 9, 3, 2000, 9
    Y, logT, X, rows = pvu.problem(model, N, J, F, 2, seed=73)
    pv, (rk, E, V) = pkg.plausibleValuesHost(mu.CODE[model], Y, logT, X, rows, 2 * m, SEED, Q, with_rows=True)
    assert np.array_equal(rk, np.repeat([0, 1], m))
    # the power of the test: the jitter's variance, were it left in, exceeds the bound for every subject and row
    sd = np.ones(2) if model == "mlirt" else np.sqrt(rows[:, -4])
    jitter = (sd * 12.0 / (Q - 1)) ** 2 / 12.0
    assert np.all(jitter[None, [0, -1]] / V[:, [0, -1]] > VAR_ROW_BOUND)
    fig = pvu.row_figures(pv.theta, rk, E, V)
    print(f"{model}: per row z {fig['z']:.3g}, var {fig['var']:.3g}; jitter / V at least {float(np.min(jitter[None, [0, -1]] / V[:, [0, -1]])):.3g}")
    assert fig["z"] <= 6.0 and fig["var"] <= VAR_ROW_BOUND


def test_twin_is_a_function_of_the_subject_the_rows_and_the_seed():
    Y, logT, X, rows = pvu.problem("rtirt", 12, 9, 3, 7, seed=75)
    whole = pkg.plausibleValuesHost(1, Y, logT, X, rows, 5, SEED)
    part = pkg.plausibleValuesHost(1, Y[4:9], logT[4:9], X[4:9], rows, 5, SEED, i_base=4)
    other = pkg.plausibleValuesHost(1, Y, logT, X, rows, 5, SEED + 1)
    moved = pkg.plausibleValuesHost(1, Y[4:9], logT[4:9], X[4:9], rows, 5, SEED)          # the same data at another index: other draws
    for c in ("theta", "zeta", "node"):
        assert np.array_equal(getattr(part, c), getattr(whole, c)[4:9]), c
    assert not np.array_equal(other.theta, whole.theta) and not np.array_equal(moved.theta, part.theta)
    assert np.array_equal(pkg.twins.pvRow(np.arange(5), 5, 7), [0, 2, 3, 4, 6])


@pytest.mark.parametrize("model,J,Q,K,R", pvu.CASES)
def test_the_device_cases_are_decidable(model, J, Q, K, R):
    """The condition under which tests/test_gpu_plausible_values.py demands equal nodes: at its seeds no draw of the twin has its two best keys closer than GAP_MIN."""
    Y, logT, X, rows = pvu.case_problem(model, J, R)
    pv, gap = pkg.plausibleValuesHost(mu.CODE[model], Y, logT, X, rows, K, pvu.CASE_SEED, Q, with_gap=True)
    print(f"{model} J={J} Q={Q} K={K} R={R}: smallest gap {gap.min():.3g}, coarse {pv.nCoarse}")
    assert gap.shape == (pvu.CASE_N, K) and gap.min() >= pvu.GAP_MIN


# ------------------------------------------------------------------------------------------------------------ the surface
def test_argument_checks_touch_no_device():
    Cond = pkg.setCond(nSubj=20, nItem=5, nFeat=1, nIter=10, nChain=1)
    for cls in (pkg.GibbsRtIrtCrossQr, pkg.GibbsRtIrtLatentQr):
        with pytest.raises(ValueError, match="getPlausibleValues is not available .* quantile"):
            pkg.getPlausibleValues(cls(Cond))
    M = pkg.GibbsRtIrt(Cond)
    args = (1, np.zeros((2, 3)), np.zeros((2, 3)), None, np.zeros((2, 18)))
    for bad in (60, 1, 1027, -3, 61.5):
        with pytest.raises(ValueError, match="odd and in 3 .. 1025"):
            pkg.getPlausibleValues(M, nodes=bad)
        for fn in (pkg.drawPlausibleValues, pkg.plausibleValuesHost):
            with pytest.raises(ValueError, match="odd and in 3 .. 1025"):
                fn(*args, nodes=bad)
    for bad in (0, -1, 4097, 2.5, True):
        with pytest.raises(ValueError, match="K must be an integer in 1 .. 4096"):
            pkg.getPlausibleValues(M, K=bad)
        for fn in (pkg.drawPlausibleValues, pkg.plausibleValuesHost):
            with pytest.raises(ValueError, match="K must be"):
                fn(*args, K=bad)
    for bad in (-1, 1 << 64, 0.5):
        with pytest.raises(ValueError, match="seed must be an integer"):
            pkg.getPlausibleValues(M, seed=bad)
        for fn in (pkg.drawPlausibleValues, pkg.plausibleValuesHost):
            with pytest.raises(ValueError, match="seed must be"):
                fn(*args, seed=bad)
    with pytest.raises(ValueError, match=r"run sample! first \(getPlausibleValues"):
        pkg.getPlausibleValues(M)
    sharded = types.SimpleNamespace(_model=1, shard=(0, 2, 40, 0, None))
    with pytest.raises(ValueError, match="getPlausibleValues is not available for a subject-sharded"):
        pkg.getPlausibleValues(sharded)
    for fn in (pkg.drawPlausibleValues, pkg.plausibleValuesHost):
        with pytest.raises(ValueError, match="quantile"):
            fn(pkg._lib.MODEL_CROSSQR, np.zeros((2, 3)), np.zeros((2, 3)), None, np.zeros((2, 19)))
    with pytest.raises(ValueError, match="columns"):
        pkg.plausibleValuesHost(1, np.zeros((2, 3)), np.zeros((2, 3)), None, np.zeros((2, 5)))
    with pytest.raises(ValueError, match="rows must be"):
        pkg.drawPlausibleValues(1, np.zeros((2, 3)), np.zeros((2, 3)), None, np.zeros((2, 5)))


def test_symbols_are_exported():
    lib, L = pkg._lib.load(), pkg._lib
    header = open(os.path.join(pu.ROOT, "include", "ertirt.h")).read()
    for name in ("erm_get_plausible_values", "erm_farm_get_plausible_values", "erm_plausible_values"):
        assert name in L.EXPORTS and hasattr(lib, name) and f"int {name}(" in header, name
    assert lib.erm_abi_version() == 4 == L.ABI_VERSION and "#define ERM_ABI_VERSION 4" in header
    assert (L.PV_DRAWS, L.PV_DRAWS_MAX, L.PV_SITE) == (5, 4096, 16) and "ERM_PV_DRAWS_DEFAULT = 5, ERM_PV_DRAWS_MAX = 4096" in header
    for name in ("getPlausibleValues", "drawPlausibleValues", "plausibleValuesHost", "OutputPv"):
        assert name in pkg.__all__ and hasattr(pkg, name)
    assert "OutputPv(shape=None" in repr(pkg.OutputPv())

"""Marginal PSIS-LOO on the CPU (include/ertirt.h: erm_get_marginal_loo).
  - csrc/erm_psis.hpp, the header psis_kernel includes, compiled by g++ with UndefinedBehaviorSanitizer into tests/psis_check.cpp and swept over S in
    {25, 26, 224, 225, 226, 4097, 8192} x the columns of psis_util (Gaussian, one row 700 below the rest, a lattice with ties across the cutoff, a constant column,
    a heavy tail, a constant tail, exceedances over 300 orders of magnitude): M, G, the Inf pattern of k^ exactly, k^, sigma, elpd and every smoothed normalised
    log-weight against psisLooHost, the numpy twin written from the papers.  Bound, per S: 64 x the largest difference between the twin in fp64 and the same twin
    in np.longdouble over these very inputs (fourteen columns, two of every kind), floor 1e-13 -- measured bounds 2.8e-13 (S = 26) ... 7.1e-11 (S = 4097, the
    column whose ratios are about 1e-304); the header's largest deviation from the twin was 3.2e-16 ... 9.5e-14.
  - k^ forced to exactly 0: psis_smooth takes the limit form.
  - the tail-length integers (M, G, the index of x*) against the float formulas for every S in 25 .. 8192.
  - invariants of the twin: l + const moves elpd by const and leaves k^; a permutation of the rows of a tie-free unit leaves k^ and elpd; constant l gives
    k^ = +Inf and elpd = l.
  - recovery of k (see test_twin_recovers_the_shape_of_a_generalised_pareto_tail).
  - getLooMarginal's argument checks that touch no device; the three symbols in EXPORTS and in the library; compareWaic on two OutputLoo."""
import os
import subprocess
import types

import numpy as np
import pytest

import parity_util as pu
import psis_util as ps

pkg = pu.ge.load_package()
SRC = os.path.join(pu.ROOT, "tests", "psis_check.cpp")
INC = os.path.join(pu.ROOT, "extendedrtirtmodeling.jl_amd", "csrc")
N_CPU = 14                                   # two columns of every kind


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("psis") / "psis_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=undefined", "-fno-sanitize-recover=all", "-I", INC, SRC, "-o", out], check=True)
    return out


def _run(exe, args, stdin=None):
    r = subprocess.run([exe, *args], input=stdin, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "runtime error" not in r.stderr, r.stdout[-2000:] + r.stderr[-2000:]
    return r.stdout.split("\n")


def _unit(exe, l):
    out = _run(exe, ["unit"], f"{l.size}\n" + "\n".join(float(v).hex() for v in l) + "\n")
    head = out[0].split()
    return int(head[0]), int(head[1]), [float.fromhex(h) for h in head[2:]], np.array([float.fromhex(h) for h in out[1:1 + l.size]])


def test_tail_length_integers_equal_the_float_formulas(exe):
    rows = np.array([[int(v) for v in line.split()] for line in _run(exe, ["tail"]) if line])
    S = np.arange(25, 8193)
    assert np.array_equal(rows[:, 0], S)
    M = np.minimum(np.ceil(S / 5.0), np.ceil(3.0 * np.sqrt(S))).astype(int)
    assert np.array_equal(rows[:, 1], M) and M.min() == 5 and M.max() == 272
    assert np.array_equal(rows[:, 2], 30 + np.floor(np.sqrt(M)).astype(int)) and rows[:, 2].max() == 46
    assert np.array_equal(rows[:, 3], np.floor(M / 4.0 + 0.5).astype(int))
    at = {int(s): int(m) for s, m in zip(S, M)}
    assert (at[224], at[225], at[226]) == (45, 45, 46) and 224 / 5.0 < 3 * np.sqrt(224) and 225 / 5.0 == 3 * np.sqrt(225) and 226 / 5.0 > 3 * np.sqrt(226)      # the arms cross at 225
    assert (at[25], at[8192]) == (5, 272)


@pytest.mark.parametrize("S", ps.S_CPU)
def test_header_equals_twin(exe, S):
    L = ps.table(S, N=N_CPU)
    bound = max(ps.FLOOR, 64.0 * ps.twin_difference(L))
    host, lw, sigma = pkg.psisLooHost(L, with_lw=True, with_fit=True)
    worst = 0.0
    for u in range(N_CPU):
        M, G, (khat, sg, elpd), lwc = _unit(exe, L[:, u])
        assert M == host.tailLen == ps.tail_len(S) and G == 30 + int(np.floor(np.sqrt(M)))
        e = max(ps.rel([khat], [host.khat[u]]), ps.rel([sg], [sigma[u]]), ps.rel([elpd], [host.elpd_u[u]]), ps.rel(lwc, lw[:, u]))
        worst = max(worst, e)
        assert e <= bound, (ps.kind_of(u), u, e, bound)
    kinds = {ps.kind_of(u): host.khat[u] for u in range(7)}
    assert np.isinf(kinds["constant"]) and np.isinf(kinds["consttail"]) and np.isfinite(kinds["gauss"]) and np.isfinite(kinds["span300"])
    print(f"S={S}: worst rel err header / twin {worst:.3g}, bound {bound:.3g}")


@pytest.mark.parametrize("M,expc,sigma", [(5, 0.25, 0.5), (272, 1e-300, 3.0), (45, 0.9, 0.01)])
def test_smoothing_at_k_exactly_zero_is_the_limit_form(exe, M, expc, sigma):
    got = np.array([float.fromhex(h) for h in _run(exe, ["smooth", str(M), repr(expc), "0", repr(sigma)]) if h])
    p = (np.arange(1, M + 1) - 0.5) / M
    want = np.minimum(0.0, np.log(expc - sigma * np.log1p(-p)))
    assert got.size == M and np.all(np.isfinite(got)) and ps.rel(got, want) <= 1e-15 * 8
    near = np.array([float.fromhex(h) for h in _run(exe, ["smooth", str(M), repr(expc), "1e-9", repr(sigma)]) if h])
    assert ps.rel(near, got) <= 1e-7                          # and it is the limit: k = 1e-9 differs by O(k)


def test_twin_invariants():
    g = np.random.default_rng(5)
    L = g.normal(-40.0, 2.0, (300, 6))
    a = pkg.psisLooHost(L)
    b = pkg.psisLooHost(L + 17.25)
    assert np.max(np.abs(b.elpd_u - a.elpd_u - 17.25)) <= 1e-12 * 40 and np.max(np.abs(b.khat - a.khat)) <= 1e-12
    c = pkg.psisLooHost(L[g.permutation(300)])
    assert np.max(np.abs(c.elpd_u - a.elpd_u)) <= 1e-12 * 40 and np.max(np.abs(c.khat - a.khat)) <= 1e-12
    k = pkg.psisLooHost(np.full((64, 3), -7.5))
    assert np.all(np.isposinf(k.khat)) and np.array_equal(k.elpd_u, np.full(3, -7.5)) and np.all(np.abs(k.nEff - 64.0) <= 1e-12 * 64) and k.nBadK == 3
    assert np.all(np.abs(k.p_u) <= 1e-14)


K_BOUNDS = {0.2: 0.321, 0.5: 0.429, 0.9: 0.490}


@pytest.mark.parametrize("k", sorted(K_BOUNDS))
def test_twin_recovers_the_shape_of_a_generalised_pareto_tail(k):
    """Ratios r = 1 + X, X ~ scipy.stats.genpareto(k), S = 4000 (M = 190): by threshold stability the exceedances over any cutoff are generalised Pareto with the
    same shape.  200 seeds per k.  Measured largest |k^ - k|: 0.2134 at k = 0.2, 0.2858 at k = 0.5, 0.3265 at k = 0.9 (means +0.028, +0.003, -0.020; standard
    deviations 0.077, 0.105, 0.120: the estimator's spread at M = 190, about (1 + k) / sqrt(M), and the pull of its weak prior towards 0.5).  Bounds: 1.5 x the
    largest deviation seen -- 0.321, 0.429, 0.490."""
    from scipy.stats import genpareto
    cols = [-np.log(1.0 + genpareto.rvs(k, size=4000, random_state=np.random.default_rng(1000 * seed + int(k * 10)))) for seed in range(200)]
    d = pkg.psisLooHost(np.stack(cols, axis=1)).khat - k
    print(f"k={k}: largest |khat - k| {np.max(np.abs(d)):.4f}, mean {d.mean():+.4f}, sd {d.std():.4f}; bound {K_BOUNDS[k]}")
    assert np.max(np.abs(d)) <= K_BOUNDS[k] and abs(d.mean()) < 0.05


def test_argument_checks_touch_no_device():
    Cond = pkg.setCond(nSubj=20, nItem=5, nFeat=1, nIter=100, nChain=1)
    for cls in (pkg.GibbsRtIrtCrossQr, pkg.GibbsRtIrtLatentQr):
        with pytest.raises(ValueError, match="quantile"):
            pkg.getLooMarginal(cls(Cond))
        with pytest.raises(ValueError, match="quantile"):
            pkg.getLooMarginalHost(cls(Cond))
    M = pkg.GibbsRtIrt(Cond)
    for bad in (60, 1, 1027, -3, 61.5):
        with pytest.raises(ValueError, match="odd and in 3 .. 1025"):
            pkg.getLooMarginal(M, nodes=bad)
    with pytest.raises(ValueError, match="run sample! first"):
        pkg.getLooMarginal(M)
    sharded = types.SimpleNamespace(_model=1, shard=(0, 2, 40, 0, None))
    with pytest.raises(ValueError, match="subject-sharded"):
        pkg.getLooMarginal(sharded)
    few = pkg.GibbsRtIrt(pkg.setCond(nSubj=20, nItem=5, nFeat=1, nIter=48, nChain=1))          # 24 post-burn-in rows
    with pytest.raises(ValueError, match="25 .. 8192"):
        pkg.getLooMarginal(few)
    many = pkg.GibbsRtIrt(pkg.setCond(nSubj=20, nItem=5, nFeat=1, nIter=8194, nChain=2))       # 8194 rows
    with pytest.raises(ValueError, match="25 .. 8192"):
        pkg.getLooMarginal(many)
    for S in (24, 8193):
        with pytest.raises(ValueError, match="25 .. 8192"):
            pkg.psisLooHost(np.zeros((S, 2)))
        with pytest.raises(ValueError, match="25 .. 8192"):
            pkg.psisLoo(np.zeros((S, 2)))


def test_symbols_are_exported_and_compare_accepts_two_loo_results():
    lib = pkg._lib.load()
    for name in ("erm_get_marginal_loo", "erm_farm_get_marginal_loo", "erm_psis_loo"):
        assert name in pkg._lib.EXPORTS and hasattr(lib, name), name
    g = np.random.default_rng(9)
    A = pkg.psisLooHost(g.normal(-30.0, 1.0, (100, 40)))
    B = pkg.psisLooHost(g.normal(-31.0, 1.0, (100, 40)))
    c = pkg.compareWaic(A, B)
    d = A.elpd_u - B.elpd_u
    assert c == pkg.compareLoo(A, B) and c["nUnits"] == 40 and c["elpd_diff"] == float(np.sum(d)) and c["se_diff"] == float(np.sqrt(40 * np.var(d, ddof=1)))
    with pytest.raises(ValueError, match="OutputLoo"):
        pkg.compareWaic(A, pkg.OutputWaic(lppd_u=np.zeros(40), p_u=np.zeros(40), unit=None))

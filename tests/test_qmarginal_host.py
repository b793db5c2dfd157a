"""LatentQr's marginal WAIC on the CPU (include/ertirt.h: erm_get_quantile_marginal_waic): theta, zeta and the quantile weight nu integrated out.
  1. csrc/erm_qmarginal.hpp, the header marginal_kernel<LATENTQR> includes, compiled by g++ with UndefinedBehaviorSanitizer into tests/qmarginal_check.cpp:
     qmarg_log_ndtr against logl(0.5L * erfcl(-x / sqrtl(2))) on x = -140 (1/64) 9 and at the joins of its three arms; qmarg_T against a brute-force long-double zeta
     integral split at m, J in {1, 7, 65}.  Bound at every point: the larger of 1e-11 and ten times the reference's own error there, which the check measures
     (logPhi: the long-double value against __float128; T: 400 against 200 panels).  Measured: logPhi 1.1e-14 against __float128, the long-double reference's own
     error 2.1e-19 for x < 0 and up to 0.17 for x >= 0 (log of a number next to 1: there the __float128 value, 1e-11, is the check that bites);
     T 7.9e-15, the reference's own 3.3e-18 -- so the bound is 1e-11 wherever the reference is good.
  2. quantileMarginalLogLikHost, the numpy twin the GPU tests compare the kernel with, against independent code: scipy's dblquad over (theta, zeta) split at the kink
     of zeta's law at J = 7, Q = 61, and quad over theta of exp(B + log N + T by brute-force quad over zeta) at J = 50; S >= 2 for every unit used.
     Bound: the larger of 1e-9 and ten times the error measured at J = 50.  Measured (max relative error): J = 50: 4.0e-12 at q = 0.5, 4.0e-12 at q = 0.85 (the rule's
     own error: fifty items narrow theta's posterior); J = 7: 2.9e-16.  So the bound is 1e-9.
  3. the extremes against 60-digit mpmath: m = +-30 (beta0 = +-30), s in {0.001, 50}, one subject's logT 22 off, J = 1.  Bound: ten times the measured error.
     Measured: beta0 = 30, s = 0.001: 7.6e-15;  30, 50: 1.8e-14;  -30, 0.001: 3.1e-14;  -30, 50: 1.5e-14.  The header's host build (the figures the GPU test takes
     its fallback bound from) is printed beside them.
  4. a narrow posterior (J = 200, a_j = 2): coarse units at Q = 21, none at Q = 201.
  5. q is plumbed with its sign: on data drawn from the model at q = 0.85 (N = 300, J = 7), sum_i [l_i(0.85) - l_i(0.15)] exceeds 2 sd(diff) sqrt(N); measured
     13.0, 12.5, 11.7 times that standard error over seeds 1, 2, 3 (printed).
  6. getWaicMarginalQr's argument checks that touch no device; the five symbols in EXPORTS, in the header and in the library; the ABI version stays 4."""
import os
import re
import subprocess
import types

import numpy as np
import pytest

import parity_util as pu
import qmarginal_util as qu

pkg = pu.ge.load_package()
SRC = os.path.join(pu.ROOT, "tests", "qmarginal_check.cpp")
INC = os.path.join(pu.ROOT, "extendedrtirtmodeling.jl_amd", "csrc")
QUAD_BOUND = 1e-9
EXTREME_BOUND = {"beta0=30 s=0.001": 7.6e-14, "beta0=30 s=50": 1.8e-13, "beta0=-30 s=0.001": 3.1e-13, "beta0=-30 s=50": 1.5e-13}      # ten times the measured
SYMBOLS = ("erm_get_quantile_marginal_waic", "erm_get_quantile_marginal_loo", "erm_farm_get_quantile_marginal_waic", "erm_farm_get_quantile_marginal_loo",
           "erm_quantile_marginal_loglik")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("qmg") / "qmarginal_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=undefined", "-fno-sanitize-recover=all", "-I", INC, SRC, "-o", out, "-lquadmath"], check=True)
    return out


def test_header_equals_brute_force_without_undefined_behaviour(exe):
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(r.stdout[-1500:])
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert "failures 0" in r.stdout and "runtime error" not in r.stderr, r.stdout[-2000:] + r.stderr[-2000:]


@pytest.mark.parametrize("J,q", [(7, 0.85), (50, 0.5), (50, 0.85)])
def test_twin_equals_independent_integration(J, q):
    F, N, R = 3, (2 if J == 7 else 3), 2
    rows = qu.make_rows(J, F, R, seed=J)
    Y, logT, X = qu.make_data(N, J, F, seed=J)
    L, S = pkg.quantileMarginalLogLikHost(qu.CODE, Y, logT, X, rows, q, 61, with_S=True)
    assert L.shape == (R, N) and np.all(S >= 2.0)                      # no unit is coarse: the bound speaks of the rule where it claims to hold
    ref = qu.dblquad_l if J == 7 else qu.quad_l
    want = np.array([[ref(Y[i], logT[i], X[i], rows[s], q) for i in range(N)] for s in range(R)])
    err = np.max(np.abs(L - want) / np.abs(want))
    print(f"J={J} q={q}: max rel err against {ref.__name__} {err:.3g}; S >= {S.min():.3g}")
    assert err <= QUAD_BOUND


def test_extremes_equal_mpmath(exe):
    for name, Y, logT, rows, q in qu.extreme_cases():
        N, R = Y.shape[0], rows.shape[0]
        L = pkg.quantileMarginalLogLikHost(qu.CODE, Y, logT, None, rows, q, 61)
        want = np.array([[qu.mp_l(Y[i], logT[i], None, rows[s], q, 61) for i in range(N)] for s in range(R)])
        built = np.array([[qu.host_build_l(exe, Y[i], logT[i], None, rows[s], q, 61) for i in range(N)] for s in range(R)])
        err, err_b = np.max(np.abs(L - want) / np.abs(want)), np.max(np.abs(built - want) / np.abs(want))
        print(f"{name}: twin against mpmath {err:.3g}, the header's host build against mpmath {err_b:.3g}; l in [{L.min():.6g}, {L.max():.6g}]")
        assert np.all(np.isfinite(L)) and err <= EXTREME_BOUND[name]


def test_narrow_posterior_is_flagged_and_cured_by_more_nodes():
    rows = qu.make_rows(200, 0, 2, seed=3, a=2.0)
    Y, logT, _ = qu.make_data(3, 200, 0, seed=3)
    for Q in (21, 201):
        L, S = pkg.quantileMarginalLogLikHost(qu.CODE, Y, logT, None, rows, 0.85, Q, with_S=True)
        coarse = int(np.sum(np.any(S < 2.0, axis=0)))
        print(f"Q={Q}: coarse units {coarse} of 3")
        assert (coarse > 0) if Q == 21 else (coarse == 0)


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_level_is_plumbed_with_its_sign(seed):
    N = 300
    Y, logT, row = qu.simulate(N, 7, 0.85, seed)
    d = pkg.quantileMarginalLogLikHost(qu.CODE, Y, logT, None, row, 0.85)[0] - pkg.quantileMarginalLogLikHost(qu.CODE, Y, logT, None, row, 0.15)[0]
    se = np.std(d, ddof=1) * np.sqrt(N)
    print(f"seed {seed}: sum of l(0.85) - l(0.15) = {d.sum():.2f} = {d.sum() / se:.2f} se")
    assert d.sum() > 2.0 * se


def test_argument_checks_touch_no_device():
    Cond = pkg.setCond(nSubj=20, nItem=5, nFeat=1, nIter=10, nChain=1, qRt=0.85)
    for cls in (pkg.GibbsMlIrt, pkg.GibbsRtIrt, pkg.GibbsRtIrtNull, pkg.GibbsRtIrtCross, pkg.GibbsRtIrtLatent):
        for fn in (pkg.getWaicMarginalQr, pkg.getLooMarginalQr, pkg.getWaicMarginalQrHost, pkg.getLooMarginalQrHost):
            with pytest.raises(ValueError, match="no quantile weights"):
                fn(cls(Cond))
    for fn in (pkg.getWaicMarginalQr, pkg.getLooMarginalQr, pkg.getWaicMarginalQrHost, pkg.getLooMarginalQrHost):
        with pytest.raises(ValueError, match="asymmetric Laplace"):
            fn(pkg.GibbsRtIrtCrossQr(Cond))
    M = pkg.GibbsRtIrtLatentQr(Cond)
    for bad in (60, 1, 1027, -3, 61.5):
        with pytest.raises(ValueError, match="odd and in 3 .. 1025"):
            pkg.getWaicMarginalQr(M, nodes=bad)
    with pytest.raises(ValueError, match="run sample! first"):
        pkg.getWaicMarginalQr(M)
    with pytest.raises(ValueError, match="25 .. 8192"):
        pkg.getLooMarginalQr(M)                                        # 10 iterations, 5 of them burn-in: too few rows for PSIS
    sharded = types.SimpleNamespace(_model=qu.CODE, shard=(0, 2, 40, 0, None))
    with pytest.raises(ValueError, match="subject-sharded"):
        pkg.getWaicMarginalQr(sharded)
    with pytest.raises(ValueError, match="columns"):
        pkg.quantileMarginalLogLikHost(qu.CODE, np.zeros((2, 3)), np.zeros((2, 3)), None, np.zeros((2, 5)), 0.5)
    for bad in (0.0, 1.0, -0.2, float("nan")):
        with pytest.raises(ValueError, match="qRt"):
            pkg.quantileMarginalLogLikHost(qu.CODE, np.zeros((2, 3)), np.zeros((2, 3)), None, np.ones((2, 18)), bad)
    with pytest.raises(ValueError, match="LatentQr only"):
        pkg.quantileMarginalLogLikHost(6, np.zeros((2, 3)), np.zeros((2, 3)), None, np.ones((2, 18)), 0.5)
    # the entries that were there keep refusing the quantile samplers
    with pytest.raises(ValueError, match="quantile"):
        pkg.getWaicMarginal(M)


def test_symbols_are_exported_and_the_abi_version_stays():
    L = pkg._lib
    lib = L.load()
    hdr = open(os.path.join(pu.ROOT, "include", "ertirt.h")).read()
    for name in SYMBOLS:
        assert name in L.EXPORTS and hasattr(lib, name) and re.search(r"\bint " + name + r"\(", hdr), name
    assert lib.erm_abi_version() == L.ABI_VERSION == 4 and "#define ERM_ABI_VERSION 4" in hdr
    assert L.item_trace_width(qu.CODE, 9, 3) == L.item_trace_width(L.MODEL_LATENT, 9, 3) == 45
    assert L.QUANTILE_MARGINAL_MODELS == (L.MODEL_LATENTQR,) and L.MODEL_LATENTQR not in L.MARGINAL_MODELS

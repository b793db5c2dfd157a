"""The marginal WAIC on the CPU (include/ertirt.h: erm_get_marginal_waic).
  - csrc/erm_marginal.hpp, the header marginal_kernel includes, compiled by g++ with UndefinedBehaviorSanitizer into tests/marginal_check.cpp: T(theta) against a
    brute-force zeta grid in long double (1e-11 relative; J in {1, 7, 65}, v = 0 included, rho != 0 for Cross), the population law against the table written out,
    the (M, S) merge over eight lanes against a one-pass log-sum over terms spanning -1400 ... 0, a degenerate rule, the nodes.
  - marginalLogLikHost, the numpy twin the GPU tests compare the kernel with, against independent code: scipy.integrate.quad over theta of
    exp(B + log N(theta) + multivariate_normal.logpdf(t, ..., diag(sig2t) + v 1 1')), all five models, J = 7 and J = 50, Q = 61.
    Bound: the larger of 1e-9 and ten times the error measured at J = 50.  Measured (max relative error over 3 subjects x 2 rows):
        J = 50:  mlirt 4.5e-13, rtirt 6.1e-16, null 2.5e-15, cross 2.9e-10, latent 4.0e-12        J = 7:  mlirt 1.6e-14, rtirt 6.2e-15, null 3.2e-16, cross 4.4e-16, latent 5.5e-16
    so the bound is 2.9e-9.  The larger figures are the rule's own error, not rounding: the trapezoid rule on a Gaussian posterior of standard deviation r h is off
    by about 2 exp(-2 pi^2 r^2) -- 3e-10 at r = 1.07 (Sigma_p[1,1] up to 1.69 makes h up to 0.26, and fifty cross-relations narrow the posterior of theta).
  - a narrow posterior (J = 200, a_j = 2: standard deviation about 0.08): coarse units at Q = 21 (h = 0.6) and none at Q = 201 (h = 0.06); the Q = 201 value
    equals quad's, the Q = 21 value does not.
  - on waic_util.spread_problem() with the oracle chain, the marginal elpd prefers 2pl over 1pl by more than 2 se_diff -- with room to spare (printed).
  - getWaicMarginal's argument checks that touch no device; the three symbols in EXPORTS and in the library."""
import os
import subprocess
import types

import numpy as np
import pytest

import marginal_util as mu
import parity_util as pu
import waic_util as wu

pkg = pu.ge.load_package()
SRC = os.path.join(pu.ROOT, "tests", "marginal_check.cpp")
INC = os.path.join(pu.ROOT, "extendedrtirtmodeling.jl_amd", "csrc")
QUAD_BOUND = 2.9e-9


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("mg") / "marginal_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=undefined", "-fno-sanitize-recover=all", "-I", INC, SRC, "-o", out], check=True)
    return out


def test_closed_forms_equal_brute_force_without_undefined_behaviour(exe):
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert "failures 0" in r.stdout and "runtime error" not in r.stderr, r.stdout[-2000:] + r.stderr[-2000:]


def test_T_known_answer(exe):
    """One item, sig2t = 1, v = 3, m = 0, d = 2: t ~ N(lambda, 1 + 3), so T = log N(2; 0, 4)."""
    r = subprocess.run([exe, "T", "1", "2", "0", "4", "0", "0", "0", "1", "0", "0", "3", "0.7"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    want = -0.5 * np.log(2 * np.pi * 4.0) - 0.5 * 4.0 / 4.0
    assert abs(float(r.stdout.split("=")[1]) - want) <= 1e-15


@pytest.mark.parametrize("J", [7, 50])
@pytest.mark.parametrize("model", mu.MODELS)
def test_twin_equals_quad(model, J):
    F, N, R = 3, 3, 2
    rows = mu.make_rows(model, J, F, R, seed=J)
    Y, logT, X = mu.make_data(model, N, J, F, seed=J)
    Xk = X if model in ("mlirt", "rtirt", "latent") else None
    L, S = pkg.marginalLogLikHost(mu.CODE[model], Y, logT, Xk, rows, 61, with_S=True)
    assert L.shape == (R, N) and np.all(S >= 2.0)                      # no unit is coarse: the bound speaks of the rule where it claims to hold
    ref = np.array([[mu.quad_l(model, Y[i], None if logT is None else logT[i], None if Xk is None else Xk[i], rows[s]) for i in range(N)] for s in range(R)])
    err = np.max(np.abs(L - ref) / np.abs(ref))
    print(f"{model} J={J}: max rel err against quad {err:.3g}")
    assert err <= QUAD_BOUND


def test_narrow_posterior_is_flagged_and_cured_by_more_nodes():
    J, N = 200, 3
    rows = mu.make_rows("rtirt", J, 0, 2, seed=3, a=2.0)
    Y, logT, _ = mu.make_data("rtirt", N, J, 0, seed=3)
    ref = np.array([[mu.quad_l("rtirt", Y[i], logT[i], None, rows[s]) for i in range(N)] for s in range(2)])
    err = {}
    for Q in (21, 201):
        L, S = pkg.marginalLogLikHost(mu.CODE["rtirt"], Y, logT, None, rows, Q, with_S=True)
        coarse = int(np.sum(np.any(S < 2.0, axis=0)))
        err[Q] = np.max(np.abs(L - ref) / np.abs(ref))
        print(f"Q={Q}: coarse units {coarse} of {N}, max rel err against quad {err[Q]:.3g}")
        assert (coarse > 0) if Q == 21 else (coarse == 0)
    assert err[201] <= QUAD_BOUND and err[21] > 1e-5


def _mlirt_rows(M):
    """Item-trace rows of a GibbsMlIrt sampler-shaped namespace (waic_util.as_sampler): a, b, lambda = 0, sig2t = 1 | beta, post-burn-in."""
    C, P = M.Cond, M.Post
    N, J = C.nSubj, C.nItem
    ra, qr = P.ra[C.nBurnin:, :, 0], P.qr[C.nBurnin:, :, 0]
    return np.hstack([ra[:, N:N + J], ra[:, N + J:N + 2 * J], np.zeros((ra.shape[0], J)), np.ones((ra.shape[0], J)), qr])


def test_marginal_elpd_prefers_2pl_on_spread_discriminations():
    Y, X, init = wu.spread_problem()
    fit = {}
    for onepl in (False, True):
        M = wu.oracle_sampler("mlirt", Y, None, X, init, wu.SPREAD_ITER, onepl=onepl)
        L, S = pkg.marginalLogLikHost(0, Y, None, X, _mlirt_rows(M), 61, with_S=True)
        fit[onepl] = pkg.twins.waicFromLogLik(L, nNodes=61, nCoarse=int(np.sum(np.any(S < 2.0, axis=0))))
        assert fit[onepl].nCoarse == 0 and fit[onepl].unit == "subject-marginal"
    cmp = pkg.compareWaic(fit[False], fit[True])
    print(f"2pl elpd {fit[False].elpd:.2f} (p {fit[False].pWaic:.2f}), 1pl elpd {fit[True].elpd:.2f} (p {fit[True].pWaic:.2f}); diff {cmp['elpd_diff']:.2f}, se_diff {cmp['se_diff']:.2f}")
    assert cmp["elpd_diff"] > 2.0 * cmp["se_diff"]


def test_argument_checks_touch_no_device():
    Cond = pkg.setCond(nSubj=20, nItem=5, nFeat=1, nIter=10, nChain=1)
    for cls in (pkg.GibbsRtIrtCrossQr, pkg.GibbsRtIrtLatentQr):
        with pytest.raises(ValueError, match="quantile"):
            pkg.getWaicMarginal(cls(Cond))
        with pytest.raises(ValueError, match="quantile"):
            pkg.getWaicMarginalHost(cls(Cond))
    M = pkg.GibbsRtIrt(Cond)
    for bad in (60, 1, 1027, -3, 61.5):
        with pytest.raises(ValueError, match="odd and in 3 .. 1025"):
            pkg.getWaicMarginal(M, nodes=bad)
    with pytest.raises(ValueError, match="run sample! first"):
        pkg.getWaicMarginal(M)
    sharded = types.SimpleNamespace(_model=1, shard=(0, 2, 40, 0, None))
    with pytest.raises(ValueError, match="subject-sharded"):
        pkg.getWaicMarginal(sharded)
    with pytest.raises(ValueError, match="columns"):
        pkg.marginalLogLikHost(1, np.zeros((2, 3)), np.zeros((2, 3)), None, np.zeros((2, 5)))


def test_symbols_are_exported():
    lib = pkg._lib.load()
    for name in ("erm_get_marginal_waic", "erm_farm_get_marginal_waic", "erm_marginal_loglik"):
        assert name in pkg._lib.EXPORTS and hasattr(lib, name), name
    L = pkg._lib
    assert [L.item_trace_width(m, 9, 3) for m in L.MARGINAL_MODELS] == [40, 48, 42, 49, 45]      # 4 J + (F+1 | 2(F+1)+4 | 2+4 | J+4 | F+2+4)
    assert L.marginal_nodes(None) == L.marginal_nodes(0) == 61 and L.marginal_nodes(127) == 127
